"""The case table of the kinematics tests: poses for armenv_fk and (pose, target, configuration) triples for one IK update, drawn from
one seeded stream per block, with the 40-digit reference values and the derived bounds of tests/kin_ref.py beside them.

build() returns the flat dict of arrays that tests/tools/gen_kin_ref_cases.py writes to tests/golden/kin_ref_cases.npz:
  families                    names; every block's `family` array indexes into it
  fk.<path>.q / .family       poses [n,7] of a chain path (kin_ref.CHAIN_PATHS)
  fk.<path>.<prec>.pos_hi/_lo, .quat_hi/_lo, .E_p, .E_q, .case, .case_margin, .use
                              reference (float64 hi + lo pairs), bounds, getRotation case; `use` = 0 on the families an engine is
                              not specified for (the f32 sincos at 1e7 and 1e9 rad: F32_UNSPECIFIED)
  ik.<group>.q / .tgt / .family / .cfg / .path
                              cfg = [lambda, max_dtheta, residual, exit_mode, angle_f32, tip xyz, target quaternion xyzw, dv];
                              dv != 0 (the `step` group): .tgt holds the env step's f32 ACTION and the target is p(q) + dv a
  ik.<group>.<prec>.q_out_hi/_lo, .count, .E_q_out, .E_trig, .trig_hi/_lo, .cond (sigma_max, sigma_min, kappa, G, G_lin, G_ang, 1 - w^2,
                              max |dtheta| before the scale-back, smallest LDL^T pivot, w, wrap taken), .dist (wrap distance, its error, exit distance,
                              its error, case margin), .terms (the five summands of the solve's bound and the angular error)

Conditions are asserted HERE, on the CPU, when the table is built (check() runs them again on a loaded table): every family is
non-empty and has the property it is named after, and every case keeps its distance from the two discontinuities the bound cannot
absorb -- the wrap of the angle at pi and the exit test of exit mode 1 -- by more than 4 times the kernel's bound at that point.  A
drawn case that does not is redrawn from the same stream; a constructed one that does not is an error.

Why the chosen t of the quaternion is >= 1: for trace > 0, t = 1 + trace; otherwise t = 1 - trace + 2 m_ii with m_ii the largest
diagonal element, m_ii >= trace / 3, so t >= 1 - trace / 3 >= 1.  A frame within its error of a case boundary may take the other case,
whose t is then within that error of the same value.
"""
import math

import numpy as np

import kin_ref as K
from kin_fixture import STEP_DV

SEED = 20261020
FAMILIES = ("random", "quat_boundary", "settled_frame", "limits", "quadrant", "zero", "large_1e5", "large_1e7", "large_1e9",      # FK
            "w_half", "w_to_one", "settled", "elbow", "wrist", "stretch", "scale_on", "scale_off", "scale_edge",     # IK
            "exit_inside", "exit_outside", "tip")
FAM = {n: i for i, n in enumerate(FAMILIES)}
# The f32 engine's sincos_all keeps E_sc = 4 u up to |q| = 1e5 (kin_ref docstring).  Beyond, k = rintf(q * (2 / pi)f) is itself off: the
# product errs by 2 u |k| = 0.76 at 1e7, so the reduced argument leaves the polynomials' interval ("accuracy degrades gradually",
# armenv_kin.h), and at 1e9 k is past 2^24.  No bound is derived there, and the f32 engine is not compared on these two families.
F32_UNSPECIFIED = ("large_1e7", "large_1e9")
INIT_Q = [0.006418, 0.413184, -0.011401, -1.589317, 0.005379, 1.137684, -0.006539]
IDENTITY_QUAT = [0.0, 0.0, 0.0, 1.0]


def quat_case(W):
    """getRotation's case of float64 frames W [n,9] (column-major): 0 w, 1 z, 2 y, 3 x."""
    m00, m11, m22 = W[:, 0], W[:, 4], W[:, 8]
    cw = m00 + m11 + m22 > 0
    cz = ~cw & np.where(m00 < m11, m11 < m22, m00 < m22)
    cy = ~cw & ~cz & (m00 < m11)
    return np.where(cw, 0, np.where(cz, 1, np.where(cy, 2, 3)))


def _case_of(C, q):
    return int(quat_case(K.emu_fk_pose(C, np.asarray(q)[None], 64)[2])[0])


def _dw(C, q, tq):
    quat = K.emu_fk_pose(C, np.asarray(q)[None], 64)[1][0]
    return float(tq[3] * quat[3] + tq[0] * quat[0] + tq[1] * quat[1] + tq[2] * quat[2])


def settled_pose(C, tq, q0, tgt, trips=40, closest=False):
    """The pose the env's own steps settle in: IK updates from q0 towards tgt, in the emulation.  closest: of the last 30 trips' poses,
    the one whose orientation is closest to the target's (1 - w^2 hovers around the 10 eps rule once the pose has settled; this picks
    a pose below it)."""
    cfg = K.make_cfg(tq=tq)
    q = np.array(q0, dtype=np.float64)[None]
    tgt = np.asarray(tgt, dtype=np.float64)[None]
    best = None
    for k in range(trips):
        q, _, _ = K.emu_ik(C, q, tgt, cfg)
        if closest and k >= trips - 30:
            s2 = float(K.ik_ref(C, q[0], tgt[0], cfg)["s2"])
            if best is None or s2 < best[0]:
                best = (s2, q[0].copy())
    return best[1] if closest else q[0]


def _boundary_poses(C, rng, n_pairs):
    """Pairs of poses on either side of a getRotation case boundary, less than 1e-9 apart: bisection on the case along the segment
    between two drawn poses of different cases."""
    out, kinds = [], set()
    while len(out) < 2 * n_pairs:
        a, b = rng.uniform(-C["limit"], C["limit"], (2, 7))
        ca, cb = _case_of(C, a), _case_of(C, b)
        if ca == cb:
            continue
        lo, hi = 0.0, 1.0
        while (hi - lo) * np.abs(b - a).max() > 2e-10:
            mid = 0.5 * (lo + hi)
            if _case_of(C, a + mid * (b - a)) == ca:
                lo = mid
            else:
                hi = mid
        qa, qb = a + lo * (b - a), a + hi * (b - a)
        out += [qa, qb]
        kinds.add((_case_of(C, qa), _case_of(C, qb)))
    return np.array(out), kinds


def _quadrant_poses(rng, n):
    m = rng.integers(-1, 2, (n, 7)).astype(np.float64)
    side = np.where(rng.integers(0, 2, (n, 7)) == 1, np.inf, -np.inf)
    return np.nextafter(m * (math.pi / 2.0), side)


def fk_block(path, rng):
    C = K.chain_consts(path, 64)
    lim = C["limit"]
    tq = K.default_target_quat() if C["robot"] == "kuka" else IDENTITY_QUAT
    q_s = settled_pose(C, tq, INIT_Q, _reachable_target(C))
    parts = [("random", rng.uniform(-lim, lim, (48, 7)))]
    bq, kinds = _boundary_poses(C, rng, 12)
    assert len({c for k in kinds for c in k}) == 4, kinds          # every case has a boundary pose
    parts.append(("quat_boundary", bq))
    parts.append(("settled_frame", q_s[None] + np.concatenate([np.zeros((1, 7)), rng.normal(0, 1e-9, (4, 7))])))
    parts.append(("limits", np.where(rng.integers(0, 2, (8, 7)) == 1, lim, -lim)))
    parts.append(("quadrant", _quadrant_poses(rng, 16)))
    parts.append(("zero", np.zeros((1, 7))))
    big = np.where(rng.integers(0, 2, (6, 7)) == 1, 1.0, -1.0) * np.where(rng.integers(0, 2, (6, 7)) == 1, 1.0, rng.uniform(0.5, 1.0, (6, 7)))
    parts.append(("large_1e5", 1e5 * big * (1 - 1e-12)))                           # |q| < 1e5: the per-joint sincos keeps its fast path
    parts.append(("large_1e7", 1e7 * big))
    parts.append(("large_1e9", 1e9 * big))       # k = rint(2 q / pi) ~ 6e8: where the THIRD piece of pi / 2 (2e-21 k) first exceeds the bound
    q = np.concatenate([p for _, p in parts])
    fam = np.concatenate([np.full(len(p), FAM[n]) for n, p in parts])
    return C, q, fam


def _reachable_target(C):
    return np.array([0.45, 0.1, 0.3])


def fk_reference(path, q, fam, prec):
    C = K.chain_consts(path, prec)
    n = q.shape[0]
    out = {k: np.zeros((n, d)) for k, d in (("pos_hi", 3), ("pos_lo", 3), ("quat_hi", 4), ("quat_lo", 4))}
    out.update(E_p=np.zeros(n), E_q=np.zeros(n), case=np.zeros(n, dtype=np.int32), case_margin=np.zeros(n),
               use=np.ones(n, dtype=np.uint8))
    for i in range(n):
        qi = K._rnd(q[i], prec)
        W, p, _, pjs = K.fk_ref(C, qi)
        qr, case, mg = K.quat_ref(W)
        b = K.fk_bound(C, qi, prec, W, p, pjs)
        for k in range(3):
            out["pos_hi"][i, k], out["pos_lo"][i, k] = K.hi_lo(p[k])
        for k in range(4):
            out["quat_hi"][i, k], out["quat_lo"][i, k] = K.hi_lo(qr[k])
        out["E_p"][i], out["E_q"][i], out["case"][i], out["case_margin"][i] = b["E_p"], b["E_q"], case, float(mg)
        if prec == 32 and FAMILIES[fam[i]] in F32_UNSPECIFIED:
            out["use"][i] = 0
    return out


# ------------------------------------------------------------------------------------------------------------ IK

def _logspace(a, b, n):
    """n values from a to b, log-uniform (libm pow on Python floats: numpy's vectorised pow differs between CPUs)."""
    return [a * (b / a) ** (i / (n - 1)) for i in range(n)]


def _unit(rng):
    u = rng.normal(size=3)
    return u / math.sqrt(float(u[0]) ** 2 + float(u[1]) ** 2 + float(u[2]) ** 2)      # (no BLAS: the same bits on any CPU)


def _pos(C, q):
    return K.emu_fk_pose(C, np.asarray(q)[None], 64)[0][0]


class _Group:
    def __init__(self, name, path, precs, **cfg):
        self.name, self.path, self.precs, self.cfg_kw = name, path, precs, cfg
        self.C = {p: K.chain_consts(path, p) for p in precs}
        self.cfg = {p: K.make_cfg(prec=p, **cfg) for p in precs}
        self.q, self.tgt, self.fam, self.rows = [], [], [], {p: [] for p in precs}

    def evaluate(self, q, tgt):
        res, ok = {}, True
        for p in self.precs:
            ref = K.ik_ref(self.C[p], q, tgt, self.cfg[p])
            b = K.ik_bound(self.C[p], ref, self.cfg[p])
            if ref["count"] == 1 and not float(ref["wrap_dist"]) > 4 * b["wrap_err"]:
                ok = False
            if self.cfg[p]["exit_mode"] == 1 and not float(ref["exit_dist"]) > 4 * b["E_diff"]:
                ok = False
            res[p] = (ref, b)
        return ok, res

    def add(self, family, q, tgt, res):
        self.q.append(np.array(q, dtype=np.float64)); self.tgt.append(np.array(tgt, dtype=np.float64)); self.fam.append(FAM[family])
        for p in self.precs:
            self.rows[p].append(res[p])

    def draw(self, family, gen, count, want=None):
        """`count` cases from the generator, redrawing those too close to a discontinuity (or without the property `want`)."""
        k = 0
        for _ in range(50 * count):
            if k == count:
                return
            q, tgt = gen()
            ok, res = self.evaluate(q, tgt)
            if ok and (want is None or want(res)):
                self.add(family, q, tgt, res)
                k += 1
        raise AssertionError(f"{self.name}/{family}: the stream does not yield {count} admissible cases")

    def must(self, family, q, tgt, want=None):
        ok, res = self.evaluate(q, tgt)
        assert ok, f"{self.name}/{family}: a constructed case sits on a discontinuity"
        assert want is None or want(res), f"{self.name}/{family}: a constructed case lacks its property"
        self.add(family, q, tgt, res)


def _solve_scalar(f, lo, hi, iters=200):
    """x in [lo, hi] with f changing sign between its float neighbours (f(lo) < 0 <= f(hi))."""
    assert f(lo) < 0 <= f(hi)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if f(mid) < 0:
            lo = mid
        else:
            hi = mid
    return lo, hi


def _near(rng, C, lim):
    def gen():
        q = rng.uniform(-lim, lim)
        return q, _pos(C, q) + rng.uniform(0.01, 0.05) * _unit(rng)
    return gen


def _singular(rng, C, lim, joints, k):
    def gen():
        q = rng.uniform(-0.8 * lim, 0.8 * lim)
        for j in joints:
            q[j] = 10.0 ** -k * rng.uniform(1.0, 3.0) * (1 if rng.integers(0, 2) else -1)
        return q, _pos(C, q) + rng.uniform(0.01, 0.03) * _unit(rng)
    return gen


def default_group(name, rng, precs=(64, 32), light=False, **cfg):
    """The KUKA built-in chain with the workload's target orientation: every family (light: the orientation and scale-back families
    only, and fewer drawn poses)."""
    g = _Group(name, "kuka_builtin", precs, **cfg)
    C = g.C[64]
    lim = C["limit"]
    tq = np.array(g.cfg[64]["tq"])
    mxd = g.cfg[64]["max_dtheta"]
    g.draw("random", _near(rng, C, lim), 24 if light else 48)
    # |w| of the error quaternion at 0.5: the last joint turns the frame about its own z, which sweeps w through a sinusoid
    for _ in range(2):
        while True:
            q = rng.uniform(-lim, lim)
            ws = [abs(_dw(C, np.r_[q[:6], a], tq)) - 0.5 for a in (-1.5, 1.5)]
            if ws[0] * ws[1] < 0:
                break
        sgn = 1.0 if ws[0] < 0 else -1.0
        lo, hi = _solve_scalar(lambda a: sgn * (abs(_dw(C, np.r_[q[:6], a], tq)) - 0.5), -1.5, 1.5)
        for a in (lo, hi, lo - 1e-3, hi + 1e-3):
            qa = np.r_[q[:6], a]
            near = a in (lo, hi)
            g.must("w_half", qa, _pos(C, qa) + 0.02 * _unit(rng),
                   lambda res, near=near: (abs(abs(float(res[64][0]["dw"])) - 0.5) < 1e-15) == near)
    # |w| -> 1: the settled pose, the last joint turned by delta: 1 - w^2 = sin^2(delta / 2), down to below the 10 eps rule
    q_s = settled_pose(C, tq, INIT_Q, [0.45, 0.1, 0.3], trips=50, closest=True)
    g.must("settled", q_s, _pos(C, q_s) + 0.02 * _unit(rng), lambda res: float(res[64][0]["s2"]) < 10 * K.EPS[64])
    for d in _logspace(2e-2, 1e-9, 12):
        qa = q_s + np.r_[np.zeros(6), d]
        g.must("w_to_one", qa, _pos(C, qa) + 0.02 * _unit(rng),
               lambda res, d=d: abs(float(res[64][0]["s2"]) - math.sin(d / 2) ** 2) < 1e-3 * math.sin(d / 2) ** 2 + 1e-15)
    # (stretch: elbow AND wrist straight; with the shoulder straight as well the flange points up, half a turn from the target
    # orientation, which is the wrap itself)
    for fam, joints in (("elbow", (3,)), ("wrist", (5,)), ("stretch", (3, 5))):
        for k in ([] if light else [2 + 6 * i / 11 for i in range(12)]):
            g.draw(fam, _singular(rng, C, lim, joints, k), 1)
    g.draw("limits", lambda: (lambda q: (q, _pos(C, q) + 0.02 * _unit(rng)))(np.where(rng.integers(0, 2, 7) == 1, lim, -lim)), 2 if light else 6)
    g.draw("quadrant", lambda: (lambda q: (q, _pos(C, q) + 0.02 * _unit(rng)))(_quadrant_poses(rng, 1)[0]), 2 if light else 8)
    # (all seven joints at 0 is the FK blocks' case: the flange then points up, the wrap again; here four drawn joints are 0)
    g.draw("zero", lambda: (lambda q: (q, _pos(C, q) + 0.02 * _unit(rng)))(rng.uniform(-lim, lim) * (rng.permutation(7) < 3)), 1 if light else 4)
    over = lambda res: all(float(r["mx"]) > 1.01 * float(r["max_dtheta"]) for r, _ in res.values())
    under = lambda res: all(float(r["mx"]) < 0.99 * float(r["max_dtheta"]) for r, _ in res.values())
    g.draw("scale_on", lambda: (lambda q: (q, _pos(C, q) + rng.uniform(0.3, 1.0) * _unit(rng)))(rng.uniform(-lim, lim)), 8, over)
    # (the orientation error alone moves a drawn pose by more than 45 degrees: start at the settled pose)
    g.draw("scale_off", lambda: (lambda q: (q, _pos(C, q) + rng.uniform(0.002, 0.01) * _unit(rng)))(q_s + rng.normal(0, 0.02, 7)), 8, under)
    # max |dtheta| just under and just over max_dtheta: the target slides along a ray until the emulation's update crosses it
    cfg64 = g.cfg[64]
    for _ in range(2):
        q = q_s + rng.normal(0, 0.02, 7)
        u, p0 = _unit(rng), _pos(C, q)

        def excess(t):
            qo, _, _ = K.emu_ik(C, q[None], (p0 + t * u)[None], dict(cfg64, max_dtheta=10.0))
            return float(np.abs(qo[0] - q).max()) - mxd
        lo, hi = _solve_scalar(excess, 1e-3, 2.0, iters=40)
        for t, side in ((lo * (1 - 1e-9), -1), (hi * (1 + 1e-9), 1)):
            g.must("scale_edge", q, p0 + t * u,
                   lambda res, side=side: 0 < side * (float(res[64][0]["mx"]) / float(res[64][0]["max_dtheta"]) - 1) < 1e-6)
    return g


def exit_group(rng):
    g = _Group("exit1", "kuka_builtin", (64, 32), exit_mode=1)
    C = g.C[64]
    lim = C["limit"]
    res = g.cfg[64]["residual"]
    for fam, scale, cnt in (("exit_inside", (0.1, 0.7), 0), ("exit_outside", (1.5, 300.0), 1)):
        g.draw(fam, lambda: (lambda q: (q, _pos(C, q) + res * rng.uniform(*scale) * _unit(rng)))(rng.uniform(-lim, lim)), 8,
               lambda r, cnt=cnt: all(ref["count"] == cnt for ref, _ in r.values()))
    return g


def step_group(rng, name="step", **cfg):
    """The env step's form of the update (make_cfg dv): actions instead of targets, for the step and rollout kernels, whose carried
    (cos, sin) pair is the only place where the trip's choice between rotate_small (max_dtheta <= 0.7854) and sincos_all shows."""
    g = _Group(name, "kuka_builtin", (64, 32), dv=STEP_DV, **cfg)
    C = g.C[64]
    lim = C["limit"]
    act = lambda lo, hi: (rng.uniform(lo, hi) / STEP_DV * _unit(rng)).astype(np.float32).astype(np.float64)
    g.draw("random", lambda: (rng.uniform(-lim, lim), act(0.01, 0.05)), 32)
    q_s = settled_pose(C, g.cfg[64]["tq"], INIT_Q, [0.45, 0.1, 0.3], trips=50, closest=True)
    g.must("settled", q_s, act(0.005, 0.02))
    for d in _logspace(2e-2, 1e-9, 8):
        g.must("w_to_one", q_s + np.r_[np.zeros(6), d], act(0.005, 0.02))
    for k in (2, 4, 6, 8):
        g.draw("elbow", lambda: (_singular(rng, C, lim, (3,), k)()[0], act(0.01, 0.03)), 1)
    over = lambda res: all(float(r["mx"]) > 1.01 * float(r["max_dtheta"]) for r, _ in res.values())
    under = lambda res: all(float(r["mx"]) < 0.99 * float(r["max_dtheta"]) for r, _ in res.values())
    g.draw("scale_on", lambda: (rng.uniform(-lim, lim), act(0.3, 1.0)), 6, over)
    g.draw("scale_off", lambda: (q_s + rng.normal(0, 0.02, 7), act(0.002, 0.01)), 6, under)
    return g


def chain_group(name, path, rng, precs, tq=None, tip=(0.0, 0.0, 0.0), family="random"):
    g = _Group(name, path, precs, tq=tq, tip=tip)
    C = g.C[64]
    g.draw(family, _near(rng, C, C["limit"]), 24)
    for fam, joints in (("elbow", (3,)), ("wrist", (5,))):
        for k in (3, 6):
            g.draw(fam, _singular(rng, C, C["limit"], joints, k), 1)
    return g


def ik_groups():
    rng = lambda k: np.random.default_rng([SEED, k])
    return [default_group("default", rng(1)),
            default_group("angle_f64", rng(2), precs=(64,), light=True, angle_f32=0),
            default_group("big_step", rng(3), precs=(64,), light=True, max_dtheta=1.0),
            exit_group(rng(4)),
            step_group(rng(9)),
            step_group(rng(10), "step_big", max_dtheta=1.0),
            chain_group("tip", "kuka_builtin", rng(5), (64,), tip=(0.01, -0.02, 0.05), family="tip"),
            chain_group("kuka_generic", "kuka_generic", rng(6), (64, 32)),
            chain_group("diana_builtin", "diana_builtin", rng(7), (64, 32), tq=IDENTITY_QUAT),
            chain_group("diana_generic_base", "diana_generic_base", rng(8), (64,), tq=IDENTITY_QUAT)]


COND = ("sigma_max", "sigma_min", "kappa", "G", "G_lin", "G_ang", "one_minus_w2", "dtheta_max", "min_pivot", "dw", "wrapped")
TERMS = ("jacobian", "linear", "angular", "solve", "jty", "E_ang")


def _ik_arrays(g):
    out = {f"ik.{g.name}.q": np.array(g.q), f"ik.{g.name}.tgt": np.array(g.tgt), f"ik.{g.name}.family": np.array(g.fam, dtype=np.int32),
           f"ik.{g.name}.path": np.array(g.path)}
    c = g.cfg[g.precs[0]]
    out[f"ik.{g.name}.cfg"] = np.array([c["lam"], c["max_dtheta"], c["residual"], c["exit_mode"], c["angle_f32"]] + c["tip"] + c["tq"] + [c["dv"]])
    out[f"ik.{g.name}.precs"] = np.array(g.precs, dtype=np.int32)
    n = len(g.q)
    for p in g.precs:
        a = dict(q_out_hi=np.zeros((n, 7)), q_out_lo=np.zeros((n, 7)), trig_hi=np.zeros((n, 14)), trig_lo=np.zeros((n, 14)),
                 count=np.zeros(n, dtype=np.int32), E_q_out=np.zeros((n, 7)), E_trig=np.zeros(n), cond=np.zeros((n, len(COND))),
                 dist=np.zeros((n, 5)), terms=np.zeros((n, len(TERMS))))
        for i, (ref, b) in enumerate(g.rows[p]):
            for j in range(7):
                a["q_out_hi"][i, j], a["q_out_lo"][i, j] = K.hi_lo(ref["q_out"][j])
                a["trig_hi"][i, j], a["trig_lo"][i, j] = K.hi_lo(K.mp.cos(ref["q_out"][j]))
                a["trig_hi"][i, 7 + j], a["trig_lo"][i, 7 + j] = K.hi_lo(K.mp.sin(ref["q_out"][j]))
            a["count"][i], a["E_q_out"][i], a["E_trig"][i] = ref["count"], b["E_q_out"], b["E_trig"]
            if ref["count"]:
                a["cond"][i] = [b["cond"][k] for k in COND]
                a["terms"][i] = [b["terms"][k] for k in TERMS[:5]] + [b["E_ang"]]
                a["dist"][i] = [float(ref["wrap_dist"]), b["wrap_err"], float(ref["exit_dist"]), b["E_diff"], float(ref["case_margin"])]
            else:
                a["dist"][i] = [np.inf, 0.0, float(ref["exit_dist"]), b["E_diff"], np.inf]
        small = ("q_out_lo", "trig_lo", "dist", "terms")          # the lo halves and the diagnostics: float32 is ample
        out.update({f"ik.{g.name}.{p}.{k}": v.astype(np.float32) if k in small else v for k, v in a.items()})
    return out


def build():
    out = {"families": np.array(FAMILIES)}
    for k, path in enumerate(K.CHAIN_PATHS):
        C, q, fam = fk_block(path, np.random.default_rng([SEED, 100 + k]))
        out[f"fk.{path}.q"], out[f"fk.{path}.family"] = q, fam.astype(np.int32)
        for prec in (64, 32):
            out.update({f"fk.{path}.{prec}.{k2}": v.astype(np.float32) if k2.endswith("_lo") else v
                        for k2, v in fk_reference(path, q, fam, prec).items()})
    groups = ik_groups()
    out["ik_groups"] = np.array([g.name for g in groups])
    for g in groups:
        out.update(_ik_arrays(g))
    check(out)
    return out


def ik_group_cfg(T, name, prec):
    c = T[f"ik.{name}.cfg"]
    return K.make_cfg(prec=prec, lam=c[0], max_dtheta=c[1], residual=c[2], exit_mode=int(c[3]), angle_f32=int(c[4]), tip=c[5:8], tq=c[8:12], dv=c[12])


def check(T):
    """The families' conditions and the distances from the discontinuities, on a built or loaded table."""
    fams = [str(s) for s in T["families"]]
    fam_of = lambda a: [fams[i] for i in a]
    seen = set()
    for path in K.CHAIN_PATHS:
        f = fam_of(T[f"fk.{path}.family"])
        seen |= set(f)
        case = T[f"fk.{path}.64.case"]
        assert set(case.tolist()) == {0, 1, 2, 3}, path
        b = np.array([x == "quat_boundary" for x in f])
        assert b.sum() >= 8 and (T[f"fk.{path}.64.case_margin"][b] < 1e-9).all(), path
        assert set(case[b].tolist()) == {0, 1, 2, 3}, path
        q = T[f"fk.{path}.q"]
        s = np.array([x == "settled_frame" for x in f])
        # the settled frame of the workload: two diagonal elements equal (KUKA: m00 = m11 ~ 0, trace ~ -1)
        d = K.emu_fk_pose(K.chain_consts(path), q[s], 64)[2][:, [0, 4, 8]]
        gap = np.min(np.abs(np.stack([d[:, 0] - d[:, 1], d[:, 1] - d[:, 2], d[:, 0] - d[:, 2]])), axis=0)
        assert s.sum() >= 1 and (gap < 1e-6).all(), (path, gap)           # (Diana settles on the identity: all three equal)
        for name, lo, hi in (("large_1e5", 4e4, 1e5), ("large_1e7", 4e6, 1.0001e7), ("large_1e9", 4e8, 1.0001e9)):
            m = np.array([x == name for x in f])
            assert m.sum() >= 1 and (np.abs(q[m]) > lo).all() and (np.abs(q[m]) < hi).all(), (path, name)
        m = np.array([x == "zero" for x in f])
        assert m.sum() == 1 and (q[m] == 0).all(), path
        m = np.array([x == "limits" for x in f])
        assert m.sum() >= 4 and (np.abs(q[m]) == K.chain_consts(path)["limit"]).all(), path
        m = np.array([x == "quadrant" for x in f])
        k = np.rint(q[m] / (math.pi / 2))
        assert m.sum() >= 8 and (np.abs(q[m] - k * (math.pi / 2)) <= 4.5e-16).all() and (q[m] != k * (math.pi / 2)).all(), path
        assert (T[f"fk.{path}.32.use"][[x in F32_UNSPECIFIED for x in f]] == 0).all()
    for name in [str(s) for s in T["ik_groups"]]:
        f = fam_of(T[f"ik.{name}.family"])
        seen |= set(f)
        for prec in T[f"ik.{name}.precs"].tolist():
            d, cnt, cond = T[f"ik.{name}.{prec}.dist"], T[f"ik.{name}.{prec}.count"], T[f"ik.{name}.{prec}.cond"]
            cfg = ik_group_cfg(T, name, prec)
            assert (d[:, 0] > 4 * d[:, 1]).all(), (name, prec, "wrap")
            if cfg["exit_mode"] == 1:
                assert (d[:, 2] > 4 * d[:, 3]).all(), (name, prec, "exit")
                assert set(cnt.tolist()) == {0, 1}
                assert all((c == 0) == (x == "exit_inside") for c, x in zip(cnt, f))
            else:
                assert (cnt == 1).all()
            sel = lambda n: np.array([x == n for x in f])
            if name in ("default", "angle_f64", "big_step"):
                s2, mx = cond[:, 6], cond[:, 7]
                w_abs = np.sqrt(np.maximum(0.0, 1 - s2))
                r = sel("random")
                assert (w_abs[r] < 0.5).sum() >= 4 and (w_abs[r] > 0.5).sum() >= 4, name                   # inner and outer form
                if prec == 64:
                    assert (cond[r, 9] < 0).sum() >= 4 and (cond[r, 10] > 0).sum() >= 4, name                # w < 0, the wrap taken
                assert sel("w_half").sum() == 8 and (np.abs(w_abs[sel("w_half")] - 0.5) < 2e-3).all()
                if prec == 64:
                    assert (s2[sel("w_to_one")] < 10 * K.EPS[64]).sum() >= 2 and (s2[sel("w_to_one")] > 1e-5).sum() >= 1       # down to the rule
                    assert (s2[sel("settled")] < 1e-12).all()
                # (a straight wrist alone costs this 7-joint arm no rank: its family is pinned by q[5], the others by the pivot too)
                qg = T[f"ik.{name}.q"]
                for fam, j in () if name != "default" else (("elbow", 3), ("wrist", 5), ("stretch", 3)):
                    piv, aq = cond[sel(fam), 8], np.abs(qg[sel(fam), j])
                    assert len(piv) == 12 and aq.min() < 3e-8 and aq.max() > 1e-3 and (aq < 0.04).all(), (name, fam)
                    assert fam == "wrist" or (piv.min() < 1e-4 and cond[sel(fam), 1].min() < 1e-5), (name, fam, piv.min())
                assert (mx[sel("scale_on")] > cfg["max_dtheta"]).all() and (mx[sel("scale_off")] < cfg["max_dtheta"]).all()
                e = mx[sel("scale_edge")] / float(K._rnd(cfg["max_dtheta"], prec)) - 1
                if prec == 64:
                    assert len(e) == 4 and (np.abs(e) < 1e-6).all() and (e > 0).sum() == 2, (name, e)
    assert seen == set(fams), set(fams) - seen
    return True
