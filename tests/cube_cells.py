"""Cell table of the two cube tasks (push, pick): single env steps whose input state sits a known margin to one side of ONE decision of
the contact / gripper / outcome code and well inside every other one.  tests/test_cube_cells.py checks the table on the CPU (every cell
lands in its branch, no cell is ambiguous under the arm's allowed disagreement, every edge is visible, every constant is pinned);
tests/test_gpu_cube_cells.py runs it through the HIP kernels.

Placement is two-pass.  The arm's motion does not depend on the cube, so a probe step of the oracle with the cube parked far away gives
the flange position before and after the IK (p0, p1) and the tool axis; the cube, target, velocity, d_last, gripper state and hold
offset of a cell are then written relative to p1 (pick: to the tip p1 + L axis).

Margins: m = 1e-5 m for the f64 engine (ten times the stated f64 per-step agreement of 1e-6), m = 1e-3 for the f32 engine (ten times its
1e-4); decisions that do not depend on the arm (fall count, outcome block with the cube at rest and away from the tool, Coulomb stop)
sit a few ulp (the stop: a relative 1e-12, fast_rsqrt being good to a few ulp) from their edge and are f64-only, as are the 1e-5
deadband, the 1 mm travel gate and the 6 mm trigger distance, which leave no room for 10 m = 1e-2.

`model_step` is a float64 restatement of the model as include/armenv.h and the gripper paragraph of DESIGN.md describe it, written
without reference to the kernel; it also returns the `trace` of the decisions it took, which is what "lands in its branch" means.

Two decisions have no edge of their own and their cells say so:
  * vertical overlap (`lo < cube_z + h`): with no vertical overlap pen_v <= 0 < pen, so the press-down test already leaves the cube alone.
    The pair `voverlap` sits either side of it with pen_v = 3 m / -m and pen = m; what it shows is the pen_v < pen edge next to it.
  * model 0, `s > 0` inside the footprint: with the default radius (r + h = 0.05 > the footprint's half diagonal 0.0283) s is always
    positive; the pair lives in the variant `m0r5` (push_eef_radius = 0.005).
"""
import math

import numpy as np

M64, M32 = 1e-5, 1e-3
PERTURB = {64: 1e-6, 32: 1e-4}      # the engine's allowed per-step disagreement with the oracle
PUSH_AUX, PICK_AUX = 10, 12

# include/armenv.h defaults, restated for the model
CONST = dict(push_success_dis=0.05, push_cube_half=0.02, push_eef_radius=0.03, push_rest_z=0.01 - 0.01474, push_place_z=0.01,
             pick_gripper_length=0.257, pick_trigger_dis=0.006, pick_jaw_half=0.02, push_tool_radius=0.045, push_tool_below=0.045,
             push_contact_erp=0.01, push_contact_split=0.04, push_friction=0.03, push_gravity=10.0, push_dt=1.0 / 240.0,
             push_drop_contact=0.015, push_drop_relax=0.1, push_contact_model=1, max_steps=500)
FALL_C = 0.5 * 10.0 / 240.0 ** 2         # g dt^2 / 2; the default cube lands in call 13 (156 c < 0.015 <= 182 c)
REST, H = CONST["push_rest_z"], CONST["push_cube_half"]

VARIANTS = {
    "push": {
        "default": {},
        "nofric": dict(push_friction=0.0),
        "bigsplit": dict(push_contact_split=0.1),
        "m0": dict(push_contact_model=0),
        "m0r5": dict(push_contact_model=0, push_eef_radius=0.005),
        # push_drop_contact a margin either side of the drop after 12 calls: the cube lands in call 13 / call 12
        "drop_hi": dict(push_drop_contact=156 * FALL_C + M64),
        "drop_lo": dict(push_drop_contact=156 * FALL_C - M64),
    },
    "pick": {
        "default": {},
        "m0": dict(push_contact_model=0),
        "r5": dict(push_eef_radius=0.005),      # a tip small enough for the sweep's `s > 0` to have two sides
    },
}

# arm name -> (flange target of the start pose [pick: of the tip], action)
ARMS = {
    "push": {
        "low": ((0.45, 0.05, 0.005), (0.0, 0.0, 0.0)),
        "mid": ((0.50, -0.08, 0.03), (0.0, 0.0, 0.0)),
        "high": ((0.42, 0.10, 0.08), (0.0, 0.0, 0.0)),
        "mid_xy": ((0.48, 0.02, 0.03), (0.25, 0.25, 0.0)),
        "low_y": ((0.53, -0.03, 0.005), (0.0, 0.25, 0.0)),
        "mid_dn": ((0.46, -0.04, 0.05), (0.0, 0.0, -0.25)),
    },
    "pick": {
        "above": ((0.50, 0.00, 0.03), (0.0, 0.0, 0.0)),
        "side": ((0.45, 0.05, 0.005), (0.0, 0.0, 0.0)),
        "hi": ((0.52, -0.05, 0.06), (0.0, 0.0, 0.0)),
        "above_xy": ((0.47, 0.03, 0.03), (0.25, 0.25, 0.0)),
        "above_dn": ((0.49, -0.03, 0.05), (0.0, 0.0, -0.25)),
    },
}
FAR = {"push": (0.25, -0.27), "pick": (0.25, -0.27)}      # where a cube is out of every tool's way


class Cell:
    __slots__ = ("name", "task", "variant", "arm", "q", "action", "step", "aux", "branch", "side", "want", "expect", "f32", "twostep")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def __repr__(self):
        return "<%s %s/%s %s>" % (self.task, self.variant, self.name, self.arm)


def make_cfg(O, task, variant, **shift):
    """the oracle's config of a variant; shift: constant -> value added (max_steps) / relative change (friction, erp: given as ('rel', x))"""
    cfg = O.default_config(task)
    for k, v in VARIANTS[task][variant].items():
        setattr(cfg, k, v)
    for k, v in shift.items():
        cur = getattr(cfg, k)
        setattr(cfg, k, cur * (1.0 + v[1]) if isinstance(v, tuple) else cur + v)
    return cfg


def constants(task, variant):
    c = dict(CONST)
    c.update(VARIANTS[task][variant])
    return c


# ------------------------------------------------------------------ the arm: poses and probe

_ARM_CACHE = {}


def arms(O, chain):
    """name -> dict(q, action, p0, p1, axis, q1, iters, minpiv) per task, by a probe step of the oracle with the cube parked far away"""
    if "arms" in _ARM_CACHE:
        return _ARM_CACHE["arms"]
    out = {}
    for task, table in ARMS.items():
        cfg = O.default_config(task)
        L = cfg.pick_gripper_length
        names = list(table)
        extra = []
        if task == "push":      # the 1 mm travel gate of model 0: a scan of small planar actions, see _travel_arms
            extra = [("scan%03d" % i, ((0.50, 0.04, 0.03), (s, 0.0, 0.0))) for i, s in enumerate(np.linspace(0.008, 0.018, 201))]
        rows = [(nm, table[nm]) for nm in names] + extra
        qs, acts = [], []
        for nm, (tgt, act) in rows:
            key = (task, tgt)
            if key not in _ARM_CACHE:
                q = np.array(O.INIT_Q, dtype=np.float64)
                t = np.array(tgt, dtype=np.float64) + (np.array([0.0, 0.0, L]) if task == "pick" else 0.0)
                for _ in range(16):
                    res, _ = O.ik(chain, cfg, q, t)
                    if task == "pick":
                        q[:6] = res[0, :6]
                    else:
                        q = res[0].copy()
                _ARM_CACHE[key] = q
            qs.append(_ARM_CACHE[key]); acts.append(act)
        n = len(rows)
        st = (O.PushState if task == "push" else O.PickState)(n)
        st.q[:] = np.array(qs); st.step[:] = 20
        st.aux[:, 0:2] = FAR[task]; st.aux[:, 2] = REST
        st.aux[:, 3:6] = (0.6, 0.25, 0.01); st.aux[:, 6] = 0.6
        if task == "pick":
            st.aux[:, 7] = 1.0
        a = np.array(acts, dtype=np.float32)
        minpiv = np.zeros(n)
        p0, _ = O.fk(chain, st.q)
        step = O.push_step if task == "push" else O.pick_step
        _, _, _, _, iters = step(chain, cfg, st, a, minpiv=minpiv)
        d = {}
        for i, (nm, (tgt, act)) in enumerate(rows):
            p1, R, _, _ = O.fk_full(chain, st.q[i])
            d[nm] = dict(q=np.array(qs[i]), action=np.array(act, dtype=np.float32), p0=p0[i].copy(), p1=p1.copy(), axis=R[:, 2].copy(),
                         q1=st.q[i].copy(), iters=int(iters[i]), minpiv=float(minpiv[i]),
                         pose_pivot=float(O.pose_min_pivot(chain, cfg, np.array(qs[i]))[0]))
        out[task] = d
    _travel_arms(out["push"])
    _ARM_CACHE["arms"] = out
    return out


def _travel_arms(d):
    """model 0's travel gate compares the arm's own horizontal travel with 1 mm, so the margin cannot be placed: it is FOUND, among
    the scanned actions, as the travel nearest to the gate that still keeps m = 1e-5 from it (and at most 10 m)"""
    best = {"under": None, "over": None}
    for nm in [k for k in d if k.startswith("scan")]:
        a = d.pop(nm)
        t = float(np.hypot(*(a["p1"][:2] - a["p0"][:2]))) - 1e-3
        side = "under" if t < 0 else "over"
        if M64 <= abs(t) <= 10 * M64 and (best[side] is None or abs(t) < best[side][0]):
            best[side] = (abs(t), a)
    for side, b in best.items():
        assert b is not None, "no scanned action leaves the 1 mm travel gate a margin in [m, 10 m] on side %s" % side
        d["travel_" + side] = b[1]


# ------------------------------------------------------------------ the model (float64, from include/armenv.h)

def land_step(c):
    k = 1
    while 0.5 * c["push_gravity"] * c["push_dt"] ** 2 * k * (k + 1) < c["push_drop_contact"]:
        k += 1
    return k


def fall_z(c, k, z):
    """cube height after stepSimulation call k since the spawn"""
    if k <= land_step(c):
        return c["push_place_z"] - 0.5 * c["push_gravity"] * c["push_dt"] ** 2 * k * (k + 1)
    return c["push_rest_z"] + (z - c["push_rest_z"]) * (1.0 - c["push_drop_relax"])


def _nearest(p, cube, h):
    qx = min(max(p[0], cube[0] - h), cube[0] + h)
    qy = min(max(p[1], cube[1] - h), cube[1] + h)
    return qx, qy


def _sphere_push(c, p0, p, cube, tr, r):
    """model 0: tool sphere against the box, the whole penetration removed"""
    h = c["push_cube_half"]
    tr["band"] = abs(p[2] - cube[2]) < h + r
    if not tr["band"]:
        return
    qx, qy = _nearest(p, cube, h)
    gx, gy = p[0] - qx, p[1] - qy
    gap = math.hypot(gx, gy)
    tr["gap<r"] = gap < r
    if not tr["gap<r"]:
        return
    tr["outside"] = gap > 1e-9
    if tr["outside"]:
        cube[0] -= (r - gap) * gx / gap
        cube[1] -= (r - gap) * gy / gap
        return
    mx, my = p[0] - p0[0], p[1] - p0[1]
    mn = math.hypot(mx, my)
    tr["travel>=1mm"] = mn >= 1e-3
    if not tr["travel>=1mm"]:
        return
    mx, my = mx / mn, my / mn
    s = (r + h) - ((cube[0] - p[0]) * mx + (cube[1] - p[1]) * my)
    tr["s>0"] = s > 0.0
    if s > 0.0:
        cube[0] += s * mx
        cube[1] += s * my


def _cylinder_contact(c, p, cube, vel, k, tr):
    """model 1: velocity-level contact against the vertical tool cylinder, Coulomb friction once landed, integration"""
    h, r, dt = c["push_cube_half"], c["push_tool_radius"], c["push_dt"]
    lo = p[2] - c["push_tool_below"]
    pen_v = cube[2] + h - lo
    tr["v_overlap"] = pen_v > 0.0
    qx, qy = _nearest(p, cube, h)
    gx, gy = qx - p[0], qy - p[1]
    gap = math.hypot(gx, gy)
    tr["h_overlap"] = gap < r
    if tr["v_overlap"] and tr["h_overlap"]:
        tr["outside"] = gap > 1e-9
        if tr["outside"]:
            pen, nx, ny = r - gap, gx / gap, gy / gap
        else:
            exits = [(cube[0] + h - p[0], -1.0, 0.0), (p[0] - (cube[0] - h), 1.0, 0.0),
                     (cube[1] + h - p[1], 0.0, -1.0), (p[1] - (cube[1] - h), 0.0, 1.0)]
            b = min(range(4), key=lambda i: exits[i][0])
            tr["face"] = b
            pen, nx, ny = exits[b][0] + r, exits[b][1], exits[b][2]
        tr["press"] = pen_v < pen
        if not tr["press"]:
            tr["pen<split"] = pen < c["push_contact_split"]
            tgt = c["push_contact_erp"] * pen / dt if tr["pen<split"] else 0.0
            vn = vel[0] * nx + vel[1] * ny
            tr["vn<tgt"] = vn < tgt
            if vn < tgt:
                vel[0] += (tgt - vn) * nx
                vel[1] += (tgt - vn) * ny
    tr["landed"] = k >= land_step(c)
    sp = math.hypot(vel[0], vel[1])
    tr["moving"] = sp > 0.0
    if tr["landed"] and sp > 0.0:
        dec = c["push_friction"] * c["push_gravity"] * dt
        tr["stop"] = not sp > dec
        f = (sp - dec) / sp if sp > dec else 0.0
        vel[0] *= f
        vel[1] *= f
    cube[0] += vel[0] * dt
    cube[1] += vel[1] * dt


def f32_dist(cube, target):
    f = np.float32
    d = [f(cube[k]) - f(target[k]) for k in range(3)]
    return np.sqrt(f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])))


def model_step(task, c, arm, aux, step):
    """one env step of a cell: returns dict(aux, step, reward, done, success, trace, test)"""
    aux = [float(x) for x in aux]
    cube, target, tr = aux[0:3], aux[3:6], {}
    p0, p1 = arm["p0"], arm["p1"]
    if task == "push":
        vel = aux[7:9]
        if c["push_contact_model"] == 1:
            k = step + 2
            tr["free_fall"] = k <= land_step(c)
            cube[2] = fall_z(c, k, cube[2])
            _cylinder_contact(c, p1, cube, vel, k, tr)
        else:
            _sphere_push(c, p0, p1, cube, tr, c["push_eef_radius"])
        aux[7:9] = vel
    else:
        grip, off = aux[7], aux[8:11]
        L, h = c["pick_gripper_length"], c["push_cube_half"]
        tip = [p1[k] + L * arm["axis"][k] for k in range(3)]
        tip0 = [tip[k] - (p1[k] - p0[k]) for k in range(3)]
        if c["push_contact_model"] == 1 and grip != 2.0:
            if step > 0:
                cube[2] = fall_z(c, 2 * step + 1, cube[2])
            tr["free_fall"] = 2 * step + 2 <= land_step(c)
            cube[2] = fall_z(c, 2 * step + 2, cube[2])
        tr["grip_in"] = grip
        if grip == 2.0:
            z = tip[2] + off[2]
            tr["clamped"] = z < c["push_rest_z"]
            cube[:] = [tip[0] + off[0], tip[1] + off[1], max(z, c["push_rest_z"])]
        else:
            held = False
            if grip == 0.0:
                g2 = sum((tip[k] - min(max(tip[k], cube[k] - h), cube[k] + h)) ** 2 for k in range(3))
                tr["trigger"] = math.sqrt(g2) - c["push_eef_radius"] < c["pick_trigger_dis"]
                if tr["trigger"]:
                    hx, hy = cube[0] - tip[0], cube[1] - tip[1]
                    tr["tip_above"] = tip[2] >= cube[2]
                    tr["in_jaw"] = math.hypot(hx, hy) <= c["pick_jaw_half"]
                    held = tr["tip_above"] and tr["in_jaw"]
                    grip = 2.0 if held else 1.0
                    if held:
                        off = [hx, hy, cube[2] - tip[2]]
            if not held:
                _sphere_push(c, tip0, tip, cube, tr, c["push_eef_radius"])
        aux[7], aux[8:11] = grip, off
    step += 1
    d_cur = math.sqrt((cube[0] - target[0]) ** 2 + (cube[1] - target[1]) ** 2 + (cube[2] - target[2]) ** 2)
    test = d_cur - aux[6]
    tr["deadband"] = abs(test) < 1e-5
    shaped = 0.01 if tr["deadband"] else test
    dt32 = f32_dist(cube, target)
    tr["timeout"] = step > c["max_steps"]
    tr["near32"] = float(dt32) < c["push_success_dis"]
    if tr["timeout"]:
        reward, done = float(np.float32(-dt32) * np.float32(50.0)), True
    elif tr["near32"]:
        reward, done = 100.0, True
    else:
        reward, done = -shaped * 100.0, False
    tr["near64"] = d_cur < c["push_success_dis"]
    aux[0:3], aux[6] = cube, d_cur
    return dict(aux=np.array(aux), step=step, reward=reward, done=done, success=tr["near64"], trace=tr, test=test, dt32=float(dt32))


# ------------------------------------------------------------------ the cells

def _ulps(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def _deadband_edge(d_cur, sign, n_ulp):
    """d_last with fabs(d_cur - d_last) on either side of 1e-5, n_ulp representable values from the flip: (inside, outside)"""
    x = d_cur - sign * 1e-5
    inside = lambda v: abs(d_cur - v) < 1e-5
    toward = math.inf if sign > 0 else -math.inf      # moving d_last towards d_cur makes |test| smaller
    while not inside(x):
        x = math.nextafter(x, toward)
    while inside(math.nextafter(x, -toward)):
        x = math.nextafter(x, -toward)
    # x is the last value inside
    a = x
    for _ in range(n_ulp - 1):
        a = math.nextafter(a, toward)
    b = x
    for _ in range(n_ulp):
        b = math.nextafter(b, -toward)
    assert inside(a) and not inside(b)
    return a, b


def _success_split(rng, want32_near, want64_near):
    """cube x / target x (same y, z) whose f32 distance and f64 distance fall on the wanted sides of 0.05"""
    for _ in range(200000):
        tx = 0.45 + 0.1 * rng.random()
        cx = tx + 0.05 + rng.uniform(-4e-8, 4e-8)
        d64 = math.sqrt((cx - tx) ** 2)
        d32 = float(f32_dist((cx, 0.0, 0.0), (tx, 0.0, 0.0)))
        # a few f32 ulp (3.7e-9 at 0.05) are not to be had when the two must disagree: any margin > 0 on the f64 side, exact on the f32 side
        if (d32 < 0.05) == want32_near and (d64 < 0.05) == want64_near and abs(d64 - 0.05) > 1e-12:
            return cx, tx
    return None


FACE_N = [(-1.0, 0.0), (1.0, 0.0), (0.0, -1.0), (0.0, 1.0)]
DIRS8 = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]


def _unit(d):
    n = math.hypot(*d)
    return (d[0] / n, d[1] / n)


def _outside(p, u, gap, t=0.004):
    """cube centre such that the closest point of its footprint lies `gap` from p along the unit direction u (face or corner)"""
    c = []
    for k in range(2):
        c.append(p[k] + u[k] * gap + math.copysign(H, u[k]) if u[k] != 0 else p[k] + t)
    return c


def _inside(p, face, e_face, other, e_other):
    """cube centre such that the tool axis p is inside the footprint, e_face from `face` and e_other from `other` (a face of the other axis)"""
    c = [0.0, 0.0]
    for f, e in ((face, e_face), (other, e_other)):
        ax = f // 2
        c[ax] = p[ax] + e - H if f % 2 == 0 else p[ax] - e + H
    return c


def _z_in(z_out, calls=1, relax=0.1):
    return REST + (z_out - REST) / (1.0 - relax) ** calls


def build_cells(O, chain, m=M64, shift=(0.0, 0.0, 0.0), f32_only=False):
    """the table.  m: the margin; shift: added to p1 before placement (the ambiguity test); f32_only: the cells the f32 engine runs"""
    A = arms(O, chain)
    shift = np.array(shift, dtype=np.float64)
    cells = []
    rng = np.random.default_rng(7)

    def add(task, variant, arm, name, side, cube, want, step=20, target=None, d_last=None, vel=(0.0, 0.0), grip=0.0, off=(0.0, 0.0, 0.0),
            expect=None, f32=True, twostep=False):
        a = A[task][arm]
        aux = np.zeros(PUSH_AUX if task == "push" else PICK_AUX)
        aux[0:3] = cube
        aux[3:6] = target if target is not None else (cube[0] - 0.15, cube[1] + 0.12, 0.01)
        # well away from the 1e-5 deadband unless the cell is about it: the distance "was" 4 mm more (test_cube_cells checks the margin)
        aux[6] = math.dist(aux[0:3], aux[3:6]) + (0.0 if d_last == "same" else 0.004) if d_last in (None, "same") else d_last
        if task == "push":
            aux[7:9] = vel
        else:
            aux[7] = grip; aux[8:11] = off
        cells.append(Cell(name=name + "/" + side, task=task, variant=variant, arm=arm, q=a["q"], action=a["action"], step=int(step), aux=aux,
                          branch=name, side=side, want=want, expect=expect or {}, f32=f32, twostep=twostep))

    c = CONST
    r, below, erp_dt = c["push_tool_radius"], c["push_tool_below"], c["push_contact_erp"] / c["push_dt"]
    dec = c["push_friction"] * c["push_gravity"] * c["push_dt"]
    P = {nm: a["p1"] + shift for nm, a in A["push"].items()}

    # ---------------- push, model 1
    p = P["high"]; lo = p[2] - below
    for side, pen_v in (("in", 3 * m), ("out", -m)):
        add("push", "nofric", "high", "voverlap", side, _outside(p, (1.0, 0.0), r - m) + [_z_in(lo + pen_v - H)],
            dict(v_overlap=side == "in", h_overlap=True), expect=dict(vel=(erp_dt * m, 0.0) if side == "in" else (0.0, 0.0)))
    for arm, u in (("low", (1.0, 0.0)), ("mid", _unit((-1, 1))), ("low_y", (0.0, -1.0))):
        p = P[arm]
        for side, pen in (("in", m), ("out", -m)):
            add("push", "nofric", arm, "hgap_" + arm, side, _outside(p, u, r - pen) + [REST], dict(v_overlap=True, h_overlap=side == "in"),
                expect=dict(vel=(erp_dt * m * u[0], erp_dt * m * u[1])) if side == "in" else dict(vel=(0.0, 0.0), untouched=True))
    for arm in ("low", "low_y"):      # a resting arm, and one that moved this step
        p = P[arm]
        for i, d in enumerate(DIRS8):
            u = _unit(d)
            add("push", "nofric", arm, "dir8_" + arm, "d%d" % i, _outside(p, u, r - 0.01) + [REST], dict(outside=True, press=False, **{"vn<tgt": True}),
                expect=dict(vel=(erp_dt * 0.01 * u[0], erp_dt * 0.01 * u[1])), twostep=True)
    p = P["low"]
    for i, d in enumerate(((0, 1), (-1, -1))):
        u = _unit(d)
        add("push", "default", "low", "dir_fric", "d%d" % i, _outside(p, u, r - 0.01) + [REST], dict(outside=True, press=False, stop=False),
            expect=dict(vel=((erp_dt * 0.01 - dec) * u[0], (erp_dt * 0.01 - dec) * u[1])), twostep=True)
    # tool axis inside the footprint: each face nearest by m against a face of the other axis (no ties).  pen = e + r = 0.06 is past the
    # default split, so the contact only takes the approaching velocity away (default) or pushes at erp pen / dt (bigsplit)
    for arm in ("low", "low_y"):
        p = P[arm]; lo = p[2] - below
        for face, other in ((0, 2), (1, 3), (2, 1), (3, 0)):
            for side, (ef, eo) in (("f%d" % face, (0.015, 0.015 + m)), ("f%d" % other, (0.015 + m, 0.015))):
                near = face if side == "f%d" % face else other
                nf, no = FACE_N[face], FACE_N[other]
                cube = _inside(p, face, ef, other, eo) + [_z_in(lo + 0.08 - H)]
                add("push", "default", arm, "inside%d_%s" % (face, arm), side, cube, dict(outside=False, face=near, press=False, **{"pen<split": False}),
                    vel=(-0.05 * (nf[0] + no[0]), -0.05 * (nf[1] + no[1])), twostep=True)
                add("push", "bigsplit", arm, "inside%d_%s" % (face, arm), side, cube, dict(outside=False, face=near, press=False, **{"pen<split": True}),
                    twostep=True)
    p = P["low"]
    for side, pen in (("lo", 0.04 - m), ("hi", 0.04 + m)):
        add("push", "default", "low", "split", side, _outside(p, (0.0, 1.0), r - pen) + [REST], {"pen<split": side == "lo", "press": False})
    p = P["mid"]; pen_v = REST + H - (p[2] - below)
    for side, pen in (("side", pen_v - m), ("down", pen_v + m)):
        add("push", "default", "mid", "press", side, _outside(p, (-1.0, 0.0), r - pen) + [REST], dict(press=side == "down"),
            expect=dict(untouched=True) if side == "down" else None)
    p = P["mid_dn"]; pen_v = REST + H - (p[2] - below)      # the tool came down this step: the same edge with a moving arm
    for side, pen in (("side", pen_v - m), ("down", pen_v + m)):
        add("push", "default", "mid_dn", "press_dn", side, _outside(p, _unit((1, 1)), r - pen) + [REST], dict(press=side == "down"))
    p = P["low"]; u = (0.0, -1.0); tgt = erp_dt * 0.02
    for side, vn in (("below", tgt - erp_dt * m), ("above", tgt + erp_dt * m), ("fast", tgt + 0.05)):
        add("push", "nofric", "low", "vn", side, _outside(p, u, r - 0.02) + [REST], {"vn<tgt": side == "below", "press": False},
            vel=(0.01 + vn * u[0], vn * u[1]))
    # Coulomb friction, the cube away from the tool
    p = P["high"]; away = [p[0] + 0.15, p[1] + 0.10]
    for side, sp, f32 in (("stop_lo", dec * (1 - 1e-12), False), ("stop_hi", dec * (1 + 1e-12), False), ("slide", 0.05, True)):
        add("push", "default", "high", "fric", side, away + [REST], dict(h_overlap=False, landed=True, stop=side == "stop_lo"),
            vel=(0.6 * sp, -0.8 * sp), f32=f32, expect=dict(vel=(0.0, 0.0)) if side == "stop_lo" else
            (dict(vel=(0.6 * (0.05 - dec), -0.8 * (0.05 - dec))) if side == "slide" else None))
    add("push", "default", "high", "still", "rest", away + [REST], dict(moving=False, deadband=True), d_last="same",
        expect=dict(untouched=True, vel=(0.0, 0.0), reward=-1.0))
    # landing: call k = step + 2 around fall_land (13 by default; 13 / 12 in drop_hi / drop_lo): friction from the landing call on, free
    # fall through it
    zk = lambda k: c["push_place_z"] - FALL_C * k * (k + 1)
    for variant, land in (("default", 13), ("drop_hi", 13), ("drop_lo", 12), ("nofric", 13)):
        for k in (land - 1, land, land + 1):
            z_in = zk(k - 1) if k - 1 <= land else REST + (zk(land) - REST) * 0.9
            add("push", variant, "high", "land", "k%+d" % (k - land), away + [z_in], dict(free_fall=k <= land, landed=k >= land, h_overlap=False),
                step=k - 2, vel=(0.03, 0.04), expect=dict(z=zk(k) if k <= land else REST + (z_in - REST) * 0.9))
    # the first steps after reset(): step 0 (call 2) and step 1, a side hit in free fall (no friction yet)
    p = P["low"]
    for step in (0, 1):
        add("push", "default", "low", "first", "s%d" % step, _outside(p, (1.0, 0.0), r - 0.01) + [zk(step + 1)],
            dict(free_fall=True, landed=False, press=False), step=step, expect=dict(vel=(erp_dt * 0.01, 0.0), z=zk(step + 2)), twostep=True)

    # ---------------- push, model 0 (tool sphere, full push-out)
    re_ = c["push_eef_radius"]
    p = P["mid"]
    for name, sgn in (("m0band_below", -1.0), ("m0band_above", 1.0)):
        for side, dz in (("in", H + re_ - m), ("out", H + re_ + m)):
            cube = _outside(p, (1.0, 0.0), re_ - 0.01) + [p[2] + sgn * dz]
            add("push", "m0", "mid", name, side, cube, dict(band=side == "in"),
                expect=dict(xy=(cube[0] + 0.01, cube[1])) if side == "in" else dict(untouched=True))
    for side, gap in (("in", re_ - m), ("out", re_ + m)):
        cube = _outside(p, _unit((1, -1)), gap) + [REST]
        add("push", "m0", "mid", "m0gap", side, cube, {"band": True, "gap<r": side == "in"}, expect=None if side == "in" else dict(untouched=True))
    for arm in ("mid", "mid_xy"):
        for i, d in enumerate(DIRS8):
            u = _unit(d)
            cube = _outside(P[arm], u, re_ - 0.01) + [REST]
            add("push", "m0", arm, "m0dir8_" + arm, "d%d" % i, cube, dict(outside=True), expect=dict(xy=(cube[0] + 0.01 * u[0], cube[1] + 0.01 * u[1])))
    for side in ("under", "over"):
        p = P["travel_" + side]
        add("push", "m0", "travel_" + side, "m0travel", side, [p[0] + 0.005, p[1] - 0.003, REST], {"outside": False, "travel>=1mm": side == "over"},
            f32=False, expect=dict(untouched=True) if side == "under" else None)
    p = P["mid"]
    add("push", "m0", "mid", "m0press", "still", [p[0] - 0.004, p[1] + 0.006, REST], {"outside": False, "travel>=1mm": False}, f32=False,
        expect=dict(untouched=True))
    a = A["push"]["mid_xy"]; p = P["mid_xy"]
    mh = _unit(a["p1"][:2] - a["p0"][:2])
    for side, proj in (("pos", 0.025 - m), ("neg", 0.025 + m)):
        add("push", "m0r5", "mid_xy", "m0s", side, [p[0] + proj * mh[0], p[1] + proj * mh[1], p[2] - 0.01], {"outside": False, "travel>=1mm": True, "s>0": side == "pos"},
            expect=None if side == "pos" else dict(untouched=True))
    add("push", "m0", "mid_xy", "m0sweep", "swept", [p[0] + 0.004, p[1] - 0.006, REST], {"outside": False, "travel>=1mm": True, "s>0": True})

    # ---------------- pick (the tip sphere; the cube at rest unless the cell says otherwise)
    L, trig, jaw = c["pick_gripper_length"], c["pick_trigger_dis"], c["pick_jaw_half"]
    T = {nm: a["p1"] + L * a["axis"] + shift for nm, a in A["pick"].items()}
    t = T["side"]
    for side, g in (("in", re_ + trig - m), ("out", re_ + trig + m)):
        add("pick", "default", "side", "trig_side", side, [t[0] + g + H, t[1] + 0.004, REST], dict(trigger=side == "in"), f32=False,
            expect=dict(grip=1.0 if side == "in" else 0.0, untouched=True))
    t = T["above"]
    for side, g in (("in", re_ + trig - m), ("out", re_ + trig + m)):
        cube = [t[0] + 0.005, t[1] + 0.003, t[2] - g - H]
        add("pick", "m0", "above", "trig_above", side, cube, dict(trigger=side == "in"), f32=False,
            expect=dict(grip=2.0 if side == "in" else 0.0, untouched=True))
    gz = t[2] - (REST + H)
    for side, g in (("in", re_ + trig - m), ("out", re_ + trig + m)):
        gxy = math.sqrt(g * g - gz * gz)
        add("pick", "default", "above", "trig_diag", side, [t[0] - gxy - H, t[1] - 0.004, REST], dict(trigger=side == "in"), f32=False,
            expect=dict(grip=1.0 if side == "in" else 0.0, untouched=True))
    for side, dz in (("above", -m), ("below", m)):      # cube centre m below / above the tip, reached through two relaxing fall calls
        add("pick", "default", "above", "hold_z", side, [t[0] + 0.005, t[1] + 0.003, _z_in(t[2] + dz, 2)], dict(trigger=True, tip_above=side == "above", in_jaw=True),
            expect=dict(grip=2.0 if side == "above" else 1.0))
    a = A["pick"]["above_xy"]; t = T["above_xy"]
    for side, o in (("in", jaw - m), ("out", jaw + m)):      # then grip 1 sweeps the cube along the 2 cm of travel
        add("pick", "default", "above_xy", "jaw", side, [t[0] + 0.6 * o, t[1] - 0.8 * o, REST], dict(trigger=True, tip_above=True, in_jaw=side == "in"),
            expect=dict(grip=2.0, untouched=True) if side == "in" else dict(grip=1.0))
    t = T["above_dn"]
    for side, o in (("in", jaw - m), ("out", jaw + m)):      # the tip came straight down: grip 1 presses, nothing is swept
        add("pick", "default", "above_dn", "jaw_dn", side, [t[0] - 0.8 * o, t[1] + 0.6 * o, REST], dict(trigger=True, tip_above=True, in_jaw=side == "in"),
            expect=dict(grip=2.0 if side == "in" else 1.0, untouched=True))
    t = T["above"]
    for side, o in (("in", jaw - m), ("out", jaw + m)):      # along +x the jaw edge is the footprint's: grip 1 pushes the cube out by r - m
        add("pick", "default", "above", "jaw_x", side, [t[0] + o, t[1], REST], dict(trigger=True, tip_above=True, in_jaw=side == "in"),
            expect=dict(grip=2.0, untouched=True) if side == "in" else dict(grip=1.0, xy=(t[0] + o + (re_ - m), t[1])))
    # a closed, non-holding gripper never re-triggers and still pushes
    cube = [t[0] + 0.02 + H, t[1] + 0.004, REST]
    add("pick", "default", "above", "closed", "push", cube, dict(grip_in=1.0, outside=True), grip=1.0, expect=dict(grip=1.0, xy=(cube[0] + 0.01, cube[1])))
    add("pick", "default", "above", "closed", "open", cube, dict(grip_in=0.0, trigger=True, in_jaw=False), grip=0.0, expect=dict(grip=1.0, xy=(cube[0] + 0.01, cube[1])))
    add("pick", "default", "above", "closed", "nohold", [t[0] + 0.005, t[1] + 0.003, REST], dict(grip_in=1.0, outside=False), grip=1.0,
        expect=dict(grip=1.0, untouched=True), f32=False)
    t = T["above_xy"]
    add("pick", "default", "above_xy", "closed", "sweep", [t[0] + 0.005, t[1] + 0.003, REST], {"grip_in": 1.0, "outside": False, "s>0": True}, grip=1.0,
        expect=dict(grip=1.0))
    mh = _unit(A["pick"]["above_xy"]["p1"][:2] - A["pick"]["above_xy"]["p0"][:2])
    for side, proj in (("pos", 0.025 - m), ("neg", 0.025 + m)):
        add("pick", "r5", "above_xy", "picks", side, [t[0] + proj * mh[0], t[1] + proj * mh[1], _z_in(t[2] - 0.01, 2)],
            {"grip_in": 1.0, "outside": False, "travel>=1mm": True, "s>0": side == "pos"}, grip=1.0, expect=dict(grip=1.0))
    # a held cube rides with the tip, never below its rest height; its fall is skipped (step 3: a free cube would be in free fall)
    for arm in ("above_xy", "above_dn"):
        t = T[arm]
        for side, z in (("clamp", REST - m), ("free", REST + m)):
            off = (0.004, -0.003, z - t[2])
            add("pick", "default", arm, "held_" + arm, side, [0.3, 0.1, 0.3], dict(grip_in=2.0, clamped=side == "clamp"), step=3, grip=2.0, off=off,
                expect=dict(grip=2.0, off=off, xy=(t[0] + off[0], t[1] + off[1]), z=REST if side == "clamp" else t[2] + off[2]), twostep=True)
    t = T["hi"]
    add("pick", "default", "hi", "held_hi", "ride", [0.3, 0.1, 0.3], dict(grip_in=2.0, clamped=False), step=3, grip=2.0, off=(-0.01, 0.002, -0.02),
        expect=dict(grip=2.0, off=(-0.01, 0.002, -0.02), z=t[2] - 0.02))
    # the cube's fall, two calls per step (the first made up for from step 1 on), across the landing call 13
    far = list(FAR["pick"])
    z1 = {0: zk(1), 5: zk(10), 6: zk(12)}
    z1[7] = REST + (zk(13) - REST) * 0.9
    zo = {0: zk(2), 5: zk(12), 6: REST + (zk(13) - REST) * 0.9, 7: REST + (z1[7] - REST) * 0.81}
    for s in (0, 5, 6, 7):
        add("pick", "default", "side", "pickfall", "s%d" % s, far + [z1[s]], dict(free_fall=s <= 5, trigger=False), step=s, expect=dict(z=zo[s], grip=0.0))
    add("pick", "m0", "side", "pickfall_m0", "s5", far + [zk(10)], dict(trigger=False), step=5, expect=dict(z=zk(10), grip=0.0))

    # ---------------- outcome block, both tasks: the cube at rest and away from the tool; distances along x only are exact in every
    # arithmetic (fused or not), general ones keep 16 ulp
    for task, variant, arm in (("push", "default", "high"), ("pick", "default", "hi")):
        cx, cy = FAR[task]
        cube = [cx, cy, REST]
        kw = dict(f32=False)
        idle = dict(moving=False) if task == "push" else dict(trigger=False)
        for nm, target, ulp in (("dead_x", (cx + 0.2, cy, REST), 2), ("dead_g", (cx + 0.12, cy + 0.15, 0.01), 16)):
            d_cur = math.sqrt((cube[0] - target[0]) ** 2 + (cube[1] - target[1]) ** 2 + (cube[2] - target[2]) ** 2)
            for sn, sign in (("pos", 1.0), ("neg", -1.0)):      # the sign of test = d_cur - d_last
                a_in, a_out = _deadband_edge(d_cur, sign, ulp)
                add(task, variant, arm, nm + "_" + sn, "in", cube, dict(deadband=True, **idle), target=target, d_last=a_in, expect=dict(reward=-1.0, done=False), **kw)
                add(task, variant, arm, nm + "_" + sn, "out", cube, dict(deadband=False, **idle), target=target, d_last=a_out,
                    expect=dict(reward=-100.0 * (d_cur - a_out), done=False), **kw)
        target = (cx + 0.2, cy, REST)
        for step in (499, 500, 501):      # the counter before the step; done when the incremented counter exceeds max_steps = 500
            d32 = float(f32_dist(cube, target))
            add(task, variant, arm, "tmo", "s%d" % step, cube, dict(timeout=step >= 500, near32=False, **idle), target=target, step=step,
                expect=dict(done=step >= 500, success=False, reward=float(np.float32(-d32) * np.float32(50.0)) if step >= 500 else 0.4))
        # success distance: f32 distance a few f32 ulp either side of 0.05 (both distances on the same side), along x
        tx = 0.0      # the f32 distance is then the cube's f32 x itself
        lo32 = np.float32(0.05)
        while float(lo32) >= 0.05:
            lo32 = np.nextafter(lo32, np.float32(0))
        for sn, d32 in (("in", float(np.nextafter(np.nextafter(lo32, np.float32(0)), np.float32(0)))),
                        ("out", float(np.nextafter(np.nextafter(np.nextafter(lo32, np.float32(1)), np.float32(1)), np.float32(1))))):
            cxs = d32
            assert float(f32_dist((cxs, 0, 0), (tx, 0, 0))) == d32
            add(task, variant, arm, "succ", sn, [cxs, cy, REST], dict(near32=sn == "in", near64=sn == "in", timeout=False, **idle), target=(tx, cy, REST),
                expect=dict(done=sn == "in", success=sn == "in", **(dict(reward=100.0) if sn == "in" else {})), **kw)
        # the f32 distance (done, +100) and the f64 distance (success) on different sides of 0.05: found by search, both ways
        for sn, n32, n64 in (("done_nosucc", True, False), ("succ_notdone", False, True)):
            hit = _success_split(rng, n32, n64)
            assert hit is not None, "no cube / target pair splits the f32 and f64 distances around 0.05 (%s)" % sn
            add(task, variant, arm, "succ_split", sn, [hit[0], cy, REST], dict(near32=n32, near64=n64, timeout=False, **idle), target=(hit[1], cy, REST),
                expect=dict(done=n32, success=n64, **(dict(reward=100.0) if n32 else {})), **kw)
        # time-out and success in the same step: the time-out reward wins, success is reported
        tx = 0.5
        cxs = tx + 0.03
        add(task, variant, arm, "tmo_succ", "s500", [cxs, cy, REST], dict(timeout=True, near32=True, near64=True, **idle), target=(tx, cy, REST), step=500,
            expect=dict(done=True, success=True, reward=float(np.float32(-f32_dist((cxs, cy, REST), (tx, cy, REST))) * np.float32(50.0))))
        add(task, variant, arm, "tmo_succ", "s499", [cxs, cy, REST], dict(timeout=False, near32=True, near64=True, **idle), target=(tx, cy, REST), step=499,
            expect=dict(done=True, success=True, reward=100.0))
    # a time-out while the cube is being pushed / carried (done with a moving cube: auto-reset must zero velocity, grip and offset)
    p = P["low"]
    add("push", "default", "low", "tmo_moving", "s500", _outside(p, (1.0, 0.0), r - 0.01) + [REST], dict(timeout=True, press=False), step=500, vel=(0.02, 0.01),
        expect=dict(done=True))
    t = T["above_xy"]
    add("pick", "default", "above_xy", "tmo_held", "s500", [0.3, 0.1, 0.3], dict(timeout=True, grip_in=2.0), step=500, grip=2.0, off=(0.004, -0.003, -0.01),
        expect=dict(done=True, grip=2.0))
    if f32_only:
        cells = [x for x in cells if x.f32]
    return cells


# ------------------------------------------------------------------ running rows through the oracle, comparing results

def groups(cells):
    """(task, variant) -> cells, in table order"""
    g = {}
    for x in cells:
        g.setdefault((x.task, x.variant), []).append(x)
    return g


def rows_of(cells, idx):
    q = np.array([cells[i].q for i in idx], dtype=np.float64)
    aux = np.array([cells[i].aux for i in idx], dtype=np.float64)
    step = np.array([cells[i].step for i in idx], dtype=np.int32)
    act = np.array([cells[i].action for i in idx], dtype=np.float32)
    return q, aux, step, act


def run_oracle(O, chain, task, cfg, q, aux, step, act, auto_reset=False, seed=0, nsteps=1):
    """the rows through the oracle (the engine's state after reset(): episode 1, return 0).  Returns a dict of arrays."""
    n = len(q)
    st = (O.PushState if task == "push" else O.PickState)(n)
    st.q[:] = q; st.aux[:] = aux; st.step[:] = step; st.episode[:] = 1
    iters, minpiv = np.zeros(n, dtype=np.int32), np.zeros(n)
    out = None
    for _ in range(nsteps):
        if auto_reset:
            fn = O.push_step_autoreset if task == "push" else O.pick_step_autoreset
            obs, rew, done, succ, term = fn(chain, cfg, st, act, seed=seed, iters=iters, minpiv=minpiv)
        else:
            fn = O.push_step if task == "push" else O.pick_step
            obs, rew, done, succ, it = fn(chain, cfg, st, act, minpiv=minpiv)
            iters, term = it, obs
        out = dict(q=st.q.copy(), aux=st.aux.copy(), step=st.step.copy(), episode=st.episode.copy(), obs=obs.copy(), reward=rew.copy(),
                   done=done.astype(bool), success=succ.astype(bool), term=term.copy(), iters=iters.copy(), minpiv=minpiv.copy())
    return out


def tolerances(precision, consts):
    """the engine's stated per-step agreement with the oracle and what follows from it (see tests/test_gpu_cube_cells.py)"""
    pos = PERTURB[precision]
    return dict(pos=pos, vel=pos * consts["push_contact_erp"] / consts["push_dt"], shaped=200.0 * pos, timeout=50.0 * (pos + 2.0 ** -25))      # 2^-25: one f32 ulp of a distance in [0.25, 0.5)


def differs(task, a, b, i, j, tol):
    """do row i of result a and row j of result b differ in an asserted output beyond the tolerance (or in a discrete / exact one)?"""
    for k in ("done", "success", "step"):
        if a[k][i] != b[k][j]:
            return k
    x, y = a["aux"][i], b["aux"][j]
    if task == "pick" and x[7] != y[7]:
        return "grip"
    if np.abs(x[0:7] - y[0:7]).max() > tol["pos"]:
        return "cube/target/d_last"
    if task == "pick":
        if np.abs(x[8:11] - y[8:11]).max() > tol["pos"]:
            return "off"
    else:
        if np.abs(x[7:9] - y[7:9]).max() > tol["vel"]:
            return "vel"
        if (not x[7:9].any()) != (not y[7:9].any()):
            return "vel==0"
    ra, rb = a["reward"][i], b["reward"][j]
    for fixed in (100.0, -1.0):
        if (ra == fixed) != (rb == fixed):
            return "reward==%g" % fixed
    if abs(ra - rb) > (tol["timeout"] if a["done"][i] else tol["shaped"]):
        return "reward"
    return None
