"""Cell table of the reach step's decisions -- the Cartesian clip of the IK target (all three tasks) and, for reach, everything after
the IK: the time-out, the success distance, the precedence of the two, the reward select, the bookkeeping of a finished episode and the
in-place reset.  A cell is one env step (a few are two) whose input state sits a known margin to one side of ONE decision and well
inside every other one.  tests/test_reach_cells.py checks the table on the CPU (every cell lands in its branch, none is ambiguous under
the engine's allowed disagreement, model == oracle, every planted defect is caught, every constant is pinned);
tests/test_gpu_reach_cells.py runs it through the HIP kernels.  Layout and names follow tests/cube_cells.py.

Placement is two-pass, as in cube_cells.arms: a probe step of the oracle from the cell's start pose and action gives the flange before
and after the IK (p0, p1); the goal (f32), the step counter, the episode counter and the running return of a cell are then written
relative to p1.  Start poses come from O.ik from q_init to a named flange target (16 calls, so that the pose is a fixed point); every
one must converge below the iteration cap with its smallest pivot above fence_pivot and no IK trip within 2e-6 of the 1e-4 residual
gate (test_reach_cells.test_arm_poses_are_well_conditioned).

Margins: M64 = 1e-5 m for the f64 engine, M32 = 1e-3 for the f32 engine -- ten times the stated per-step agreement of 1e-6 / 1e-4, the
rule and constants of cube_cells.  The f32 table is rebuilt from start poses rounded to f32 and with its own margin.  The step counter
is an integer: its cells sit on max_steps - 1, max_steps and max_steps + 1 exactly.

`model_step` is a float64 restatement of the step as the step paragraph of include/armenv.h and ArmEnvConfig's field comments give it
(FK -> add dv * action -> clip to the box -> IK -> FK -> counter, distance from the f32 goal, three-way outcome, reward, observation,
terminal observation, episode accounting, in-place reset), written without reference to the kernel.  It uses the oracle for FK, IK and
the Philox uniforms of the goal draw only, and returns the `trace` of the decisions it took.

What the table cannot pin: the STRICTNESS of the two floating-point compares at exact equality (`dist < reach_dis`, and `v < lo` /
`v > hi` of the clip).  A cell on the edge itself would need the engine's flange to equal the oracle's to the last bit; the engine is
allowed 1e-6.  `reach_dis/zero` (distance 0 in the variant `never`, reach_dis = 0) pins `<` against `<=` at the one place where the
edge is reachable: dist >= 0 always, so `dist <= 0` would succeed on an exact hit and `dist < 0` never does -- and even there the hit is
exact only if the flange is f32-representable; the cell says which it got (`expect["nearest"]`).  The clip's `clip_face/on` cell sits
on a face to within the IK's residual; either side gives the same target to that residual, and its trace says which it took.  The
time-out is an integer compare and IS pinned at equality (`timeout/s0`).

One planted defect is below every tolerance of the GPU test and is pinned on the CPU only: a distance taken to the goal BEFORE its
rounding to f32 differs from the stated one by at most half an f32 ulp of a coordinate (3e-8 m at 0.5), the reward by 3e-7, against
margins of 1e-5 and a reward tolerance of 1e-5.  The model-against-oracle check (1e-12) sees it; test_reach_cells says so per defect.

Default-box faces (KUKA).  The CPU probe finds a converging, well-conditioned start pose 0.35 dv inside every face of the default
reach box, so none is left out: x_lo (0.207, 0, 0.3) pose pivot 3.6e-2, step 3 updates, x_hi (0.693, 0.1, 0.15) 1.8e-1 / 3 (at (0.693, 0, 0.3) an IK trip ends 6e-7 from the residual gate), y_lo
(0.5, -0.293, 0.3) 2.3e-1 / 2, y_hi 2.6e-1 / 2, z_lo (0.5, 0, 0.007) 1.2e-1 / 2, z_hi (0.5, 0, 0.543) 8.6e-2 / 2; push's ceiling 0.1
from (0.5, 0, 0.072) 1.3e-1 / 3; pick's ceiling 0.55 + 0.257 for the flange from (0.4, 0, 0.779) 1.6e-1 / 4 (poses further out, at
x = 0.3 or 0.45, leave a joint 0.34-0.38 rad beyond its URDF limit and were not used).  At x_lo joint 4 stands 0.54 rad beyond its URDF
limit, which the default clamp_joint_limits = 0 ignores; the cell is kept (the criteria are convergence and conditioning).

The small box (variant `smallbox`, KUKA): FK(q_init) = (0.532054, -0.001121, 0.496298); box_lo = (0.507, -0.031, 0.469), box_hi =
(0.567, 0.036, 0.529): every bound 2.5 to 3.7 cm from the reset pose, no two equal, |lo| != |hi| on every axis.  A face pair starts
0.35 dv inside the face; `out` pushes 0.7 dv across it (0.35 dv past it unclipped: 7 mm for reach, 28 mm for push and pick), `in` has
the sign reversed and clips nowhere.  For push and pick (dv = 0.08) the reversed action is -0.2, not -0.7: 1.05 dv = 8.4 cm is wider
than any box whose faces lie within 4 cm of the reset pose, so the full reversal would clip on the opposite face.
"""
import math

import numpy as np

import cube_cells as CC

M64, M32 = CC.M64, CC.M32
PERTURB = CC.PERTURB      # the engine's allowed per-step disagreement with the oracle
GATE_BAND = 2e-6          # no IK trip of a cell may end this close to the 1e-4 residual gate (a flipped trip moves q by ~1e-4)

# include/armenv.h defaults, restated for the model (pinned to O.default_config by test_reach_cells)
CONST = dict(reach_dis=0.01, max_steps=500,
             dv=dict(reach=0.02, push=0.08, pick=0.08),
             box_lo=(0.2, -0.3, 0.0),
             box_hi=dict(reach=(0.7, 0.3, 0.55), push=(0.7, 0.3, 0.1), pick=(0.7, 0.3, 0.55 + 0.257)),
             goal_lo=(0.2, -0.3, 0.0), goal_hi=(0.7, 0.3, 0.55))
SMALLBOX = dict(box_lo=(0.507, -0.031, 0.469), box_hi=(0.567, 0.036, 0.529))
VARIANTS = {
    "reach": {"default": {}, "short": dict(max_steps=3), "zero": dict(max_steps=0), "never": dict(reach_dis=0.0), "wide": dict(reach_dis=10.0),
              "smallbox": SMALLBOX},
    "push": {"default": {}, "smallbox": SMALLBOX},
    "pick": {"default": {}, "smallbox": SMALLBOX},
}
OUTCOME_VARIANTS = ("default", "short", "zero", "never", "wide")
AXES = "xyz"
FACES = [(k, s) for k in range(3) for s in ("lo", "hi")]
IN_ACTION = {"reach": 0.7, "push": 0.2, "pick": 0.2}      # magnitude of the reversed action of a face pair's `in` twin (module docstring)

# start poses of the outcome cells: flange target as an offset from FK(q_init), action
OUTCOME_ARMS = {
    "still": ((-0.03, 0.05, -0.10), (0.0, 0.0, 0.0)),
    "still2": ((0.02, -0.06, -0.15), (0.0, 0.0, 0.0)),
    "move": ((-0.05, -0.04, -0.12), (0.3, -0.2, 0.25)),
    "down": ((0.0, 0.08, -0.2), (0.0, 0.0, -0.5)),
}
# default-box faces: task -> face name -> (flange target with the face's own coordinate left to the builder, face axis, side)
DEFAULT_FACES = {
    "reach": {"x_lo": ((None, 0.0, 0.3), 0, "lo"), "x_hi": ((None, 0.1, 0.15), 0, "hi"), "y_lo": ((0.5, None, 0.3), 1, "lo"),
              "y_hi": ((0.5, None, 0.3), 1, "hi"), "z_lo": ((0.5, 0.0, None), 2, "lo"), "z_hi": ((0.5, 0.0, None), 2, "hi")},
    "push": {"z_hi": ((0.5, 0.0, None), 2, "hi")},
    "pick": {"z_hi": ((0.4, 0.0, None), 2, "hi")},
}


class Cell:
    __slots__ = ("name", "task", "variant", "arm", "q", "action", "step", "goal", "aux", "episode", "ep_return", "branch", "side", "want", "expect",
                 "twostep", "zero_action")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def __repr__(self):
        return "<%s %s/%s %s>" % (self.task, self.variant, self.name, self.arm)


# ------------------------------------------------------------------ chains, configs, constants

_SETUP = {}


def setup(O, robot):
    """config overrides of a chain: none for KUKA; for Diana the reachable set-up tests/test_gpu_parity.py uses for the second chain"""
    if robot not in _SETUP:
        if robot == "kuka":
            _SETUP[robot] = {}
        else:
            q_init = [0.0, 0.5, 0.0, 1.6, 0.0, -1.0, 0.0]
            p, _ = O.fk(O.make_chain(robot), q_init)
            lo, hi = (p[0] - 0.25).tolist(), (p[0] + 0.25).tolist()
            _SETUP[robot] = dict(target_quat=[1.0, 0.0, 0.0, 0.0], q_init=q_init, box_lo=lo, box_hi=hi, goal_lo=lo, goal_hi=hi)
    return _SETUP[robot]


def overrides(O, task, variant, robot="kuka"):
    """what a handle of this variant is created with, beyond the defaults (lists for array fields)"""
    kw = dict(setup(O, robot))
    kw.update({k: (list(v) if isinstance(v, tuple) else v) for k, v in VARIANTS[task][variant].items()})
    return kw


def make_cfg(O, task, variant, robot="kuka"):
    cfg = O.default_config(task, robot)
    for k, v in overrides(O, task, variant, robot).items():
        if hasattr(getattr(cfg, k), "__len__"):
            getattr(cfg, k)[:] = v
        else:
            setattr(cfg, k, v)
    return cfg


def constants(O, task, variant, robot="kuka"):
    """the model's constants: the header's defaults restated above, the chain's set-up, the variant"""
    c = dict(reach_dis=CONST["reach_dis"], max_steps=CONST["max_steps"], dv=CONST["dv"][task], box_lo=CONST["box_lo"], box_hi=CONST["box_hi"][task],
             goal_lo=CONST["goal_lo"], goal_hi=CONST["goal_hi"], q_init=tuple(O.INIT_Q))
    c.update(overrides(O, task, variant, robot))
    c.pop("target_quat", None)
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in c.items()}


# ------------------------------------------------------------------ the model (float64, from include/armenv.h)

DEFECTS = ("timeout_ge", "success_first", "success_reward", "timeout_reward0", "dist_f64_goal",
           "no_lo0", "no_hi0", "no_lo1", "no_hi1", "no_lo2", "no_hi2", "clip_other_axis",
           "last_len_off", "ep_return_kept", "episode_kept", "term_after_reset", "obs_not_reset", "reset_always", "last_success_timeout")
CPU_ONLY_DEFECTS = ("dist_f64_goal",)      # below the GPU test's tolerances by construction (module docstring)
_IK_MEMO = {}


def _arm(O, chain, cfg, task, q, tgt):
    key = (id(chain), task, q.tobytes(), tgt.tobytes(), cfg.ik_max_iters)
    if key not in _IK_MEMO:
        res, it = O.ik(chain, cfg, q, tgt)
        q1 = res[0].copy()
        if task == "pick":
            q1[6] = q[6]                   # the pick task applies the IK result to joints 0..5 only
        p1, _ = O.fk(chain, q1)
        _IK_MEMO[key] = (q1, p1[0].copy(), int(it[0]))
    return _IK_MEMO[key]


def new_goal(O, c, seed, env_id, episode):
    """goal ~ U(goal box) per axis from the env's Philox stream (draw 0 of (seed, global id, episode)), cast to f32"""
    u = O.draw6(seed, int(env_id), int(episode), 0)
    return np.array([c["goal_lo"][k] + (c["goal_hi"][k] - c["goal_lo"][k]) * u[k] for k in range(3)], dtype=np.float32)


def model_step(O, chain, cfg, c, task, st, action, env_id=0, seed=0, auto_reset=False, defect=None, goal64=None):
    """One env step.  st: dict(q, goal f32[3], step, episode, ep_return) (push / pick: q and step only -- the arm and its clip are all
    this model restates of them).  Returns the state after the step, the step's outputs, `ended` (None or the finished episode's
    (return, length, success)) and the trace.  cfg: the oracle's config, for its IK parameters only.  defect: one of DEFECTS."""
    q = np.array(st["q"], dtype=np.float64)
    tr = {}
    p0 = O.fk(chain, q)[0][0]
    a = np.asarray(action, dtype=np.float32).astype(np.float64)
    start = p0.astype(np.float32).astype(np.float64) if task == "pick" else p0      # pick: the start position goes through float32
    tgt = np.zeros(3)
    for k in range(3):
        v = start[k] + a[k] * c["dv"]
        kb = (k + 1) % 3 if defect == "clip_other_axis" else k
        lo, hi = c["box_lo"][kb], c["box_hi"][kb]
        tr["lo%d" % k], tr["hi%d" % k] = bool(v < c["box_lo"][k]), bool(v > c["box_hi"][k])
        if v < lo and defect != "no_lo%d" % k:
            v = lo
        elif v > hi and defect != "no_hi%d" % k:
            v = hi
        tgt[k] = v
    q1, p1, iters = _arm(O, chain, cfg, task, q, tgt)
    step = int(st["step"]) + 1
    out = dict(q=q1, eef=p1, step=step, iters=iters, trace=tr, p0=p0, tgt=tgt)
    if task != "reach":
        return out
    goal = np.array(st["goal"], dtype=np.float32)
    g = goal.astype(np.float64) if not (defect == "dist_f64_goal" and goal64 is not None) else np.array(goal64, dtype=np.float64)
    dist = math.sqrt((p1[0] - g[0]) ** 2 + (p1[1] - g[1]) ** 2 + (p1[2] - g[2]) ** 2)
    over = step >= c["max_steps"] if defect == "timeout_ge" else step > c["max_steps"]
    near = dist < c["reach_dis"]
    tr["timeout"], tr["near"] = bool(over), bool(near)
    if defect == "success_first" and near:
        reward, done, success = 0.0, True, True
    elif over:
        reward, done, success = (0.0 if defect == "timeout_reward0" else -10.0 * dist), True, False
    elif near:
        reward, done, success = (-10.0 * dist if defect == "success_reward" else 0.0), True, True
    else:
        reward, done, success = -10.0 * dist, False, False
    ep_return = float(st["ep_return"]) + reward
    episode = int(st["episode"])
    obs = np.concatenate([p1.astype(np.float32), goal])
    term = obs.copy()
    ended, reset = None, False
    if done:
        ended = (ep_return, step - 1 if defect == "last_len_off" else step, True if defect == "last_success_timeout" else success)
        if auto_reset or defect == "reset_always":
            reset = True
            goal = new_goal(O, c, seed, env_id, episode)
            if defect != "episode_kept":
                episode += 1
            q1 = np.array(c["q_init"], dtype=np.float64)
            step = 0
            if defect != "ep_return_kept":
                ep_return = 0.0
            p_init = O.fk(chain, q1)[0][0]
            if defect != "obs_not_reset":
                obs = np.concatenate([p_init.astype(np.float32), goal])
            if defect == "term_after_reset":
                term = obs.copy()
    tr["reset"] = reset
    out.update(q=q1, goal=goal, step=step, episode=episode, ep_return=ep_return, obs=obs, term=term, reward=reward, done=done, success=success,
               ended=ended, dist=dist)
    return out


FIELDS = ("q", "goal", "step", "episode", "ep_return", "obs", "term", "reward", "done", "success", "eef", "last_return", "last_len", "last_success",
          "ended", "n_done", "n_success")


def model_run(O, chain, cfg, c, x, env_id=0, seed=0, auto_reset=False, nsteps=1, defect=None):
    """a reach cell through `nsteps` steps of the model: the last step's outputs, the state after it, the statistics of the episode
    that ended last (`ended`: did one end), the number of finished episodes and successes, and each step's trace"""
    st = dict(q=x.q, goal=x.goal, step=x.step, episode=x.episode, ep_return=x.ep_return)
    last, n_done, n_succ, traces, dists = None, 0, 0, [], []
    goal64 = x.expect.get("goal64")
    for t in range(nsteps):
        r = model_step(O, chain, cfg, c, "reach", st, x.action, env_id, seed, auto_reset, defect, goal64 if t == 0 else None)
        traces.append(r["trace"]); dists.append(r["dist"])
        if r["ended"] is not None:
            last = r["ended"]; n_done += 1; n_succ += int(r["success"])
        st = r
    out = {k: r[k] for k in ("q", "goal", "step", "episode", "ep_return", "obs", "term", "reward", "done", "success", "eef")}
    out.update(last_return=last[0] if last else 0.0, last_len=last[1] if last else 0, last_success=bool(last[2]) if last else False,
               ended=last is not None, n_done=n_done, n_success=n_succ, traces=traces, dists=dists)
    return out


def stack(results):
    """list of model_run results -> dict of arrays over the rows"""
    return {k: np.array([r[k] for r in results]) for k in FIELDS}


def tolerances(precision, nsteps=1):
    """the project's stated per-step agreement and what follows from it, as tests/test_gpu_cube_cells.py applies it"""
    pos = PERTURB[precision]
    return dict(pos=pos, reward=10.0 * pos, nsteps=nsteps)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def compare(g, r, tol, worst=None, ulp=True):
    """result g (an engine's, or a defective model's) against the model's r, row by row over every checked output.  Returns the list of
    (row, output, deviation) that miss; worst (optional dict) receives the largest deviation per toleranced output."""
    bad = []
    n = len(r["done"])

    def exact(name, a, b, rows=None):
        ne = np.asarray(a) != np.asarray(b)
        ne = ne.reshape(n, -1).any(1)
        if rows is not None:
            ne &= rows
        bad.extend((int(i), name, None) for i in np.flatnonzero(ne))

    def close(name, a, b, t, rows=None):
        d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).reshape(n, -1).max(1)
        if rows is not None:
            d = np.where(rows, d, 0.0)
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), float(d.max(initial=0.0)))
        bad.extend((int(i), name, float(d[i])) for i in np.flatnonzero(d > t))

    ended = np.asarray(r["ended"], dtype=bool)
    for k in ("done", "success", "step", "episode", "ended"):
        exact(k, g[k], r[k])
    exact("goal", np.asarray(g["goal"], dtype=np.float32).view(np.uint32), np.asarray(r["goal"], dtype=np.float32).view(np.uint32))
    exact("obs_goal", np.asarray(g["obs"], dtype=np.float32)[:, 3:].view(np.uint32), np.asarray(r["obs"], dtype=np.float32)[:, 3:].view(np.uint32))
    exact("term_goal", np.asarray(g["term"], dtype=np.float32)[:, 3:].view(np.uint32), np.asarray(r["term"], dtype=np.float32)[:, 3:].view(np.uint32))
    exact("last_len", g["last_len"], r["last_len"], ended)
    exact("last_success", g["last_success"], r["last_success"], ended)
    exact("n_done", g["n_done"], r["n_done"])
    exact("n_success", g["n_success"], r["n_success"])
    succ = np.asarray(r["success"], dtype=bool)
    exact("reward==0", np.asarray(g["reward"]) == 0.0, np.ones(n, dtype=bool), succ)      # exact by construction
    close("q", g["q"], r["q"], tol["pos"])
    close("obs", g["obs"], r["obs"], tol["pos"])
    close("terminal_obs", g["term"], r["term"], tol["pos"])
    rt = tol["reward"] + (_ulp32(r["reward"]) if ulp else 0.0)      # ulp: one f32 ulp of the reward, for its f32 store
    close("reward", g["reward"], r["reward"], rt)
    close("ep_return", g["ep_return"], r["ep_return"], tol["nsteps"] * rt)
    close("last_return", g["last_return"], r["last_return"], tol["nsteps"] * rt, ended)
    return bad


# ------------------------------------------------------------------ the arm: poses and probe

_ARM_CACHE = {}


def _pose(O, chain, cfg, task, tgt):
    q = np.array(cfg.q_init[:], dtype=np.float64)
    for _ in range(16):
        res, _ = O.ik(chain, cfg, q, np.array(tgt, dtype=np.float64))
        if task == "pick":
            q[:6] = res[0, :6]
        else:
            q = res[0].copy()
    return q


def _gate(O, chain, cfg, q, tgt, iters):
    """smallest distance of an IK trip's position residual from the residual gate over the call (the loop tests the residual of the
    pose each trip starts from)"""
    best, cap = math.inf, cfg.ik_max_iters
    try:
        for k in range(iters + (1 if iters >= cap else 0)):      # the pose the last update leaves is not tested below the cap
            cfg.ik_max_iters = k
            qk = O.ik(chain, cfg, q, tgt)[0][0] if k else q
            pk = O.fk(chain, qk)[0][0]
            best = min(best, abs(float(np.linalg.norm(pk - tgt)) - cfg.ik_residual))
    finally:
        cfg.ik_max_iters = cap
    return best


def arm_rows(O, task, variant, robot):
    """name -> (flange target of the start pose, action) of the arms a (task, variant) uses"""
    rows = {}
    dv = CONST["dv"][task]
    if task == "reach" and variant in OUTCOME_VARIANTS:
        p_init = O.fk(O.make_chain(robot), make_cfg(O, task, variant, robot).q_init[:])[0][0]
        for nm, (off, act) in OUTCOME_ARMS.items():
            rows[nm] = (tuple(p_init + np.array(off)), act)
    if robot != "kuka":
        return rows
    if variant == "default":
        lo, hi = CONST["box_lo"], CONST["box_hi"][task]
        for nm, (tgt, k, side) in DEFAULT_FACES[task].items():
            t = list(tgt)
            t[k] = lo[k] + 0.35 * dv if side == "lo" else hi[k] - 0.35 * dv
            sgn = -1.0 if side == "lo" else 1.0
            for tw, mag in (("out", 0.7 * sgn), ("in", -IN_ACTION[task] * sgn)):
                act = [0.0, 0.0, 0.0]; act[k] = mag; act[(k + 1) % 3 if k < 2 else 0] = 0.15
                rows["dflt_%s_%s" % (nm, tw)] = (tuple(t), tuple(act))
    if variant == "smallbox":
        lo, hi = SMALLBOX["box_lo"], SMALLBOX["box_hi"]
        mid = [(lo[k] + hi[k]) / 2 for k in range(3)]
        for k, side in FACES:
            t = list(mid)
            t[k] = lo[k] + 0.35 * dv if side == "lo" else hi[k] - 0.35 * dv
            sgn = -1.0 if side == "lo" else 1.0
            for tw, mag in (("out", 0.7 * sgn), ("in", -IN_ACTION[task] * sgn)):
                act = [0.0, 0.0, 0.0]; act[k] = mag; act[(k + 1) % 3] = 0.15 if k != 1 else -0.15
                rows["sb_%s_%s_%s" % (AXES[k], side, tw)] = (tuple(t), tuple(act))
        t = list(mid); t[0] = hi[0] - 0.35 * dv; t[1] = lo[1] + 0.35 * dv
        rows["sb_two"] = (tuple(t), (0.7, -0.7, 0.15))
        t = list(mid); t[2] = lo[2]
        rows["sb_on"] = (tuple(t), (0.0, 0.0, 0.0))
    return rows


def arms(O, chain, robot="kuka", f32=False):
    """(task, variant) -> name -> dict(q, action, p0, p1, q1, iters, minpiv, pose_pivot, gate) by a probe step of the oracle; f32: the
    start poses rounded to f32 first (the f32 engine's table)"""
    key = (robot, f32)
    if key in _ARM_CACHE:
        return _ARM_CACHE[key]
    out = {}
    for task in VARIANTS:
        for variant in VARIANTS[task]:
            rows = arm_rows(O, task, variant, robot)
            if not rows:
                continue
            cfg = make_cfg(O, task, variant, robot)
            names = list(rows)
            qs = []
            for nm in names:
                pk = (robot, task, rows[nm][0])
                if pk not in _ARM_CACHE:
                    _ARM_CACHE[pk] = _pose(O, chain, make_cfg(O, task, "default", robot), task, rows[nm][0])
                q = _ARM_CACHE[pk]
                qs.append(q.astype(np.float32).astype(np.float64) if f32 else q)
            n = len(names)
            acts = np.array([rows[nm][1] for nm in names], dtype=np.float32)
            st = {"reach": O.ReachState, "push": O.PushState, "pick": O.PickState}[task](n)
            st.q[:] = np.array(qs); st.step[:] = 20
            if task == "reach":
                st.goal[:] = 0.0
            else:      # the cube parked out of every tool's way, at rest; pick's gripper closed (it never triggers)
                st.aux[:, 0:2] = CC.FAR[task]; st.aux[:, 2] = CC.REST
                st.aux[:, 3:6] = (0.6, 0.25, 0.01); st.aux[:, 6] = 0.6
                if task == "pick":
                    st.aux[:, 7] = 1.0
            aux0 = None if task == "reach" else st.aux.copy()
            minpiv = np.zeros(n)
            p0, _ = O.fk(chain, st.q)
            step = {"reach": O.reach_step, "push": O.push_step, "pick": O.pick_step}[task]
            _, _, _, _, iters = step(chain, cfg, st, acts, minpiv=minpiv)
            p1, _ = O.fk(chain, st.q)
            d = {}
            for i, nm in enumerate(names):
                start = p0[i].astype(np.float32).astype(np.float64) if task == "pick" else p0[i]
                tgt = np.clip(start + acts[i].astype(np.float64) * cfg.dv, cfg.box_lo[:], cfg.box_hi[:])
                d[nm] = dict(q=np.array(qs[i]), action=acts[i].copy(), p0=p0[i].copy(), p1=p1[i].copy(), q1=st.q[i].copy(), iters=int(iters[i]),
                             minpiv=float(minpiv[i]), pose_pivot=float(O.pose_min_pivot(chain, cfg, np.array(qs[i]))[0]),
                             gate=_gate(O, chain, cfg, np.array(qs[i]), tgt, int(iters[i])), aux=None if aux0 is None else aux0[i].copy(),
                             target=rows[nm][0])
            out[(task, variant)] = d
    _ARM_CACHE[key] = out
    return out


# ------------------------------------------------------------------ the cells

def _unit(v):
    v = np.array(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def build_cells(O, chain, robot="kuka", m=M64, shift=(0.0, 0.0, 0.0), f32=False):
    """the table.  m: the margin; shift: added to p1 before placement (the ambiguity test); f32: the f32 engine's table (poses rounded to
    f32; with m = M32)"""
    A = arms(O, chain, robot, f32)
    shift = np.array(shift, dtype=np.float64)
    cells = []

    def add(task, variant, arm, name, side, want, goal=None, step=20, expect=None, twostep=False):
        a = A[(task, variant)][arm]
        i = len(cells)
        expect = dict(expect or {})
        g32 = None
        if task == "reach":
            expect["goal64"] = np.array(goal, dtype=np.float64)
            g32 = np.array(goal, dtype=np.float32)
        # a running return and an episode counter of its own for every cell, so that a stale one shows (both exact in f32)
        cells.append(Cell(name=name + "/" + side, task=task, variant=variant, arm=arm, q=a["q"], action=a["action"], step=int(step), goal=g32,
                          aux=a["aux"], episode=2 + i % 5, ep_return=-(1.0 + 0.125 * (i % 64)), branch=name, side=side, want=want, expect=expect,
                          twostep=twostep, zero_action=not a["action"].any()))

    FAR_OFF = np.array([-0.12, 0.10, -0.08])      # a goal 0.176 m from where the arm ends: well outside reach_dis
    rd, ms = CONST["reach_dis"], CONST["max_steps"]
    if ("reach", "default") in A:
        P = {nm: a["p1"] + shift for nm, a in A[("reach", "default")].items()}
        # ---------------- reach_dis: a margin either side, approached along +x, -z and a diagonal, from a resting and a moving arm
        for arm in ("still", "move"):
            for dn, u in (("x", (1.0, 0.0, 0.0)), ("z", (0.0, 0.0, -1.0)), ("diag", _unit((1.0, -2.0, 2.0)))):
                for side, d in (("in", rd - m), ("out", rd + m)):
                    add("reach", "default", arm, "reach_dis_%s_%s" % (dn, arm), side, dict(near=side == "in", timeout=False), P[arm] + d * np.array(u),
                        expect=dict(done=side == "in", success=side == "in", **(dict(reward=0.0) if side == "in" else {})))
        # distance 0: the goal on the flange itself, as near as f32 has it
        for variant, arm in (("default", "still2"), ("never", "still2")):
            p = A[("reach", variant)][arm]["p1"] + shift
            g = p.astype(np.float32)
            hit = bool((g.astype(np.float64) == p).all())
            add("reach", variant, arm, "reach_dis", "zero", dict(near=variant == "default", timeout=False), g.astype(np.float64),
                expect=dict(done=variant == "default", success=variant == "default", nearest=not hit))
        # ---------------- max_steps: the counter before the step; done when the incremented counter exceeds max_steps.  s0 is run a
        # second step without auto-reset: a finished env stepped again is done again, counted again, last_len follows
        for arm in ("still", "down"):
            for sn, s in (("s-1", ms - 1), ("s0", ms), ("s+1", ms + 1)):
                add("reach", "default", arm, "timeout_" + arm, sn, dict(timeout=s >= ms, near=False), P[arm] + FAR_OFF, step=s,
                    expect=dict(done=s >= ms, success=False), twostep=sn == "s0")
        # ---------------- precedence: the time-out step ending inside reach_dis is no success; the last in-time step is
        for arm in ("still", "move"):
            u = _unit((2.0, 1.0, -2.0))
            add("reach", "default", arm, "precedence_" + arm, "timeout", dict(timeout=True, near=True), P[arm] + (rd - m) * u, step=ms,
                expect=dict(done=True, success=False, reward=-10.0 * (rd - m)))
            add("reach", "default", arm, "precedence_" + arm, "intime", dict(timeout=False, near=True), P[arm] + (rd - m) * u, step=ms - 1,
                expect=dict(done=True, success=True, reward=0.0))
        # ---------------- reward of a step that ends nothing: -10 d (its f64 value through diag, its f32 store through the reward)
        for arm in ("still", "move", "down"):
            for sn, d in (("d5cm", 0.05), ("d40cm", 0.4)):
                add("reach", "default", arm, "reward_" + arm, sn, dict(timeout=False, near=False), P[arm] + d * _unit((-2.0, 1.0, 2.0)),
                    expect=dict(done=False, success=False, reward=-10.0 * d))
        # ---------------- the end of an episode (under auto_reset: the in-place reset; without: the env stays where it ended)
        add("reach", "default", "move", "episode_end", "success", dict(timeout=False, near=True), P["move"] + 0.004 * _unit((1.0, 1.0, 1.0)), step=137,
            expect=dict(done=True, success=True, reward=0.0, last_len=138))
        add("reach", "default", "down", "episode_end", "timeout", dict(timeout=True, near=False), P["down"] + FAR_OFF, step=ms,
            expect=dict(done=True, success=False, last_len=ms + 1))
    # ---------------- variants of the two constants
    if ("reach", "short") in A:      # max_steps = 3; also the two-step cells: the step that ends an episode, then the next one's first
        P = {nm: a["p1"] + shift for nm, a in A[("reach", "short")].items()}
        for arm in ("still", "move"):
            add("reach", "short", arm, "short_timeout_" + arm, "s2", dict(timeout=False, near=False), P[arm] + FAR_OFF, step=2, expect=dict(done=False))
            add("reach", "short", arm, "short_timeout_" + arm, "s3", dict(timeout=True, near=False), P[arm] + FAR_OFF, step=3,
                expect=dict(done=True, success=False), twostep=True)
            add("reach", "short", arm, "short_success_" + arm, "in", dict(timeout=False, near=True), P[arm] + (rd - m) * _unit((-1.0, 2.0, 2.0)), step=1,
                expect=dict(done=True, success=True, reward=0.0), twostep=True)
            add("reach", "short", arm, "short_success_" + arm, "out", dict(timeout=False, near=False), P[arm] + (rd + m) * _unit((-1.0, 2.0, 2.0)), step=1,
                expect=dict(done=False), twostep=True)
    if ("reach", "zero") in A:       # max_steps = 0: every first step is a time-out, whatever the distance
        P = {nm: a["p1"] + shift for nm, a in A[("reach", "zero")].items()}
        add("reach", "zero", "still", "zero", "far", dict(timeout=True, near=False), P["still"] + FAR_OFF, step=0, expect=dict(done=True, success=False), twostep=True)
        add("reach", "zero", "move", "zero", "near", dict(timeout=True, near=True), P["move"] + (rd - m) * _unit((1.0, 0.0, 1.0)), step=0,
            expect=dict(done=True, success=False, reward=-10.0 * (rd - m)), twostep=True)
    if ("reach", "never") in A:      # reach_dis = 0: dist < 0 is never true
        P = {nm: a["p1"] + shift for nm, a in A[("reach", "never")].items()}
        add("reach", "never", "still", "never", "m", dict(timeout=False, near=False), P["still"] + m * _unit((1.0, 1.0, -1.0)), expect=dict(done=False, reward=-10.0 * m))
        add("reach", "never", "move", "never", "far", dict(timeout=False, near=False), P["move"] + FAR_OFF, expect=dict(done=False))
        add("reach", "never", "down", "never", "timeout", dict(timeout=True, near=False), P["down"] + m * _unit((0.0, 1.0, 0.0)), step=ms,
            expect=dict(done=True, success=False))
    if ("reach", "wide") in A:       # reach_dis = 10: every in-time step succeeds; the time-out still wins
        P = {nm: a["p1"] + shift for nm, a in A[("reach", "wide")].items()}
        add("reach", "wide", "still", "wide", "far", dict(timeout=False, near=True), P["still"] + FAR_OFF, expect=dict(done=True, success=True, reward=0.0))
        add("reach", "wide", "move", "wide", "s-1", dict(timeout=False, near=True), P["move"] + FAR_OFF, step=ms - 1, expect=dict(done=True, success=True, reward=0.0))
        add("reach", "wide", "down", "wide", "s0", dict(timeout=True, near=True), P["down"] + FAR_OFF, step=ms,
            expect=dict(done=True, success=False, reward=-10.0 * float(np.linalg.norm(FAR_OFF))))
    # ---------------- the clip (KUKA): per face of the small box a pair, two faces at once, a target on a face; the default boxes
    for task in VARIANTS:
        none = {"%s%d" % (s, k): False for k in range(3) for s in ("lo", "hi")}
        for variant in ("smallbox", "default"):
            d = A.get((task, variant), {})
            box = (SMALLBOX["box_lo"], SMALLBOX["box_hi"]) if variant == "smallbox" else (CONST["box_lo"], CONST["box_hi"][task])
            for arm in d:
                if not (arm.startswith("sb_") or arm.startswith("dflt_")):
                    continue
                goal = d[arm]["p1"] + shift + FAR_OFF if task == "reach" else None
                parts = arm.split("_")
                if arm == "sb_two":
                    add(task, variant, arm, "clip_two", "x_hi+y_lo", dict(none, hi0=True, lo1=True), goal, expect=dict(faces=((0, box[1][0]), (1, box[0][1]))))
                elif arm == "sb_on":
                    add(task, variant, arm, "clip_face", "on", {}, goal, expect=dict(on=(2, box[0][2])))
                else:
                    k, side, tw = AXES.index(parts[1]), parts[2], parts[3]
                    key = "%s%d" % (side, k)
                    name = ("clip_" if variant == "smallbox" else "clip_default_") + parts[1] + "_" + side
                    add(task, variant, arm, name, tw, dict(none, **{key: tw == "out"}), goal,
                        expect=dict(faces=((k, box[0 if side == "lo" else 1][k]),)) if tw == "out" else dict(unclipped=True))
    return cells


def groups(cells):
    """(task, variant) -> cells, in table order"""
    g = {}
    for x in cells:
        g.setdefault((x.task, x.variant), []).append(x)
    return g


def rows_of(cells, idx):
    task = cells[0].task
    r = dict(q=np.array([cells[i].q for i in idx], dtype=np.float64), step=np.array([cells[i].step for i in idx], dtype=np.int32),
             action=np.array([cells[i].action for i in idx], dtype=np.float32), episode=np.array([cells[i].episode for i in idx], dtype=np.uint32),
             ep_return=np.array([cells[i].ep_return for i in idx], dtype=np.float64))
    if task == "reach":
        r["goal"] = np.array([cells[i].goal for i in idx], dtype=np.float32)
    else:
        r["aux"] = np.array([cells[i].aux for i in idx], dtype=np.float64)
    return r


def run_oracle(O, chain, task, cfg, rows, auto_reset=False, seed=0, nsteps=1):
    """the rows through the oracle's own step; a dict of arrays with compare()'s fields where the oracle has them"""
    n = len(rows["q"])
    st = {"reach": O.ReachState, "push": O.PushState, "pick": O.PickState}[task](n)
    st.q[:] = rows["q"]; st.step[:] = rows["step"]; st.episode[:] = rows["episode"]; st.ep_return[:] = rows["ep_return"]
    if task == "reach":
        st.goal[:] = rows["goal"]
    else:
        st.aux[:] = rows["aux"]
    ended = np.zeros(n, dtype=bool); n_done = np.zeros(n, dtype=np.int64); n_succ = np.zeros(n, dtype=np.int64)
    for _ in range(nsteps):
        if auto_reset:
            fn = {"reach": O.reach_step_autoreset, "push": O.push_step_autoreset, "pick": O.pick_step_autoreset}[task]
            obs, rew, done, succ, term = fn(chain, cfg, st, rows["action"], seed=seed)
        else:
            fn = {"reach": O.reach_step, "push": O.push_step, "pick": O.pick_step}[task]
            obs, rew, done, succ, _ = fn(chain, cfg, st, rows["action"])
            term = obs
            d = done.astype(bool)      # the engine's accounting of a finished episode, which the oracle keeps only under auto-reset
            st.last_return[d] = st.ep_return[d]; st.last_len[d] = st.step[d]; st.last_success[d] = succ[d]
        ended |= done.astype(bool); n_done += done; n_succ += succ
    out = dict(q=st.q.copy(), step=st.step.copy(), episode=st.episode.copy(), ep_return=st.ep_return.copy(), obs=obs.copy(), term=term.copy(),
               reward=rew.copy(), done=done.astype(bool), success=succ.astype(bool), last_return=st.last_return.copy(), last_len=st.last_len.copy(),
               last_success=st.last_success.astype(bool), ended=ended, n_done=n_done, n_success=n_succ)
    if task == "reach":
        out["goal"] = st.goal.copy()
    else:
        out["aux"] = st.aux.copy()
    return out
