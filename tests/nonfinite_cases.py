"""The seeded case table of the non-finite input tests (tests/test_nonfinite_host.py on the CPU oracle, tests/test_gpu_nonfinite.py
through the HIP kernels): which envs are poisoned, with what, at which step; what that does to the `nonfinite` counter by a closed
form; the bit-comparison helpers; a numpy restatement of armenv_summary.  numpy only: importable without torch or a GPU.

Every launch of the table: N = 133 envs (two full waves and a ragged five), T = 12 steps, max_steps = 4, so an episode has
EPISODE = 5 steps and every env sees two in-place resets inside one launch; reach_dis = push_success_dis = 1e-9, so no episode ends
early and a poisoned env resets on the same step as its never-poisoned twin.  The poisoned envs are ALWAYS poisoned_envs(n) =
{0, 31, 32, 63, 64, n - 1}: first lane, both sides of the half-wave and the wave boundary, the last lane of the ragged tail.  A test may
leave out exactly those envs from a comparison of "clean" envs and no others.

A case poisons either actions (env -> (launch step, kind)) or the state before the launch (env -> (episode step the env stands at,
kind)).  An env poisoned before launch step t diverges from its twin on the launch steps t .. the last step of the episode it is in
(`diverged`); where the poison makes its joint angles non-finite (`q_bad`), each of those (env, step) pairs counts once in `nonfinite`
(the kernels test q before the in-place reset); from the step after, the env is its twin's again, bit for bit."""
import numpy as np

N, T, MAX_STEPS = 133, 12, 4
EPISODE = MAX_STEPS + 1          # done at step counter > max_steps: 5 steps per episode
SEED = 5
TINY = 1e-9                      # reach_dis / push_success_dis: no episode ends before its time-out
TASKS = ("reach", "push", "pick")
OBS_DIM = dict(reach=6, push=9, pick=9)


def poisoned_envs(n=N):
    return (0, 31, 32, 63, 64, n - 1)


POISONED = poisoned_envs()


def f32_bits(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def f64_bits(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


NAN_POS, NAN_NEG = 0x7FC00000, 0xFFC00000
PNAN, NNAN, INF = f32_bits(NAN_POS), f32_bits(NAN_NEG), np.float32(np.inf)
PNAN64, NNAN64 = f64_bits(0x7FF8000000000000), f64_bits(0xFFF8000000000000)

# action poisons: name -> (the action, the finite action that clips the same components | None)
ACTION_KINDS = {
    "nan": ((PNAN, PNAN, PNAN), None),
    "nan_x": ((PNAN, 0.25, -0.125), None),
    "neg_nan_z": ((0.25, -0.125, NNAN), None),
    "inf": ((INF, 0.0, -INF), (1e6, 0.0, -1e6)),
    "inf_all": ((-INF, INF, INF), (-1e6, 1e6, 1e6)),
    "1e30": ((1e30, 0.0, -1e30), (1e6, 0.0, -1e6)),
    "3e38": ((3e38, -3e38, 0.0), (1e6, -1e6, 0.0)),
}


def _q_kind(kind, row):
    row = row.copy()
    if kind == "q_nan":
        row[:] = PNAN64
    elif kind == "q_inf_pair":          # only +inf in one joint and -inf in another: their sum is NaN
        row[0], row[3] = np.inf, -np.inf
    elif kind == "q_inf_one":
        row[2] = np.inf
    elif kind == "q_nan_j4":
        row[3] = PNAN64
    elif kind == "q_neg_nan":
        row[1] = NNAN64
    elif kind == "q7_nan":
        row[6] = PNAN64
    else:
        raise KeyError(kind)
    return row


def _goal_kind(kind, row):
    row = row.copy()
    if kind == "goal_nan":
        row[:] = PNAN
    elif kind == "goal_x_nan":
        row[0] = PNAN
    elif kind == "goal_neg_nan_z":
        row[2] = NNAN
    elif kind == "goal_inf":
        row[2] = INF
    elif kind == "goal_neg_inf":
        row[1] = -INF
    else:
        raise KeyError(kind)
    return row


def _aux_kind(kind, row):
    """cube state of push ([10]) / pick ([12]): cube xyz, target xyz, d_last, ..."""
    row = row.copy()
    if kind == "cube_nan":
        row[0:3] = PNAN64
    elif kind == "cube_x_nan":
        row[0] = NNAN64
    elif kind == "target_inf":
        row[3:6] = np.inf
    elif kind == "target_y_neg_inf":
        row[4] = -np.inf
    elif kind == "d_last_nan":
        row[6] = PNAN64
    elif kind == "target_x_nan":
        row[3] = NNAN64
    else:
        raise KeyError(kind)
    return row


def _per_env(values):
    return dict(zip(POISONED, values))


_ACTION_STEPS = (0, 3, 4, 6, 9, 11)       # first step, mid-episode, an episode's last step, second episode, its last step, third (unfinished)
_STATE_STEPS = (0, 1, 2, 3, 4, 2)         # the episode step each env stands at when its state is poisoned

# name -> case.  ik_exit_mode as in ArmEnvConfig; action: env -> (launch step, kind); state: env -> (episode step, kind) with `field`
# one of q / goal (reach) / aux (push, pick); twin "base": the twin run gives those envs the table's ordinary actions / the reset
# state, "stand_in": the finite action that clips the same components (C3: ALL envs agree, the poisoned ones included);
# q_bad: whether the poison makes the env's joint angles non-finite; hold: the poisoned envs get the zero action while diverged, in
# both runs (the IK target then sits inside the residual and ik_exit_mode 1 runs no update).
CASES = {
    "nan_action": dict(ik_exit_mode=0, tasks=TASKS, q_bad=True, twin="base",
                       action=_per_env(zip(_ACTION_STEPS, ("nan", "nan_x", "neg_nan_z", "nan", "nan_x", "nan")))),
    "nan_action_exit1": dict(ik_exit_mode=1, tasks=TASKS, q_bad=False, twin="base",
                             action=_per_env(zip(_ACTION_STEPS, ("nan", "nan_x", "neg_nan_z", "nan", "nan_x", "nan")))),
    "saturate": dict(ik_exit_mode=0, tasks=TASKS, q_bad=False, twin="stand_in",
                     action=_per_env(zip(_ACTION_STEPS, ("inf", "inf_all", "1e30", "3e38", "inf", "1e30")))),
    "q_state": dict(ik_exit_mode=0, tasks=TASKS, q_bad=True, twin="base", field="q",
                    state=_per_env(zip(_STATE_STEPS, ("q_nan", "q_inf_pair", "q_inf_one", "q_nan_j4", "q7_nan", "q_neg_nan")))),
    # joint 7 only, test-before-update, target inside the residual: no update runs, the flange position does not depend on joint 7,
    # so the observation stays finite while q is not -- what the detector reads is q.  Not push: its workspace box ends below the
    # reset pose, so the zero action's target is clipped away from the flange and an update runs.
    "q7_exit1": dict(ik_exit_mode=1, tasks=("reach", "pick"), q_bad=True, twin="base", field="q", hold=True,
                     state=_per_env(zip(_STATE_STEPS, ("q7_nan",) * 6))),
    "goal": dict(ik_exit_mode=0, tasks=("reach",), q_bad=False, twin="base", field="goal",
                 state=_per_env(zip(_STATE_STEPS, ("goal_nan", "goal_x_nan", "goal_neg_nan_z", "goal_inf", "goal_neg_inf", "goal_nan")))),
    "aux": dict(ik_exit_mode=0, tasks=("push", "pick"), q_bad=False, twin="base", field="aux",
                state=_per_env(zip(_STATE_STEPS, ("d_last_nan", "cube_x_nan", "target_inf", "target_y_neg_inf", "cube_nan", "target_x_nan")))),
}
for _name, _case in CASES.items():
    _case["name"] = _name


def cases_of(task):
    return [c for c in CASES.values() if task in c["tasks"]]


def base_actions(seed=SEED, n=N, steps=T):
    """the ordinary actions every run starts from: uniform in +-0.7, f32 [steps][n][3]"""
    return np.random.default_rng(seed).uniform(-0.7, 0.7, (steps, n, 3)).astype(np.float32)


def first_step(case, env):
    """(episode step the env stands at when the launch starts, launch step before which it is poisoned)"""
    if "action" in case:
        return 0, case["action"][env][0]
    return case["state"][env][0], 0


def diverged(case, env, steps=T):
    """(t0, t1, resets): the env differs from its twin on launch steps t0..t1 inclusive; resets: t1 is its episode's last step (the
    in-place reset happens inside the launch and the env is its twin's again from t1 + 1 on)"""
    s0, t0 = first_step(case, env)
    t1 = t0 + (EPISODE - 1 - (s0 + t0) % EPISODE)
    return t0, min(t1, steps - 1), t1 <= steps - 1


def diverged_mask(case, steps=T, n=N):
    m = np.zeros((steps, n), dtype=bool)
    for env in poisoned_envs(n):
        t0, t1, _ = diverged(case, env, steps)
        m[t0:t1 + 1, env] = True
    return m


def expected_nonfinite(case, steps=T):
    """closed form: an env poisoned before step s of an episode of max_steps + 1 steps counts every step from s to the episode's last"""
    if not case["q_bad"]:
        return 0
    return sum(t1 - t0 + 1 for t0, t1, _ in (diverged(case, env, steps) for env in POISONED))


def actions_for(case, which):
    """f32 [T][N][3]; which: "poisoned" | "twin" """
    a = base_actions()
    if case.get("hold"):
        for env in POISONED:
            t0, t1, _ = diverged(case, env)
            a[t0:t1 + 1, env] = 0.0
    for env, (t, kind) in case.get("action", {}).items():
        bad, stand_in = ACTION_KINDS[kind]
        if which == "poisoned":
            a[t, env] = np.array(bad, dtype=np.float32)
        elif case["twin"] == "stand_in":
            a[t, env] = np.array(stand_in, dtype=np.float32)
    return a


def apply_state(case, which, fields):
    """fields: dict of numpy arrays q f64 [N][7], step i32 [N] and goal f32 [N][3] / aux f64 [N][k] as the reset left them; returns the
    dict of the fields to set before the launch (copies), the same in both runs except for the poison itself"""
    out = {}
    if "state" not in case:
        return out
    step = fields["step"].copy()
    field = case["field"]
    x = fields[field].copy()
    fn = dict(q=_q_kind, goal=_goal_kind, aux=_aux_kind)[field]
    for env, (s0, kind) in case["state"].items():
        step[env] = s0
        if which == "poisoned":
            x[env] = fn(kind, x[env])
    out["step"] = step
    out[field] = x
    return out


# ------------------------------------------------------------------ bit comparison

def bits(a):
    """floats as integers of their width (NaN compares equal to itself, -0 differs from +0); everything else unchanged"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.int32)
    if a.dtype == np.float64:
        return a.view(np.int64)
    return a


def differing_envs(a, b, axis):
    """sorted env indices at which a and b differ in any bit; `axis` is the env axis"""
    x, y = bits(a), bits(b)
    assert x.shape == y.shape and x.dtype == y.dtype, (x.shape, y.shape, x.dtype, y.dtype)
    d = np.moveaxis(x != y, axis, 0)
    return np.flatnonzero(d.reshape(d.shape[0], -1).any(1)).tolist()


def assert_same_bits(a, b, axis, allowed=(), what=""):
    """a and b agree bit for bit at every env outside `allowed` (which must be a subset of the poisoned envs)"""
    n = np.shape(a)[axis]
    assert set(allowed) <= set(poisoned_envs(n)), (what, allowed)
    bad = [e for e in differing_envs(a, b, axis) if e not in allowed]
    assert not bad, (what, bad[:8])


def assert_count(got, want, what=""):
    assert int(got) == int(want), (what, int(got), int(want))


PER_STEP = ("obs", "reward", "done", "success", "terminal_obs", "actions", "ik_updates")      # [T][N]...
STATE = ("q", "goal", "aux", "step", "episode", "ep_return", "trig")                          # [N]...
STATS = ("last_return", "last_len", "last_success", "returns_f32")                           # [N]


# ------------------------------------------------------------------ the CPU oracle on a case

def oracle_config(O, task, case):
    cfg = O.default_config(task)
    cfg.max_steps = MAX_STEPS
    cfg.reach_dis = TINY
    cfg.push_success_dis = TINY
    cfg.ik_exit_mode = case["ik_exit_mode"]
    return cfg


def oracle_run(O, chain, task, case, which="poisoned", steps=T):
    """The case on the CPU oracle, stepped with reach_step / push_step / pick_step (no auto-reset; finished envs are reset by mask, as
    the kernels' in-place reset does).  Per step [steps][N]: q_bad (q not all-finite after the step, before the reset), q_nan [..][7],
    obs_bad (the pre-reset observation), updates, reward, done, success, obs (pre-reset); and the final q."""
    State = dict(reach=O.ReachState, push=O.PushState, pick=O.PickState)[task]
    reset, step = getattr(O, task + "_reset"), getattr(O, task + "_step")
    cfg = oracle_config(O, task, case)
    st = State(N)
    reset(chain, cfg, st, seed=SEED)
    if case.get("field") == "goal":
        goal = apply_state(case, which, dict(step=st.step, goal=st.goal))["goal"]
        O.reach_reset_with_goal(chain, cfg, st, goal)
    new = apply_state(case, which, {k: getattr(st, k) for k in ("q", "step", "goal", "aux") if hasattr(st, k)})
    for k, v in new.items():
        if k != "goal":
            getattr(st, k)[...] = v
    acts = actions_for(case, which)
    out = dict(q_bad=[], q_nan=[], obs_bad=[], updates=[], reward=[], done=[], success=[], obs=[])
    for t in range(steps):
        o, r, d, s, it = step(chain, cfg, st, acts[t])
        out["q_bad"].append(~np.isfinite(st.q).all(1))
        out["q_nan"].append(np.isnan(st.q))
        out["obs_bad"].append(~np.isfinite(o).all(1))
        for k, v in (("updates", it), ("reward", r), ("done", d.astype(bool)), ("success", s.astype(bool)), ("obs", o)):
            out[k].append(np.array(v, copy=True))
        if d.any():
            reset(chain, cfg, st, seed=SEED, mask=d)
    out = {k: np.stack(v) for k, v in out.items()}
    out["q"] = st.q.copy()
    return out


# ------------------------------------------------------------------ armenv_summary, restated

def summary_restated(dist, last_return, last_len, last_success):
    """env_summary_kernel + summary_reduce_kernel in numpy, operation for operation: per wave of 64 envs an xor-butterfly (offsets 32 ..
    1) of sums and of an fmax, lane 0's value kept as the wave's row; then 32 slots each folding rows slot, slot + 32, ... in order,
    and slot 0 .. 31 folded in order.  out[8] = [sum distance, max distance, sum return, sum length, sum success, envs, 0, 0].  Sums
    propagate a NaN, the max column (fmax) ignores it."""
    dist, ret, ln, su = (np.asarray(x, dtype=np.float64) for x in (dist, last_return, last_len, last_success))
    n = dist.size
    n_rows = (n + 63) // 64
    rows = np.zeros((n_rows, 8))
    for w in range(n_rows):
        idx = 64 * w + np.arange(64)
        live = idx < n
        ic = np.where(live, idx, n - 1)
        v = np.stack([np.where(live, x[ic], 0.0) for x in (dist, ret, ln, su)] + [live.astype(np.float64)])
        mx = v[0].copy()
        for o in (32, 16, 8, 4, 2, 1):
            perm = np.arange(64) ^ o
            v = v + v[:, perm]
            mx = np.fmax(mx, mx[perm])
        rows[w] = [v[0, 0], mx[0], v[1, 0], v[2, 0], v[3, 0], v[4, 0], 0.0, 0.0]
    part = np.zeros((32, 8))
    for slot in range(32):
        for col in range(8):
            acc = 0.0
            for r in range(slot, n_rows, 32):
                acc = np.fmax(acc, rows[r, col]) if col == 1 else acc + rows[r, col]
            part[slot, col] = acc
    out = part[0].copy()
    for k in range(1, 32):
        for col in range(8):
            out[col] = np.fmax(out[col], part[k, col]) if col == 1 else out[col] + part[k, col]
    return out


# ------------------------------------------------------------------ fused policies (C8, C9)

POLICY_VALUES = {"nan_pos": PNAN, "nan_neg": NNAN, "inf": INF, "neg_inf": -INF, "above_f16": np.float32(1.0e5)}     # 1e5 > 65504
POLICY_PLACES = ("fc1.weight", "fc2.weight", "fc3.bias", "all")
MLP_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")


def mlp(rng, n_in, n_out, hidden=256):
    """a state dict of the reference's PolicyNet / QValueNet shapes with torch.nn.Linear's default initial range, f32 numpy"""
    def lin(o, i):
        k = 1.0 / np.sqrt(i)
        return rng.uniform(-k, k, (o, i)).astype(np.float32), rng.uniform(-k, k, o).astype(np.float32)
    (w1, b1), (w2, b2), (w3, b3) = lin(hidden, n_in), lin(hidden, hidden), lin(n_out, hidden)
    return dict(zip(MLP_KEYS, (w1, b1, w2, b2, w3, b3)))


def poison_mlp(sd, value, place):
    """a copy of sd with `value` in ONE element (a fixed, non-corner one) of tensor `place`, or of every tensor ("all")"""
    out = {k: v.copy() for k, v in sd.items()}
    for k in (MLP_KEYS if place == "all" else (place,)):
        flat = out[k].reshape(-1)
        flat[(7 * flat.size) // 11] = value
    return out


def poisoned_rows(n):
    """the poisoned rows of a batch of n states: poisoned_envs(n) without repeats and without what lies beyond a one-wave batch"""
    return tuple(sorted({r for r in poisoned_envs(n) if r < n}))


# what a poisoned row / observation holds, in turn over the poisoned rows: (column, value); column None = the whole row
ROW_VALUES = ((None, PNAN), (1, INF), (2, NNAN), (0, np.float32(1e30)), (None, NNAN), (-1, -INF))


def poison_rows(states):
    """a copy of states f32 [n][D] with its poisoned_rows(n) poisoned by ROW_VALUES in turn"""
    out = states.copy()
    for r, (col, v) in zip(poisoned_rows(len(out)), ROW_VALUES):
        if col is None:
            out[r, :] = v
        else:
            out[r, col] = v
    return out
