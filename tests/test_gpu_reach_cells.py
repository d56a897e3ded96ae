"""The cell table of tests/reach_cells.py through the HIP kernels: every cell -- one env step (a few: two) placed a known margin to one
side of one decision of the Cartesian clip or of the reach step's tail (time-out, success distance, their precedence, the reward
select, the accounting of a finished episode, the in-place reset) -- against the float64 model of reach_cells.model_step, cell by cell
and with no cell excluded.

Layouts (tests/test_gpu_cube_cells._layouts): `mixed` interleaves the cells so that every wavefront holds lanes of different branches
(and is run again in reverse order: a cell's outputs are the same bits wherever it sits), `uniform` fills whole 64-lane wavefronts with
one cell each plus a ragged tail of 5.

Grid: one base configuration (f64 engine, KUKA fast FK path, default build, step kernel) over all cells, variants and layouts, with and
without auto-reset; every other factor is varied one at a time from it -- rollout(1), rollout(2) against two step launches, the five
rollout schedules of tests/test_gpu_noise_ref.py, fence_counters 1 and 2 (with 2: diag against the model's f64 flange and reward),
the generic FK path, the Diana chain (outcome families), the fused policies on the zero-action cells (all-zero nets, noise_sigma = 0:
the copies of the step tail that carry no frame) -- plus the f32 engine x {step, lockstep rollout, count33}.  Every path agrees with
the model; all paths of one engine precision, chain and FK path agree with each other bit for bit.

Tolerances (the project's stated per-step agreement, as tests/test_gpu_cube_cells.py applies it): q, obs and terminal obs 1e-6 (f64
engine) / 1e-4 (f32 engine); reward ten times that plus one f32 ulp of the reward; the running and the last return the same bound added
over the steps they sum; done, success, step, episode, last_len, last_success, the counters' increase and every goal (bits) equal;
reward 0.0 on success, and the observation row, q and (cos q, sin q) after an in-place reset against a fresh reset()'s, equal because
exact by construction.

ARMENV_REACH_CELLS_LOG=<path>: the largest measured deviation per task, precision and quantity is written there (a record:
profiles/reach_cells_errors.txt is one such run; no assertion reads it)."""
import os

import numpy as np
import pytest
import torch

import reach_cells as RC
from test_gpu_cube_cells import _layouts
from test_gpu_noise_ref import SCHEDULES, _zero_net

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 3
WORST = {}
REACH_VARIANTS = list(RC.VARIANTS["reach"])
CUBE_GROUPS = [(t, v) for t in ("push", "pick") for v in RC.VARIANTS[t]]
POLICIES = ("actor", "actor_f16x3", "datd3", "daddpg", "random")
BITS = ("obs", "reward", "done", "success", "term", "q", "goal", "step", "episode", "ep_return", "trig", "last_return", "last_len", "last_success",
        "ended", "n_done", "n_success")
_REF = {}


@pytest.fixture(scope="module")
def envs():
    from armenv import envs
    return envs


@pytest.fixture(scope="module", autouse=True)
def _error_log():
    yield
    path = os.environ.get("ARMENV_REACH_CELLS_LOG")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("largest |engine - model| per task, engine precision and quantity over every cell, layout and path of tests/test_gpu_reach_cells.py\n")
            for k, v in sorted(WORST.items()):
                fh.write("%-6s f%d %-14s %.3e\n" % (k[0], k[1], k[2], v))


@pytest.fixture(scope="module")
def chains(O, kuka, diana):
    return dict(kuka=kuka, diana=diana)


@pytest.fixture(scope="module")
def tables(O, chains):
    return {(robot, p): RC.groups(RC.build_cells(O, chains[robot], robot, m=RC.M64 if p == 64 else RC.M32, f32=p == 32))
            for robot in chains for p in (64, 32)}


def _np(t):
    return t.detach().cpu().numpy().copy()


def _engine(envs, O, task, variant, n, precision=64, fk_path=0, auto_reset=False, robot="kuka", **extra):
    Env = dict(reach=envs.BatchedReachEnv, push=envs.BatchedPushEnv, pick=envs.BatchedPickEnv)[task]
    kw = RC.overrides(O, task, variant, robot); kw.update(extra)
    e = Env(n, device=DEV, seed=SEED, auto_reset=auto_reset, precision=precision, fk_path=fk_path, robot=robot, **kw)
    obs = _np(e.reset())
    s = e.get_state()
    e.fresh = dict(eef=obs[0, :3].copy(), q=_np(s["q"])[0], trig=_np(s["trig"])[0])      # what a reset leaves, the same for every env
    assert (obs[:, :3] == obs[0, :3]).all() and (_np(s["q"]) == e.fresh["q"]).all()
    return e


def _install(e, policy):
    D = e.obs_dim
    a, c = ({k: torch.from_numpy(v) for k, v in _zero_net(d, r).items()} for d, r in ((D, 3), (D + 3, 1)))
    kw = dict(action_bound=0.7, noise_sigma=0.0, noise_clip=0.7)
    if policy == "random":
        e.set_policy("random", **kw)
    elif policy in ("actor", "actor_f16x3"):
        e.set_policy(policy, actor_state_dict=a, **kw)
    elif policy == "datd3":
        e.set_policy_datd3(a, a, c, c, **kw)
    else:
        e.set_policy_daddpg(a, a, c, **kw)


def _run(e, task, rows, path, steps=1, fused=False, diag=False):
    """set the rows, run `steps` env steps by the step kernel or one rollout launch (fused: the installed policy acts); the last step's
    outputs, the state after it, the statistics of the episodes that ended and what the counters gained"""
    n = len(rows["q"])
    e.set_state(q=rows["q"], goal=rows.get("goal"), aux=rows.get("aux"), step=rows["step"], ep_return=rows["ep_return"], episode=rows["episode"].view(np.int32))
    c0 = e.counters()
    a = None if fused else torch.from_numpy(rows["action"]).to(DEV)
    out = {}
    if path == "step":
        dn, sc = [], []
        for _ in range(steps):
            obs, rew, done, succ = e.step(a, want_terminal_obs=True, want_diag=diag)
            dn.append(_np(done)); sc.append(_np(succ))
        out.update(obs=_np(obs), reward=_np(rew), term=_np(e.terminal_obs))
        if diag:
            out["diag"] = _np(e.diag)
    else:
        o = e.rollout(steps, None if fused else a[None].repeat(steps, 1, 1).contiguous(), want_terminal_obs=True, want_actions=fused, want_diag=diag)
        dn, sc = list(_np(o["done"])), list(_np(o["success"]))
        out.update(obs=_np(o["obs"][-1]), reward=_np(o["reward"][-1]), term=_np(o["terminal_obs"][-1]))
        if diag:
            out["diag"] = _np(o["diag"][-1])
        if fused:
            out["actions"] = _np(o["actions"])
    dn, sc = np.array(dn, dtype=bool), np.array(sc, dtype=bool)
    ended = dn.any(0)
    s = e.get_state()
    ret, ln, su = (_np(t) for t in e.episode_stats())
    out.update(done=dn[-1], success=sc[-1], ended=ended, n_done=dn.sum(0), n_success=sc.sum(0), q=_np(s["q"]), step=_np(s["step"]),
               episode=_np(s["episode"]).view(np.uint32), ep_return=_np(s["ep_return"]), trig=_np(s["trig"]),
               last_return=np.where(ended, ret, 0.0), last_len=np.where(ended, ln, 0), last_success=np.where(ended, su, 0).astype(bool))
    out["goal" if task == "reach" else "aux"] = _np(s["goal" if task == "reach" else "aux"])
    c1 = e.counters()
    assert c1["nonfinite"] == c0["nonfinite"] and c1["env_steps"] - c0["env_steps"] == n * steps, (c0, c1)
    assert c1["episodes"] - c0["episodes"] == dn.sum() and c1["successes"] - c0["successes"] == sc.sum(), (c0, c1, dn.sum(), sc.sum())
    assert not (sc & ~dn).any()
    return out


def _same_bits(a, b, perm=None, what="", keys=BITS):
    for k in keys:
        if k not in a:
            continue
        y = b[k] if perm is None else b[k][perm]
        assert np.array_equal(a[k], y), (what, k, np.flatnonzero((a[k] != y).reshape(len(y), -1).any(1))[:8])


def _ref(O, chains, robot, precision, cs, lname, idx, auto_reset, steps):
    """the model's rows of a layout (the row is the env's global id), computed once per session and left unchanged"""
    x0 = cs[0]
    key = (robot, precision, x0.task, x0.variant, lname, len(idx), auto_reset, steps, tuple(x.name for x in cs))
    if key not in _REF:
        cfg, c = RC.make_cfg(O, x0.task, x0.variant, robot), RC.constants(O, x0.task, x0.variant, robot)
        r = RC.stack([RC.model_run(O, chains[robot], cfg, c, cs[i], env_id=row, seed=SEED, auto_reset=auto_reset, nsteps=steps) for row, i in enumerate(idx)])
        r["c"] = c
        _REF[key] = r
    return _REF[key]


def _check(e, cs, idx, rows, g, r, precision, steps, what):
    """engine result g against the model's r, row by row; every row is checked"""
    worst = {}
    bad = RC.compare(g, r, RC.tolerances(precision, steps), worst=worst)
    for k, v in worst.items():
        WORST[("reach", precision, k)] = max(WORST.get(("reach", precision, k), 0.0), v)
    assert not bad, (what, [(cs[idx[i]], name, dev) for i, name, dev in bad[:8]])
    # an env reset in place holds what a fresh reset() leaves: the observation row's flange, q and (cos q, sin q), bit for bit
    fresh = r["done"] & (r["step"] == 0)
    assert fresh.any() == bool(e.cfg.auto_reset and r["done"].any()), what
    for k, col in (("eef", g["obs"][:, :3]), ("q", g["q"]), ("trig", g["trig"])):
        assert (col[fresh] == e.fresh[k]).all(), (what, k)
    if not e.cfg.auto_reset:      # ... and without auto-reset nothing is re-drawn, the env stays where it ended
        assert np.array_equal(g["goal"].view(np.uint32), rows["goal"].view(np.uint32)) and np.array_equal(g["episode"], rows["episode"]), what
        assert np.array_equal(g["obs"], g["term"]), what
    if "diag" in g:
        d = g["diag"]
        assert np.array_equal(d[:, :3].astype(np.float32), g["term"][:, :3]) and np.array_equal(d[:, 3].astype(np.float32), g["reward"]), what
        tol = RC.tolerances(precision, steps)
        for k, dev, t in (("diag_eef", np.abs(d[:, :3] - r["eef"]).max(1), tol["pos"]), ("diag_reward", np.abs(d[:, 3] - r["reward"]), tol["reward"])):
            WORST[("reach", precision, k)] = max(WORST.get(("reach", precision, k), 0.0), float(dev.max()))
            assert (dev <= t).all(), (what, k, [(cs[idx[i]], float(dev[i])) for i in np.flatnonzero(dev > t)[:8]])
        if steps == 1:      # success <=> the f64 flange the step itself used lies within reach_dis of the goal, on every cell
            dist = np.sqrt(((d[:, :3] - rows["goal"].astype(np.float64)) ** 2).sum(1))
            over = rows["step"] + 1 > r["c"]["max_steps"]
            assert np.array_equal(g["success"], ~over & (dist < r["c"]["reach_dis"])), what
            assert np.array_equal(g["done"], over | (dist < r["c"]["reach_dis"])), what


def _sweep(envs, O, chains, tables, variant, precision, paths, robot="kuka", fk_path=0, layouts=("mixed", "uniform"), extra=None, diag=False, keep=None):
    """the reach cells of a variant through `paths` (names of 'step', 'rollout') on one handle per (auto_reset, layout): each against the
    model, all of them the same bits; two-step cells also over two steps.  keep (dict): receives the first path's results per
    (auto_reset, layout, steps)"""
    cs = tables[(robot, precision)][("reach", variant)]
    lay = _layouts(len(cs))
    for auto_reset in (False, True):
        for lname in layouts:
            if lname == "reversed" and auto_reset:      # the re-drawn goals depend on the env's index: no permutation invariance to test
                continue
            idx = lay[lname]
            rows = RC.rows_of(cs, idx)
            two = np.array([cs[i].twostep for i in idx])
            e = _engine(envs, O, "reach", variant, len(idx), precision, fk_path, auto_reset, robot, **(extra or {}))
            for steps in (1, 2) if two.any() else (1,):
                r = _ref(O, chains, robot, precision, cs, lname, idx, auto_reset, steps)
                first = None
                for path in paths:
                    what = "%s/%s f%d fk%d %s %s x%d auto_reset=%d %s" % (robot, variant, precision, fk_path, lname, path, steps, auto_reset, extra or "")
                    g = _run(e, "reach", rows, path, steps, diag=diag)
                    _check(e, cs, idx, rows, g, r, precision, steps, what)
                    if first is None:
                        first = g
                    else:
                        _same_bits(first, g, what=what)
                if keep is not None:
                    keep[(auto_reset, lname, steps)] = first
            e.close()


# ------------------------------------------------------------------ the base configuration: every cell, variant and layout

@pytest.mark.parametrize("variant", REACH_VARIANTS)
def test_base_step_kernel_vs_model(envs, O, chains, tables, variant):
    """f64 engine, KUKA fast FK path, default build, step kernel: every cell in every layout, with and without auto-reset"""
    keep = {}
    _sweep(envs, O, chains, tables, variant, 64, ("step",), layouts=("mixed", "reversed", "uniform"), keep=keep)
    n = len(keep[(False, "mixed", 1)]["done"])
    _same_bits(keep[(False, "mixed", 1)], keep[(False, "reversed", 1)], perm=np.arange(n)[::-1], what="reversed")      # a cell's bits do not depend on its lane


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("task,variant", CUBE_GROUPS, ids=["%s-%s" % g for g in CUBE_GROUPS])
def test_cube_tasks_clip_vs_model(envs, O, chains, tables, task, variant, precision):
    """the clip cells of push and pick (the cube parked out of the tool's way): q and the observed flange against the model, the step
    kernel and rollout(1) the same bits, both FK paths"""
    cs = tables[("kuka", precision)][(task, variant)]
    cfg, c = RC.make_cfg(O, task, variant), RC.constants(O, task, variant)
    model = [RC.model_step(O, chains["kuka"], cfg, c, task, dict(q=x.q, step=x.step), x.action) for x in cs]
    tol = RC.PERTURB[precision]
    rnd = (lambda v: v) if precision == 64 else (lambda v: v.astype(np.float32).astype(np.float64))      # the f32 engine holds its state in f32
    for lname, idx in _layouts(len(cs)).items():
        if lname == "reversed":
            continue
        rows = RC.rows_of(cs, idx)
        q = np.array([model[i]["q"] for i in idx]); eef = np.array([model[i]["eef"] for i in idx])
        for fk_path in (0, 1):
            e = _engine(envs, O, task, variant, len(idx), precision, fk_path, False)
            got = {}
            for path in ("step", "rollout"):
                what = "%s/%s f%d %s fk%d %s" % (task, variant, precision, lname, fk_path, path)
                g = got[path] = _run(e, task, rows, path)
                for k, dev in (("q", np.abs(g["q"] - q).max(1)), ("obs", np.abs(g["obs"][:, :3].astype(np.float64) - eef).max(1))):
                    WORST[(task, precision, k)] = max(WORST.get((task, precision, k), 0.0), float(dev.max()))
                    assert (dev <= tol).all(), (what, k, [(cs[idx[i]], float(dev[i])) for i in np.flatnonzero(dev > tol)[:8]])
                assert not g["done"].any() and np.array_equal(g["step"], rows["step"] + 1), what
                assert np.array_equal(g["aux"][:, 0:2], rnd(rows["aux"][:, 0:2])), what      # the parked cube is not touched
            _same_bits(got["step"], got["rollout"], what=what, keys=BITS + ("aux",))
            e.close()


# ------------------------------------------------------------------ one factor at a time

@pytest.mark.parametrize("variant", REACH_VARIANTS)
def test_rollout_launches_agree_with_the_step_kernel(envs, O, chains, tables, variant):
    """rollout(1) and, for the two-step cells, rollout(2) against two step launches: the model's values, the step kernel's bits"""
    _sweep(envs, O, chains, tables, variant, 64, ("step", "rollout"))


@pytest.mark.parametrize("schedule", [s[0] for s in SCHEDULES])
def test_rollout_schedules(envs, O, chains, tables, schedule):
    """the lockstep kernel, the lane-asynchronous kernel under both transition rules, two waves per SIMD and half-filled waves: every
    variant through the step kernel and rollout(1) / rollout(2) on a handle of that schedule"""
    for variant in REACH_VARIANTS:
        _sweep(envs, O, chains, tables, variant, 64, ("step", "rollout"), extra=dict(SCHEDULES)[schedule])


@pytest.mark.parametrize("fence", [1, 2])
def test_fence_counter_builds(envs, O, chains, tables, fence):
    """the two bookkeeping builds of the kernels: the model's values and the default build's bits; with 2, diag = the model's f64
    flange and reward, and success <=> |diag[:3] - goal| < reach_dis on every cell"""
    for variant in REACH_VARIANTS:
        base, keep = {}, {}
        _sweep(envs, O, chains, tables, variant, 64, ("step",), layouts=("mixed",), keep=base)
        _sweep(envs, O, chains, tables, variant, 64, ("step", "rollout"), layouts=("mixed",), extra=dict(fence_counters=fence), diag=fence == 2, keep=keep)
        for k in base:
            _same_bits(base[k], keep[k], what="fence_counters=%d %s %s" % (fence, variant, k))


@pytest.mark.parametrize("path", ["step", "lockstep", "count33"])
def test_f32_engine(envs, O, chains, tables, path):
    """the f32 engine's outcome block and clip: the table rebuilt with q rounded to f32 and the 1e-3 margin"""
    for variant in REACH_VARIANTS:
        if path == "step":
            _sweep(envs, O, chains, tables, variant, 32, ("step",), layouts=("mixed", "reversed", "uniform"))
        else:
            _sweep(envs, O, chains, tables, variant, 32, ("step", "rollout"), extra=dict(SCHEDULES)[path])


def test_generic_fk_path(envs, O, chains, tables):
    for variant in REACH_VARIANTS:
        _sweep(envs, O, chains, tables, variant, 64, ("step", "rollout"), fk_path=1)


def test_diana_chain(envs, O, chains, tables):
    """the second chain (its own FK tables): the outcome families, the table rebuilt for it by the probe"""
    for variant in RC.OUTCOME_VARIANTS:
        _sweep(envs, O, chains, tables, variant, 64, ("step", "rollout"), robot="diana")


@pytest.mark.parametrize("policy", POLICIES)
def test_fused_policies_on_the_zero_action_cells(envs, O, chains, tables, policy):
    """the copies of the step tail behind a fused policy (the fused actors carry no frame between steps): all-zero nets and
    noise_sigma = 0 give mu = 0 and the action +0 exactly, so the zero-action cells must come out as the step kernel gives them for an
    external zero action -- bit for bit -- and as the model has them"""
    n_cells = 0
    for variant in RC.OUTCOME_VARIANTS:
        cs = [x for x in tables[("kuka", 64)][("reach", variant)] if x.zero_action]
        n_cells += len(cs)
        for lname, idx in _layouts(len(cs)).items():
            if lname == "reversed":
                continue
            idx = idx[:len(idx) // 64 * 64]      # the fused policies take full wavefronts only: no ragged tail
            assert set(idx) == set(range(len(cs)))
            rows = RC.rows_of(cs, idx)
            assert not rows["action"].any()
            two = np.array([cs[i].twostep for i in idx])
            for auto_reset in (False, True):
                ext = _engine(envs, O, "reach", variant, len(idx), 64, 0, auto_reset)
                e = _engine(envs, O, "reach", variant, len(idx), 64, 0, auto_reset)
                _install(e, policy)
                for steps in (1, 2) if two.any() else (1,):
                    what = "%s %s %s x%d auto_reset=%d" % (policy, variant, lname, steps, auto_reset)
                    r = _ref(O, chains, "kuka", 64, cs, lname, idx, auto_reset, steps)
                    a = _run(ext, "reach", rows, "step", steps)
                    for path in ("rollout", "step"):
                        g = _run(e, "reach", rows, path, steps, fused=True)
                        _check(e, cs, idx, rows, g, r, 64, steps, what + " " + path)
                        _same_bits(a, g, what=what + " " + path)
                        if path == "rollout":
                            assert g["actions"].shape == (steps, len(idx), 3)
                            assert not g["actions"].any() and not np.signbit(g["actions"]).any(), what      # +0, not -0
                ext.close(); e.close()
    assert n_cells >= 15, n_cells
