"""The cell table of tests/cube_cells.py through the HIP kernels: every cell of the push and pick tasks -- one env step placed a known
margin to one side of one decision of contact(), contact_dyn(), cube_fall(), grip_step() or the outcome block -- against the CPU
oracle, cell by cell and with no cell excluded.

Layouts: `mixed` interleaves the cells so that every wavefront holds lanes of different branches (and is run again in reverse order:
a cell's outputs are the same bits wherever it sits), `uniform` fills whole 64-lane wavefronts with one cell each (plus a ragged tail of
5).  Paths: the step kernel, rollout(1), rollout(2) against two step launches, pick's three rollout schedules, both FK paths, with and
without in-kernel auto-reset.  Step and rollout agree bit for bit; each agrees with the oracle.

Tolerances, f64 engine (the project's stated per-step agreement, tests/test_gpu_parity.py): q, cube, target, d_last, hold offset and
obs 1e-6; cube velocity 1e-6 x push_contact_erp / push_dt (how a position error enters it); shaped reward 2e-4 (-100 x a difference of
two distances); time-out reward 50 x (1e-6 + one f32 ulp of the distance); done, success, gripper state, step counter and the fixed
rewards (+100, -1) equal; what is exact by construction (velocity 0 after a Coulomb stop, an untouched cube's xy, a held cube's
offset) equal.  f32 engine: the cells that leave a 1e-3 margin, rebuilt with it, and 1e-4 (the stated f32 step tolerance) in place of
1e-6 throughout.

ARMENV_CUBE_CELLS_LOG=<path>: the largest measured deviation per task, precision and quantity is written there (a record:
profiles/cube_cells_errors.txt is one such run; no assertion reads it)."""
import os

import numpy as np
import pytest
import torch

import cube_cells as CC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 3
WORST = {}
GROUPS = [(task, variant) for task in ("push", "pick") for variant in CC.VARIANTS[task]]
SCHEDULES = (("lockstep", dict(rollout_ready_lanes=0)), ("count", dict(rollout_straggler_trips=0)), ("straggler", {}))


@pytest.fixture(scope="module")
def envs():
    from armenv import envs
    return envs


@pytest.fixture(scope="module", autouse=True)
def _error_log():
    yield
    path = os.environ.get("ARMENV_CUBE_CELLS_LOG")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("largest |engine - oracle| per task, engine precision and quantity over every cell, layout and path of tests/test_gpu_cube_cells.py\n")
            for k, v in sorted(WORST.items()):
                fh.write("%-6s f%d %-12s %.3e\n" % (k[0], k[1], k[2], v))


@pytest.fixture(scope="module")
def tables(O, kuka):
    return {64: CC.groups(CC.build_cells(O, kuka, m=CC.M64)), 32: CC.groups(CC.build_cells(O, kuka, m=CC.M32, f32_only=True))}


def _np(t):
    return t.detach().cpu().numpy().copy()


def _layouts(n_cells):
    """name -> row -> cell index"""
    rng = np.random.default_rng(1)
    mixed = np.concatenate([rng.permutation(n_cells) for _ in range(max(1, -(-133 // n_cells)))])
    uniform = np.concatenate([np.repeat(np.arange(n_cells), 64), np.arange(5) % n_cells])
    return dict(mixed=mixed, reversed=mixed[::-1].copy(), uniform=uniform)


def _engine(envs, task, variant, n, precision, fk_path, auto_reset, **extra):
    Env = envs.BatchedPushEnv if task == "push" else envs.BatchedPickEnv
    kw = dict(CC.VARIANTS[task][variant]); kw.update(extra)
    e = Env(n, device=DEV, seed=SEED, auto_reset=auto_reset, precision=precision, fk_path=fk_path, **kw)
    e.reset()
    return e


def _run(e, rows, path, steps=1):
    """set the rows, run `steps` env steps by the step kernel or one rollout launch; outputs of the last step and the state after it"""
    q, aux, step, act = rows
    n = len(q)
    e.set_state(q=q, aux=aux, step=step, ep_return=np.zeros(n), episode=np.ones(n, dtype=np.int32))      # the episode after reset()
    c0 = e.counters()
    a = torch.from_numpy(act).to(DEV)
    if path == "step":
        for _ in range(steps):
            obs, rew, done, succ = e.step(a, want_terminal_obs=True)
        out = dict(obs=_np(obs), reward=_np(rew), done=_np(done), success=_np(succ), term=_np(e.terminal_obs))
    else:
        o = e.rollout(steps, a[None].repeat(steps, 1, 1).contiguous(), want_terminal_obs=True)
        out = dict(obs=_np(o["obs"][-1]), reward=_np(o["reward"][-1]), done=_np(o["done"][-1]), success=_np(o["success"][-1]),
                   term=_np(o["terminal_obs"][-1]))
    s = e.get_state()
    out.update(q=_np(s["q"]), aux=_np(s["aux"]), step=_np(s["step"]), episode=_np(s["episode"]).astype(np.uint32))
    c1 = e.counters()
    assert c1["nonfinite"] == 0 and c1["env_steps"] - c0["env_steps"] == n * steps, (c0, c1)
    return out


def _same_bits(a, b, perm=None, what=""):
    for k in ("obs", "reward", "done", "success", "term", "q", "aux", "step", "episode"):
        y = b[k] if perm is None else b[k][perm]
        assert np.array_equal(a[k], y), (what, k, np.flatnonzero((a[k] != y).reshape(len(y), -1).any(1))[:8])


def _worst(task, precision, what, v):
    k = (task, precision, what)
    WORST[k] = max(WORST.get(k, 0.0), float(v))


def _check(task, variant, cs, idx, rows, g, r, precision, auto_reset, what):
    """engine result g against oracle result r, row by row; every row is checked"""
    consts = CC.constants(task, variant)
    tol = CC.tolerances(precision, consts)
    rnd = (lambda v: v) if precision == 64 else (lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64))
    aux_in = rows[1]
    assert np.array_equal(g["done"], r["done"]), (what, [cs[idx[i]] for i in np.flatnonzero(g["done"] != r["done"])[:8]])
    assert np.array_equal(g["success"], r["success"]), (what, [cs[idx[i]] for i in np.flatnonzero(g["success"] != r["success"])[:8]])
    assert np.array_equal(g["step"], r["step"]), what
    if task == "pick":
        assert np.array_equal(g["aux"][:, 7], r["aux"][:, 7]), (what, [cs[idx[i]] for i in np.flatnonzero(g["aux"][:, 7] != r["aux"][:, 7])[:8]])
    fresh = r["done"] if auto_reset else np.zeros(len(idx), dtype=bool)      # rows that show the next episode's first state
    assert np.array_equal(g["episode"], r["episode"]) and np.array_equal(r["episode"], 1 + fresh.astype(np.uint32)), what

    def close(name, a, b, t, rows_=slice(None)):
        d = np.abs(np.asarray(a, dtype=np.float64) - b)
        d = d.reshape(len(d), -1).max(1)
        _worst(task, precision, name, d[rows_].max(initial=0.0))
        bad = np.flatnonzero(d > t) if isinstance(rows_, slice) else np.flatnonzero((d > t) & rows_)
        assert bad.size == 0, (what, name, t, [(cs[idx[i]], float(d[i])) for i in bad[:8]])

    close("q", g["q"], r["q"], tol["pos"])
    close("cube", g["aux"][:, 0:3], r["aux"][:, 0:3], tol["pos"])
    close("target", g["aux"][:, 3:6], r["aux"][:, 3:6], tol["pos"])
    close("d_last", g["aux"][:, 6], r["aux"][:, 6], tol["pos"])
    if task == "pick":
        close("hold_offset", g["aux"][:, 8:11], r["aux"][:, 8:11], tol["pos"])
    else:
        close("velocity", g["aux"][:, 7:9], r["aux"][:, 7:9], tol["vel"])
    close("obs", g["obs"], r["obs"], tol["pos"])
    close("terminal_obs", g["term"], r["term"], tol["pos"])
    # rewards: the fixed ones exactly, the time-out's and the shaped one within their bounds
    for fixed in (100.0, -1.0):
        assert np.array_equal(g["reward"] == fixed, r["reward"] == fixed), (what, fixed)
    tmo = r["done"] & (r["reward"] != 100.0)
    close("reward_timeout", g["reward"], r["reward"], tol["timeout"], tmo)
    close("reward_shaped", g["reward"], r["reward"], tol["shaped"], ~r["done"])
    # a finished episode under auto-reset: the next one's first state -- re-sampled goals bit for bit, velocity / gripper / offset zeroed,
    # d_last re-derived, the counters reset
    if fresh.any():
        # (the f32 engine computes the falling cube's first height in f32: its z is within the tolerance above, not the same bits)
        cols = np.arange(6) if precision == 64 else np.array([0, 1, 3, 4, 5])
        assert np.array_equal(g["obs"][fresh][:, 3 + cols], r["obs"][fresh][:, 3 + cols]), what
        assert np.array_equal(g["aux"][fresh][:, cols], rnd(r["aux"][fresh][:, cols])), what
        assert not g["aux"][fresh, 7:].any() and not g["step"][fresh].any(), what
        d = g["aux"][fresh, 0:3] - g["aux"][fresh, 3:6]
        assert np.abs(g["aux"][fresh, 6] - np.sqrt((d * d).sum(1))).max() <= (1e-15 if precision == 64 else 1e-7), what
        assert np.array_equal(g["q"][fresh], rnd(r["q"][fresh])), what
    # exact by construction
    for i in np.flatnonzero(~fresh):
        x = cs[idx[i]]
        e = x.expect
        if e.get("vel") == (0.0, 0.0):
            assert not g["aux"][i, 7:9].any(), (what, x, g["aux"][i, 7:9])
        if "untouched" in e:
            assert np.array_equal(g["aux"][i, 0:2], rnd(aux_in[i, 0:2])), (what, x, g["aux"][i, 0:2] - aux_in[i, 0:2])
        if e.get("grip") == 2.0 and "off" in e:
                assert np.array_equal(g["aux"][i, 8:11], rnd(aux_in[i, 8:11])), (what, x)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("task,variant", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_cells_step_and_rollout_vs_oracle(envs, O, kuka, tables, task, variant, precision):
    cs = tables[precision].get((task, variant))
    if cs is None:
        assert precision == 32      # every variant has f64 cells; the f32 set may leave one empty
        return
    cfg = CC.make_cfg(O, task, variant)
    lay = _layouts(len(cs))
    for auto_reset in (False, True):
        if auto_reset and not any(x.expect.get("done") for x in cs):
            continue
        ref, first = {}, {}
        for name, idx in lay.items():
            if name == "reversed" and auto_reset:      # the re-sampled goals depend on the env's index: no permutation invariance to test
                continue
            rows = CC.rows_of(cs, idx)
            ref[name] = CC.run_oracle(O, kuka, task, cfg, *rows, auto_reset=auto_reset, seed=SEED)
            for fk_path in (0, 1):
                e = _engine(envs, task, variant, len(idx), precision, fk_path, auto_reset)
                got = {}
                for path in ("step", "rollout"):
                    what = "%s/%s f%d %s fk%d %s auto_reset=%d" % (task, variant, precision, name, fk_path, path, auto_reset)
                    got[path] = _run(e, rows, path)
                    _check(task, variant, cs, idx, rows, got[path], ref[name], precision, auto_reset, what)
                _same_bits(got["step"], got["rollout"], what=what)
                e.close()
                first.setdefault((name, fk_path), got["step"])
        if not auto_reset:
            for fk_path in (0, 1):      # a cell's outputs do not depend on its lane or on its neighbours' branches
                _same_bits(first[("mixed", fk_path)], first[("reversed", fk_path)], perm=np.arange(len(lay["mixed"]))[::-1], what="reversed fk%d" % fk_path)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("task", ["push", "pick"])
def test_two_step_rollout_equals_two_step_launches(envs, tables, task, precision):
    """rollout(2) against two step launches from the side-hit / carried cells among all the others: the velocity, the held cube and (push)
    the frame carried between the steps, bit for bit; pick under its three rollout schedules"""
    for (t, variant), cs in tables[precision].items():
        if t != task or not any(x.twostep for x in cs):
            continue
        idx = _layouts(len(cs))["mixed"]
        rows = CC.rows_of(cs, idx)
        moved = 0
        for fk_path in (0, 1):
            e = _engine(envs, task, variant, len(idx), precision, fk_path, False)
            a = _run(e, rows, "step", steps=2)
            e.close()
            for name, over in (SCHEDULES if task == "pick" else (("default", {}),)):
                e = _engine(envs, task, variant, len(idx), precision, fk_path, False, **over)
                b = _run(e, rows, "rollout", steps=2)
                e.close()
                _same_bits(a, b, what="%s/%s f%d fk%d %s" % (task, variant, precision, fk_path, name))
            two = np.array([cs[i].twostep for i in idx])
            moved += int((np.abs(a["aux"][two, 0:2] - rows[1][two, 0:2]).max(1) > 1e-5).sum())
        assert moved > 0, (task, variant)


@pytest.mark.parametrize("precision", [64, 32])
def test_pick_rollout_schedules_agree_with_the_step_kernel(envs, tables, precision):
    """rollout(1) of every pick cell under the lockstep, count and straggler schedules: the step kernel's bits"""
    for (task, variant), cs in tables[precision].items():
        if task != "pick":
            continue
        for lname, idx in _layouts(len(cs)).items():
            if lname == "reversed":
                continue
            rows = CC.rows_of(cs, idx)
            e = _engine(envs, task, variant, len(idx), precision, 0, False)
            a = _run(e, rows, "step")
            e.close()
            for name, over in SCHEDULES:
                e = _engine(envs, task, variant, len(idx), precision, 0, False, **over)
                _same_bits(a, _run(e, rows, "rollout"), what="%s/%s f%d %s %s" % (task, variant, precision, lname, name))
                e.close()
