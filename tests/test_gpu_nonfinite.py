"""Non-finite and huge inputs through every env and policy kernel (the contract C1-C10 of INTEGRATION.md, "Non-finite inputs"), on the
case table of tests/nonfinite_cases.py.  No tolerance anywhere: bit equality (floats compared as integers, so NaN equals itself), exact
counts, finiteness.

External actions (reach, push, pick; f64 and f32 engines; N = 133, T = 12, max_steps = 4): every case is run poisoned under the step
kernel, the lockstep rollout, the lane-asynchronous rollout (straggler rule with ready_lanes 1 and 33, count rule 33), two waves per
SIMD and half-filled waves, and as a never-poisoned twin.  All schedules give the same bits and counters, poisoned envs included (C6);
the clean envs are the twin's (C1); `nonfinite` is the table's closed-form number, which tests/test_nonfinite_host.py derives from the
oracle as well, and the other counters are what the per-step outputs imply (C2); a saturating action is the clipped finite one (C3);
the poisoned envs' update counts, NaN pattern and flags are the oracle's (C4); after its reset -- in place, or reset(mask) -- a
poisoned env is the twin's again (C5); goal and cube-state poison obey the same and are not counted (C7).  Controls: the poisoned
envs do differ from their twins, the counts are non-zero.

Fused policies: no poisoned net or observation hands an env a non-finite action (C8); rows and envs are independent (C9).
Population learners: a diverged member leaves its neighbours' bits alone and exploit heals it (C10)."""
import numpy as np
import pytest
import torch

import nonfinite_cases as NC
import pop_common as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FULL = dict(rollout_waves_per_simd=1, rollout_lanes_per_wave=64)
SCHEDULES = (
    ("step", dict(FULL)),
    ("lockstep", dict(FULL, rollout_ready_lanes=0, rollout_straggler_trips=0)),
    ("async1", dict(FULL, rollout_ready_lanes=1, rollout_straggler_trips=3)),
    ("async33", dict(FULL, rollout_ready_lanes=33, rollout_straggler_trips=3)),
    ("count33", dict(FULL, rollout_ready_lanes=33, rollout_straggler_trips=0)),
    ("two_waves", dict(rollout_ready_lanes=0, rollout_straggler_trips=0, rollout_waves_per_simd=2, rollout_lanes_per_wave=64)),
    ("half_waves", dict(rollout_ready_lanes=0, rollout_straggler_trips=0, rollout_waves_per_simd=1, rollout_lanes_per_wave=32)),
)
TWIN_SCHEDULES = ("step", "async1")
COUNTERS = ("episodes", "successes", "env_steps", "nonfinite", "ik_updates")
AFTER = 3      # steps run after reset(mask)


@pytest.fixture(scope="module")
def envs():
    from armenv import envs
    return envs


@pytest.fixture(scope="module")
def oracle_runs(O, kuka):
    cache = {}

    def get(task, case):
        key = (task, case["name"])
        if key not in cache:
            cache[key] = NC.oracle_run(O, kuka, task, case)
        return cache[key]
    return get


def _np(t):
    return t.detach().cpu().numpy().copy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _env_class(envs, task):
    return dict(reach=envs.BatchedReachEnv, push=envs.BatchedPushEnv, pick=envs.BatchedPickEnv)[task]


def _state(e):
    s = e.get_state()
    out = {k: _np(v) for k, v in s.items()}
    ret, ln, su = e.episode_stats()
    out.update(last_return=_np(ret), last_len=_np(ln), last_success=_np(su), returns_f32=_np(e.episode_returns_f32()))
    return out


def _run(envs, task, precision, case, which, schedule, fence):
    """one handle through one case: the launch (12 steps by the schedule's kernel), then reset(mask = the poisoned envs) and AFTER
    more steps.  Returns numpy arrays: the per-step outputs, the state and statistics after the launch, the counters' increase."""
    name, over = schedule
    e = _env_class(envs, task)(NC.N, device=DEV, seed=NC.SEED, auto_reset=True, precision=precision, max_steps=NC.MAX_STEPS,
                               reach_dis=NC.TINY, push_success_dis=NC.TINY, ik_exit_mode=case["ik_exit_mode"], fence_counters=fence,
                               **over)
    e.reset()
    if case.get("field") == "goal":
        s = e.get_state()
        e.reset(goal=_dev(NC.apply_state(case, which, dict(step=_np(s["step"]), goal=_np(s["goal"])))["goal"]))
    s = e.get_state()
    new = NC.apply_state(case, which, {k: _np(v) for k, v in s.items() if k in ("q", "step", "goal", "aux")})
    new.pop("goal", None)
    if new:
        e.set_state(**{k: _dev(v) for k, v in new.items()})
    c0 = e.counters()
    acts = _dev(NC.actions_for(case, which))
    out = {}
    if name == "step":
        per = {k: [] for k in NC.PER_STEP}
        for t in range(NC.T):
            o, r, d, sc = e.step(acts[t], want_terminal_obs=True, want_ik_updates=bool(fence))
            for k, v in (("obs", o), ("reward", r), ("done", d), ("success", sc), ("terminal_obs", e.terminal_obs), ("actions", acts[t])):
                per[k].append(_np(v))
            if fence:
                per["ik_updates"].append(_np(e.ik_updates))
        out.update({k: np.stack(v) for k, v in per.items() if v})
    else:
        o = e.rollout(NC.T, acts, want_actions=True, want_terminal_obs=True, want_ik_updates=bool(fence))
        out.update({k: _np(o[k]) for k in NC.PER_STEP if k in o})
    out.update(_state(e))
    c1 = e.counters()
    out["counters"] = {k: c1[k] - c0[k] for k in COUNTERS}
    mask = np.zeros(NC.N, dtype=np.uint8)
    mask[list(NC.POISONED)] = 1
    e.reset(mask=_dev(mask))
    o = e.rollout(AFTER, _dev(NC.base_actions()[:AFTER]), want_terminal_obs=True)
    for k in ("obs", "reward", "done", "success", "terminal_obs"):
        out["after_" + k] = _np(o[k])
    for k, v in e.get_state().items():
        out["after_" + k] = _np(v)
    out["after_nonfinite"] = e.counters()["nonfinite"] - c1["nonfinite"]
    e.close()
    return out


def _keys(out, names):
    return [k for k in names if k in out]


def _check_case(envs, oracle_runs, task, precision, case, fence):
    what = "%s f%d %s fence=%d" % (task, precision, case["name"], fence)
    assert set(case.get("action", case.get("state"))) == set(NC.POISONED) == {0, 31, 32, 63, 64, NC.N - 1}
    sched = dict(SCHEDULES)
    P = {name: _run(envs, task, precision, case, "poisoned", (name, sched[name]), fence) for name, _ in SCHEDULES}
    W = {name: _run(envs, task, precision, case, "twin", (name, sched[name]), fence) for name in TWIN_SCHEDULES}
    ref, twin = P["step"], W["step"]
    every = _keys(ref, NC.PER_STEP + NC.STATE + NC.STATS) + [k for k in ref if k.startswith("after_") and k != "after_nonfinite"]
    env_axis = lambda k: 1 if k in NC.PER_STEP or k in ("after_obs", "after_reward", "after_done", "after_success", "after_terminal_obs") else 0

    # C6: every schedule, the same bits and counters, poisoned and clean envs alike; T step launches are one T-step rollout
    for runs in (P, W):
        first = runs["step"]
        for name, r in runs.items():
            for k in every:
                NC.assert_same_bits(first[k], r[k], env_axis(k), what=(what, name, k))
            assert r["counters"] == first["counters"] and r["after_nonfinite"] == 0, (what, name, r["counters"], first["counters"])

    # C2: the counters.  nonfinite: the table's closed form (derived from the oracle too, tests/test_nonfinite_host.py)
    c = ref["counters"]
    print("%s: nonfinite %d (expected %d), counters %s" % (what, c["nonfinite"], NC.expected_nonfinite(case), c))
    NC.assert_count(c["nonfinite"], NC.expected_nonfinite(case), what)
    NC.assert_count(twin["counters"]["nonfinite"], 0, what)
    for r in (ref, twin):
        NC.assert_count(r["counters"]["episodes"], r["done"].sum(), what)
        NC.assert_count(r["counters"]["successes"], (r["done"] & r["success"]).sum(), what)
        NC.assert_count(r["counters"]["env_steps"], NC.N * NC.T, what)
        if fence:
            NC.assert_count(r["counters"]["ik_updates"], r["ik_updates"].astype(np.int64).sum(), what)
    assert c["episodes"] == 2 * NC.N + sum(1 for e in NC.POISONED if NC.first_step(case, e)[0] > 2), what

    div = NC.diverged_mask(case)
    if case["twin"] == "stand_in":
        # C3: the whole run is the finite stand-in's, the poisoned envs included; only the echoed action itself differs
        echo = np.zeros((NC.T, NC.N), dtype=bool)
        for env, (t, _) in case["action"].items():
            echo[t, env] = True
        for k in every:
            if k == "actions":
                x, y = NC.bits(ref[k]), NC.bits(twin[k])
                assert np.array_equal(x[~echo], y[~echo]) and (x[echo] != y[echo]).any(1).all(), what
                assert np.array_equal(x, NC.bits(NC.actions_for(case, "poisoned"))), what      # the poison reached the kernel
            else:
                NC.assert_same_bits(ref[k], twin[k], env_axis(k), what=(what, k))
        assert np.isfinite(ref["q"]).all() and np.isfinite(ref["obs"]).all(), what
    else:
        # C1: the clean envs are the twin's in every per-step output, every state field, every statistic
        for k in every:
            NC.assert_same_bits(ref[k], twin[k], env_axis(k), allowed=NC.POISONED, what=(what, k))
        # control: the poisoned envs do differ (the joint-7 case changes no output, only q: its control is the count above)
        if case["name"] != "q7_exit1":
            changed = set()
            for k in ("obs", "reward", "terminal_obs"):
                changed |= set(NC.differing_envs(ref[k], twin[k], 1))
            assert changed == set(NC.POISONED), (what, sorted(changed))
        else:
            assert NC.expected_nonfinite(case) > 0 and np.isfinite(ref["terminal_obs"]).all(), what
        # C5: outside the steps from the poison to the episode's last, a poisoned env is the twin's again, bit for bit: the in-place
        # reset heals it (the observation of the reset step is already the next episode's)
        resets = np.zeros((NC.T, NC.N), dtype=bool)
        for env in NC.POISONED:
            _, t1, r = NC.diverged(case, env)
            resets[t1, env] = r
        for k in _keys(ref, NC.PER_STEP):
            m = div & ~resets if k == "obs" else div
            x, y = NC.bits(ref[k]), NC.bits(twin[k])
            assert np.array_equal(x[~m], y[~m]), (what, k)
        for env in NC.POISONED:
            t0, t1, r = NC.diverged(case, env)
            if r:       # healed inside the launch: its state is the twin's
                for k in _keys(ref, NC.STATE):
                    assert np.array_equal(NC.bits(ref[k][env]), NC.bits(twin[k][env])), (what, k, env)
                if t1 + NC.EPISODE <= NC.T - 1:      # and a whole episode after it: its statistics too
                    for k in NC.STATS:
                        assert np.array_equal(NC.bits(ref[k][env]), NC.bits(twin[k][env])), (what, k, env)
    # C5, the other reset: after reset(mask) every env is the twin's in every output and field, and the counter stands still
    for k in every:
        if k.startswith("after_"):
            NC.assert_same_bits(ref[k], twin[k], env_axis(k), what=(what, k))
    assert np.isfinite(ref["after_q"]).all() and np.isfinite(ref["after_obs"]).all(), what

    # C4 / C2: the poisoned envs against the oracle on the same inputs -- flags everywhere, NaN pattern of reward and observation,
    # update counts on the NaN-driven steps, which joints are NaN at the end
    orc = oracle_runs(task, case)
    assert np.array_equal(ref["done"], orc["done"]) and np.array_equal(ref["success"], orc["success"]), what
    pe = list(NC.POISONED)
    assert np.array_equal(np.isnan(ref["reward"][:, pe]), np.isnan(orc["reward"][:, pe])), what
    assert np.array_equal(~np.isfinite(ref["terminal_obs"][:, pe]).all(-1), orc["obs_bad"][:, pe]), what
    assert np.isfinite(ref["reward"][~div]).all() and np.isfinite(ref["terminal_obs"][~div]).all(), what
    assert np.array_equal(np.isnan(ref["q"]), np.isnan(orc["q"])), what
    if fence:
        if case["name"] in ("nan_action", "q7_exit1"):
            assert np.array_equal(ref["ik_updates"][div], orc["updates"][div]), (what, ref["ik_updates"][div], orc["updates"][div])
        if case["name"] == "q_state":
            # not pinned to the oracle: with NaN in joint 7 alone the kernels' orientation error (its acos argument is clamped, which
            # drops a NaN) is finite on the first trip and they apply TWO updates where the oracle applies one.  What holds by the loop's
            # form: its first update always runs (ik_exit_mode 0) and it ends by the iteration cap (20) at the latest
            print("%s: updates of the state-poisoned envs %s (oracle %s)" % (what, ref["ik_updates"][div].tolist(), orc["updates"][div].tolist()))
            assert ((ref["ik_updates"][div] >= 1) & (ref["ik_updates"][div] <= 20)).all(), (what, ref["ik_updates"][div])
        if "action" in case:
            at = [(t, env) for env, (t, _) in case["action"].items()]
            got = [int(ref["ik_updates"][t, env]) for t, env in at]
            assert got == [int(orc["updates"][t, env]) for t, env in at], (what, got)


_PARAMS = [(task, c["name"], fence) for task in NC.TASKS for c in NC.cases_of(task)
           for fence in ((1, 0) if c["name"] in ("nan_action", "q_state") else (1,))]


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("task,case,fence", _PARAMS, ids=["%s-%s-fence%d" % p for p in _PARAMS])
def test_external_actions(envs, oracle_runs, task, case, fence, precision):
    """C1-C7 for one case of the table; fence 1: the bookkeeping build (per-step update counts), fence 0: the default kernels"""
    _check_case(envs, oracle_runs, task, precision, NC.CASES[case], fence)


def test_nonzero_counts_are_asserted_for_every_task():
    """the table holds, for each task, cases whose expected `nonfinite` is a non-zero number (test_external_actions asserts it for
    both engines under the step kernel, the lockstep and the asynchronous rollout)"""
    for task in NC.TASKS:
        assert sum(NC.expected_nonfinite(c) > 0 for c in NC.cases_of(task)) >= 2
    assert {s[0] for s in SCHEDULES} >= {"step", "lockstep", "async1", "async33", "two_waves", "half_waves"}


@pytest.mark.parametrize("precision", [64, 32])
def test_summary_sums_nan_and_its_max_skips_it(envs, precision):
    """C7: armenv_summary with one poisoned env (31: NaN goal now, NaN return of its last episode) against the numpy restatement of
    env_summary_kernel / summary_reduce_kernel and against a twin in which env 31 is a copy of env 30: the sums are NaN, the max
    column is the twin's bits, the other columns are the restatement's bits."""
    bad, src = 31, 30
    acts = NC.base_actions()[:NC.EPISODE].copy()
    acts[:, bad] = acts[:, src]
    raw, stats = {}, {}
    for which in ("poisoned", "twin"):
        e = envs.BatchedReachEnv(NC.N, device=DEV, seed=NC.SEED, precision=precision, max_steps=NC.MAX_STEPS, reach_dis=NC.TINY)
        e.reset()
        goal = _np(e.get_state()["goal"])
        goal[bad] = goal[src]
        if which == "poisoned":
            goal[bad, 1] = NC.PNAN
        e.reset(goal=_dev(goal))
        out = e.rollout(NC.EPISODE, _dev(acts))                   # one whole episode: env 31's return is NaN
        assert bool(out["done"][-1].all())
        goal2 = _np(e.get_state()["goal"])
        goal2[bad] = goal2[src]
        if which == "poisoned":
            goal2[bad, 2] = NC.NNAN
        e.set_state(goal=_dev(goal2))
        raw[which] = _np(e.summary()["raw"])
        stats[which] = [_np(x) for x in e.episode_stats()]
        assert e.counters()["nonfinite"] == 0                     # the counter watches joint angles only
        e.close()
    p, t = raw["poisoned"], raw["twin"]
    print("summary f%d poisoned %s twin %s" % (precision, p.tolist(), t.tolist()))
    assert np.isnan(p[0]) and np.isnan(p[2]) and np.isfinite(t).all()
    assert NC.bits(p[1:2]) == NC.bits(t[1:2]) and p[1] > 0                  # fmax skips the NaN env: the max over the others
    assert np.array_equal(NC.bits(p[3:]), NC.bits(t[3:])) and p[5] == NC.N
    for which in ("poisoned", "twin"):
        ret, ln, su = stats[which]
        assert np.isnan(ret[bad]) == (which == "poisoned") and np.isfinite(np.delete(ret, bad)).all()
        want = NC.summary_restated(np.zeros(NC.N), ret, ln, su)             # (the distances are not visible from outside)
        assert np.array_equal(NC.bits(raw[which][2:]), NC.bits(want[2:])), which


# ------------------------------------------------------------------ fused policies

POLICY_KINDS = ("actor", "actor_f16x3", "datd3", "darc", "daddpg")


def _policy_env(envs, D, n, **kw):
    return (envs.BatchedReachEnv if D == 6 else envs.BatchedPushEnv)(n, device=DEV, seed=7, **kw)


def _nets(rng, D):
    return dict(actor1=NC.mlp(rng, D, 3), actor2=NC.mlp(rng, D, 3), critic1=NC.mlp(rng, D + 3, 1), critic2=NC.mlp(rng, D + 3, 1))


def _install(e, kind, nets):
    t = lambda name: {k: torch.from_numpy(v) for k, v in nets[name].items()}
    if kind in ("actor", "actor_f16x3"):
        e.set_policy(kind, actor_state_dict=t("actor1"))
    elif kind == "daddpg":
        e.set_policy_daddpg(t("actor1"), t("actor2"), t("critic1"))
    elif kind == "datd3":
        e.set_policy_datd3(t("actor1"), t("actor2"), t("critic1"), t("critic2"))
    else:
        e.set_policy_darc(t("actor1"), t("actor2"), t("critic1"), t("critic2"))


def _sub_cases(kind):
    """which nets are poisoned: the single actor; the two-actor agents: only actor 1, only one critic, everything"""
    if kind in ("actor", "actor_f16x3"):
        return (("actor1",),)
    every = ("actor1", "actor2", "critic1") + (() if kind == "daddpg" else ("critic2",))
    return (("actor1",), ("critic1",) if kind == "daddpg" else ("critic2",), every)


def _poisoned_goal(e, D, n):
    s = e.get_state()
    if D == 6:
        g = _np(s["goal"])
    else:
        g = _np(s["aux"])[:, :6].astype(np.float32)
    return NC.poison_rows(g)


@pytest.mark.parametrize("n", [192, 320])
@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("kind", POLICY_KINDS)
def test_no_nonfinite_action_reaches_an_env(envs, kind, D, n):
    """C8.  Two handles go through the same installs: one acts by rollout(3), the other by three step(None) launches.  Whatever the net
    holds -- NaN of either sign, +-inf, a finite weight beyond f16, in one element of fc1.weight, fc2.weight, fc3.bias or of every
    tensor -- and with clean nets on a poisoned observation: every action is finite and within +-noise_clip, q stays finite,
    `nonfinite` stays 0, and the two handles agree bit for bit."""
    clip = 0.7
    rng = np.random.default_rng(11)
    nets = _nets(rng, D)
    a, b = _policy_env(envs, D, n), _policy_env(envs, D, n)
    installs = [(name, place, sub) for name in NC.POLICY_VALUES for place in NC.POLICY_PLACES for sub in _sub_cases(kind)]
    worst = 0.0
    for name, place, sub in installs + [("observation", None, ())]:
        what = (kind, D, n, name, place, sub)
        bad = dict(nets)
        for net in sub:
            bad[net] = NC.poison_mlp(nets[net], NC.POLICY_VALUES[name], place)
        for e in (a, b):
            _install(e, kind, bad)
            e.reset()
            if name == "observation":
                e.reset(goal=_dev(_poisoned_goal(e, D, n)))
        out = a.rollout(3, None, want_actions=True)
        acts = _np(out["actions"])
        assert np.isfinite(acts).all() and np.abs(acts).max() <= np.float32(clip), (what, np.argwhere(~np.isfinite(acts))[:4].tolist())
        worst = max(worst, float(np.abs(acts).max()))
        for t in range(3):
            o, r, d, s = b.step(None)
            for k, v in (("obs", o), ("reward", r), ("done", d), ("success", s)):
                assert np.array_equal(NC.bits(_np(out[k][t])), NC.bits(_np(v))), (what, t, k)
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert np.array_equal(NC.bits(_np(sa[k])), NC.bits(_np(sb[k]))), (what, k)
        assert np.isfinite(_np(sa["q"])).all(), what
        if name == "observation":
            assert not np.isfinite(_np(out["obs"])).all(), what      # the poison was there
    assert a.counters()["nonfinite"] == 0 and b.counters()["nonfinite"] == 0
    assert a.counters()["env_steps"] == 3 * n * (len(installs) + 1)
    print("C8 %s D=%d n=%d: %d installs, largest |action| %.9g" % (kind, D, n, len(installs) + 1, worst))
    a.close(); b.close()


@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("kind", ["actor", "actor_f16x3", "datd3", "daddpg"])
def test_forward_rows_are_independent(envs, kind, D):
    """C9: actor_forward / datd3_forward(want_q=True) on a batch whose rows {0, 31, 32, 63, 64, n - 1} are poisoned: every other row
    returns the bits of the clean batch (n = 261: four full waves and a ragged five; n = 64: one wave)"""
    rng = np.random.default_rng(12)
    e = _policy_env(envs, D, 64)
    _install(e, kind, _nets(rng, D))
    for n in (261, 64):
        rows = NC.poisoned_rows(n)
        assert rows == ((0, 31, 32, 63) if n == 64 else (0, 31, 32, 63, 64, 260))
        st = rng.uniform(-1, 1, (n, D)).astype(np.float32)
        fwd = (lambda x: (e.actor_forward(_dev(x)),)) if kind.startswith("actor") else (lambda x: e.datd3_forward(_dev(x), want_q=True))
        clean, bad = [_np(x) for x in fwd(st)], [_np(x) for x in fwd(NC.poison_rows(st))]
        again = [_np(x) for x in fwd(NC.poison_rows(st))]
        assert len(clean) == (1 if kind.startswith("actor") else 4)
        keep = np.array([r for r in range(n) if r not in rows])
        for x, y, z in zip(clean, bad, again):
            assert np.isfinite(x).all()
            assert np.array_equal(NC.bits(x[keep]), NC.bits(y[keep])), (kind, D, n, NC.differing_envs(x[keep], y[keep], 0)[:8])
            assert np.array_equal(NC.bits(y), NC.bits(z)), (kind, D, n)
        assert set(NC.differing_envs(clean[0], bad[0], 0)) <= set(rows) and len(NC.differing_envs(clean[0], bad[0], 0)) >= len(rows) - 1
    e.close()


@pytest.mark.parametrize("n", [192, 320])
@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("kind", POLICY_KINDS)
def test_fused_rollout_envs_are_independent(envs, kind, D, n):
    """C9 inside a rollout: envs {0, 31, 32, 63, 64, n - 1} get a NaN q through set_state, so their observation rows are NaN in the
    workgroup-cooperative actor forward (n = 192: three waves of one workgroup sharing the W2 ring; n = 320: a second, ragged
    workgroup).  Every other env matches the twin run bit for bit; every action is finite (C8); the poisoned envs are counted until
    their in-place reset (five steps each) and are the twin's afterwards."""
    rng = np.random.default_rng(13)
    nets = _nets(rng, D)
    steps = NC.EPISODE + 2
    rows = NC.poisoned_envs(n)
    runs = {}
    for which in ("poisoned", "twin"):
        e = _policy_env(envs, D, n, max_steps=NC.MAX_STEPS, reach_dis=NC.TINY, push_success_dis=NC.TINY)
        _install(e, kind, nets)
        e.reset()
        q = _np(e.get_state()["q"])
        if which == "poisoned":
            q[list(rows)] = NC.PNAN64
        e.set_state(q=_dev(q))
        out = e.rollout(steps, None, want_actions=True, want_terminal_obs=True)
        r = {k: _np(out[k]) for k in ("obs", "reward", "done", "success", "actions", "terminal_obs")}
        r.update({k: _np(v) for k, v in e.get_state().items()})
        r["nonfinite"] = e.counters()["nonfinite"]
        runs[which] = r
        e.close()
    p, t = runs["poisoned"], runs["twin"]
    what = (kind, D, n)
    assert p["nonfinite"] == len(rows) * NC.EPISODE and t["nonfinite"] == 0, (what, p["nonfinite"])
    assert np.isfinite(p["actions"]).all() and np.abs(p["actions"]).max() <= np.float32(0.7), what
    for k in p:
        if k == "nonfinite":
            continue
        axis = 1 if p[k].ndim >= 2 and p[k].shape[0] == steps and p[k].shape[1] == n else 0
        NC.assert_same_bits(p[k], t[k], axis, allowed=rows, what=(what, k))
    assert set(NC.differing_envs(p["terminal_obs"], t["terminal_obs"], 1)) == set(rows), what
    for k in ("obs", "reward", "done", "success", "actions", "terminal_obs"):      # healed by the in-place reset
        first = NC.EPISODE - 1 if k == "obs" else NC.EPISODE
        assert np.array_equal(NC.bits(p[k][first:]), NC.bits(t[k][first:])), (what, k)
    for k in ("q", "step", "episode", "ep_return", "trig"):
        assert np.array_equal(NC.bits(p[k]), NC.bits(t[k])), (what, k)


# ------------------------------------------------------------------ population learners

POP_POISONS = ("critic_weight", "batch", "adam_v")
_CRITIC = dict(td3="q1", daddpg="critic", datd3="critic1", darc="critic1")


def _pop_run(kind, D, hyper, poison):
    """three train calls (snapshots after the first and the third), exploit([0, 0, 2]), a fourth with member 1 on member 0's batch"""
    P, B = 3, 65
    gen = pc.generator(91)
    batches = [pc.batch(gen, P, B, D) for _ in range(4)]
    noises = pc.train_noises(kind, gen, P, B, 4)
    for t in batches[3].values():
        t[1].copy_(t[0])
    if noises[3] is not None:
        for z in (noises[3] if isinstance(noises[3], tuple) else (noises[3],)):
            z[1].copy_(z[0])
    pop = pc.population(kind, P, D, pc.generator(92))
    pop.always_hyper = hyper
    pop._hyper_changed()
    assert pop.entry_point.endswith("_hyper") == hyper
    if poison == "critic_weight":
        pop.stacks[_CRITIC[kind]][2][1, 100, 17] = float("nan")            # fc2.weight of member 1
    elif poison == "adam_v":
        pop.stacks[_CRITIC[kind] + "_v"][2][1, 100, 17] = float("inf")
    elif poison == "batch":
        for b in batches[:3]:
            b["rewards"][1, 40] = float("nan")
            b["states"][1, 64, 0] = float("inf")
    snaps, losses = [], []
    for i in range(3):
        losses.append(torch.stack(pc.train(kind, pop, batches[i], noises[i])).clone())
        if i in (0, 2):
            torch.cuda.synchronize(DEV)
            snaps.append([[t.clone() for t in pc.state(pop, p)] for p in range(P)])
    pop.exploit([0, 0, 2])
    torch.cuda.synchronize(DEV)
    snaps.append([[t.clone() for t in pc.state(pop, p)] for p in range(P)])
    losses.append(torch.stack(pc.train(kind, pop, batches[3], noises[3])).clone())
    torch.cuda.synchronize(DEV)
    snaps.append([[t.clone() for t in pc.state(pop, p)] for p in range(P)])
    return snaps, losses


def _tbits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(xs, ys):
    return all(torch.equal(_tbits(x), _tbits(y)) for x, y in zip(xs, ys))


@pytest.mark.parametrize("hyper", [False, True], ids=["uniform", "hyper"])
@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("kind", ["td3", "daddpg", "datd3", "darc"])
def test_a_diverged_member_cannot_touch_its_neighbours_and_exploit_heals_it(kind, D, hyper):
    """C10, P = 3, B = 65.  Member 1 poisoned one way at a time -- a NaN in a critic's fc2.weight; a NaN reward and a +inf state element
    in its batch; +inf in one element of its Adam second moment -- against the run in which it is clean: after one update and after
    three, every tensor of members 0 and 2 (nets, targets, both moments) and their losses are that run's bits.  exploit([0, 0, 2])
    then makes member 1 member 0's bits, all finite, and its next update (on member 0's batch and noise) equals member 0's."""
    clean, closs = _pop_run(kind, D, hyper, None)
    assert all(bool(torch.isfinite(t).all()) for snap in clean for member in snap for t in member)
    for poison in POP_POISONS:
        what = (kind, D, hyper, poison)
        snaps, losses = _pop_run(kind, D, hyper, poison)
        for i, (got, want) in enumerate(zip(snaps, clean)):
            for p in (0, 2):
                assert _same(got[p], want[p]), (what, "snapshot", i, "member", p)
        for i, (got, want) in enumerate(zip(losses, closs)):
            for p in (0, 2):
                assert torch.equal(_tbits(got[..., p].contiguous()), _tbits(want[..., p].contiguous())), (what, "loss", i, p)
        assert not _same(snaps[1][1], clean[1][1]), what                    # control: the poison did reach member 1
        if poison != "adam_v":
            assert not all(bool(torch.isfinite(t).all()) for t in snaps[1][1]), what
        healed = snaps[2]
        assert _same(healed[1], healed[0]) and all(bool(torch.isfinite(t).all()) for t in healed[1]), what
        assert _same(snaps[3][1], snaps[3][0]) and _same(snaps[3][0], clean[3][0]), what
        assert torch.equal(_tbits(losses[3][..., 1].contiguous()), _tbits(losses[3][..., 0].contiguous())), what
        assert all(bool(torch.isfinite(t).all()) for member in snaps[3] for t in member), what
