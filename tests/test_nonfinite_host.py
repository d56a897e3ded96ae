"""The case table of tests/nonfinite_cases.py on the CPU oracle (no GPU): the table regenerates identically; the `nonfinite` counts it
states by a closed form are the ones the oracle gives when stepped through the cases; what a NaN action does under both IK exit modes
(C4) and that +-inf / huge actions are the box-clipped finite ones bit for bit (C3) on the oracle; the comparison helpers report
planted differences; the numpy restatement of armenv_summary sums NaN and skips it in the max."""
import hashlib

import numpy as np
import pytest

import nonfinite_cases as NC


def _digest(case):
    h = hashlib.sha256()
    for which in ("poisoned", "twin"):
        h.update(NC.actions_for(case, which).tobytes())
    fields = dict(q=np.arange(NC.N * 7, dtype=np.float64).reshape(NC.N, 7), step=np.zeros(NC.N, dtype=np.int32),
                  goal=np.ones((NC.N, 3), dtype=np.float32), aux=np.ones((NC.N, 12)))
    for which in ("poisoned", "twin"):
        for k, v in sorted(NC.apply_state(case, which, fields).items()):
            h.update(k.encode() + v.tobytes())
    return h.hexdigest()


def test_the_table_regenerates_identically_and_poisons_the_fixed_envs_only():
    assert NC.POISONED == (0, 31, 32, 63, 64, NC.N - 1) and NC.N == 133 and NC.T == 12 and NC.EPISODE == 5
    base = NC.base_actions()
    assert np.array_equal(NC.bits(base), NC.bits(NC.base_actions())) and np.isfinite(base).all() and np.abs(base).max() <= 0.7
    for case in NC.CASES.values():
        assert _digest(case) == _digest(case)
        assert set(case.get("action", case.get("state"))) == set(NC.POISONED), case["name"]
        a, b = NC.actions_for(case, "poisoned"), NC.actions_for(case, "twin")
        assert set(NC.differing_envs(a, b, axis=1)) <= set(NC.POISONED)
        assert np.isfinite(b).all()
        if "action" in case:
            assert NC.differing_envs(a, b, axis=1) == sorted(NC.POISONED)
            for env, (t, _) in case["action"].items():      # one poisoned step per env, the rest are the base actions
                assert NC.differing_envs(a[:, env:env + 1], b[:, env:env + 1], axis=0) == [t]
        else:
            assert np.array_equal(NC.bits(a), NC.bits(b))
    # both NaN signs and both infinities occur among the actions, and the payloads are the stated bit patterns
    a = NC.actions_for(NC.CASES["nan_action"], "poisoned").view(np.uint32)
    assert (a == NC.NAN_POS).any() and (a == NC.NAN_NEG).any()
    s = NC.actions_for(NC.CASES["saturate"], "poisoned")
    assert (s == np.inf).any() and (s == -np.inf).any() and (s == np.float32(1e30)).any() and (s == np.float32(3e38)).any()


def test_closed_form_intervals():
    c = NC.CASES["nan_action"]
    assert [NC.diverged(c, e) for e in NC.POISONED] == [(0, 4, True), (3, 4, True), (4, 4, True), (6, 9, True), (9, 9, True), (11, 11, False)]
    assert NC.expected_nonfinite(c) == 5 + 2 + 1 + 4 + 1 + 1
    s = NC.CASES["q_state"]
    assert [NC.diverged(s, e) for e in NC.POISONED] == [(0, 4, True), (0, 3, True), (0, 2, True), (0, 1, True), (0, 0, True), (0, 2, True)]
    assert NC.expected_nonfinite(s) == 5 + 4 + 3 + 2 + 1 + 3
    assert NC.expected_nonfinite(NC.CASES["saturate"]) == 0 and NC.expected_nonfinite(NC.CASES["nan_action_exit1"]) == 0
    assert NC.diverged_mask(c).sum() == 14 and NC.diverged_mask(c)[:, [e for e in range(NC.N) if e not in NC.POISONED]].sum() == 0


@pytest.fixture(scope="module")
def runs(O, kuka):
    """every case of every task on the oracle, once: (task, case name) -> oracle_run"""
    return {(task, c["name"]): NC.oracle_run(O, kuka, task, c) for task in NC.TASKS for c in NC.cases_of(task)}


@pytest.mark.parametrize("task", NC.TASKS)
def test_nonfinite_counts_oracle_and_closed_form_agree(runs, task):
    """C2's expected number two ways: counted on the oracle (q not all-finite after the step, before the reset) and by the closed form
    of the table; (env, step) by (env, step), not only in total"""
    nonzero = 0
    for c in NC.cases_of(task):
        r = runs[(task, c["name"])]
        want = NC.diverged_mask(c) if c["q_bad"] else np.zeros((NC.T, NC.N), dtype=bool)
        assert np.array_equal(r["q_bad"], want), (task, c["name"], np.argwhere(r["q_bad"] != want)[:8].tolist())
        NC.assert_count(r["q_bad"].sum(), NC.expected_nonfinite(c), (task, c["name"]))
        nonzero += NC.expected_nonfinite(c) > 0
        # every episode of every env takes EPISODE steps: the twins reset on the same steps
        done_want = np.zeros((NC.T, NC.N), dtype=bool)
        for env in range(NC.N):
            s0 = NC.first_step(c, env)[0] if env in NC.POISONED else 0
            done_want[[t for t in range(NC.T) if (s0 + t) % NC.EPISODE == NC.EPISODE - 1], env] = True
        assert np.array_equal(r["done"], done_want) and not r["success"].any(), (task, c["name"])
    assert nonzero >= 2


@pytest.mark.parametrize("task", NC.TASKS)
def test_nan_action_outcome_under_both_exit_modes(runs, task):
    """C4 on the oracle.  ik_exit_mode 0 (Bullet's loop): the first trip's update always runs, on a NaN target: ONE update, and the
    joints the IK writes are all NaN (pick: joints 1..6, joint 7 keeps its reset value) until the next reset; every later step of
    the episode again applies one update.  ik_exit_mode 1 (test before update): `!(NaN > residual)` stops the loop: ZERO updates, q
    untouched and finite."""
    r0, r1 = runs[(task, "nan_action")], runs[(task, "nan_action_exit1")]
    written = 6 if task == "pick" else 7
    for env, (t, _) in NC.CASES["nan_action"]["action"].items():
        t0, t1, _ = NC.diverged(NC.CASES["nan_action"], env)
        assert (r0["updates"][t0:t1 + 1, env] == 1).all(), (task, env)
        assert r0["q_nan"][t0:t1 + 1, env, :written].all() and not r0["q_nan"][t0:t1 + 1, env, written:].any(), (task, env)
        assert r0["obs_bad"][t0:t1 + 1, env].all()
        assert np.isnan(r0["reward"][t0:t1 + 1, env]).all() == (task == "reach"), (task, env)      # the cube tasks' reward reads the cube only
        assert r1["updates"][t, env] == 0 and not r1["q_nan"][:, env].any() and not r1["obs_bad"][:, env].any(), (task, env)
        assert np.isfinite(r1["reward"][:, env]).all(), (task, env)
    clean = [e for e in range(NC.N) if e not in NC.POISONED]
    assert not r0["q_nan"][:, clean].any() and np.isfinite(r0["reward"][:, clean]).all()


@pytest.mark.parametrize("task", NC.TASKS)
def test_saturating_actions_equal_the_clipped_finite_ones_on_the_oracle(O, kuka, runs, task):
    """C3: +-inf, 1e30 and 3e38 components act as `beyond the box`: every number of the run equals the run with 1e6 in their place"""
    c = NC.CASES["saturate"]
    a, b = runs[(task, "saturate")], NC.oracle_run(O, kuka, task, c, which="twin")
    for k in a:
        assert np.array_equal(NC.bits(a[k]), NC.bits(b[k])), (task, k)
    assert np.isfinite(a["obs"]).all() and np.isfinite(a["q"]).all()
    base = NC.oracle_run(O, kuka, task, NC.CASES["nan_action"], which="twin")      # the base actions: the saturating ones did act
    assert NC.differing_envs(a["obs"], base["obs"], axis=1) == sorted(NC.POISONED)
    for env, (t, _) in c["action"].items():
        assert a["updates"][t, env] >= 2, (task, env)


def test_joint7_case_leaves_the_observation_finite(runs):
    """the q7_exit1 case: no update runs, q stays non-finite in joint 7 alone, the observation is finite: a count taken from the
    observation would be zero"""
    for task in NC.CASES["q7_exit1"]["tasks"]:
        r = runs[(task, "q7_exit1")]
        m = NC.diverged_mask(NC.CASES["q7_exit1"])
        assert r["q_bad"][m].all() and (r["updates"][m] == 0).all() and not r["obs_bad"].any(), task
        assert r["q_nan"][m][:, 6].all() and not r["q_nan"][m][:, :6].any(), task


def test_goal_and_cube_state_poison_is_not_a_joint_poison(runs):
    for task, name in (("reach", "goal"), ("push", "aux"), ("pick", "aux")):
        r = runs[(task, name)]
        m = NC.diverged_mask(NC.CASES[name])
        # (d_last is not observed and the falling cube's height is recomputed from the step count: not every cube poison shows in obs)
        assert not r["q_bad"].any() and (r["obs_bad"][m].all() if task == "reach" else r["obs_bad"][m].sum() >= 8), (task, name)
        assert not r["obs_bad"][~m].any(), (task, name)


@pytest.mark.parametrize("task", NC.TASKS)
def test_every_poison_shows_in_its_own_env_and_in_no_other(O, kuka, runs, task):
    """the control of the GPU tests, on the oracle: against the twin run every poisoned env differs in an output, and no other env does
    (the joint-7 case changes q alone, a saturating action equals its stand-in: no output differs there)"""
    for c in NC.cases_of(task):
        a, b = runs[(task, c["name"])], NC.oracle_run(O, kuka, task, c, which="twin")
        changed = set(NC.differing_envs(a["obs"], b["obs"], 1)) | set(NC.differing_envs(a["reward"], b["reward"], 1))
        assert changed == (set() if c["name"] in ("saturate", "q7_exit1") else set(NC.POISONED)), (task, c["name"], sorted(changed))
        assert not b["q_bad"].any() and not b["obs_bad"].any(), (task, c["name"])


# ------------------------------------------------------------------ the helpers report planted differences

def test_helpers_report_a_flipped_bit_in_a_clean_envs_reward():
    rew = np.random.default_rng(1).normal(size=(NC.T, NC.N)).astype(np.float32)
    other = rew.copy()
    other.view(np.uint32)[7, 40] ^= 1
    assert NC.differing_envs(rew, other, axis=1) == [40]
    with pytest.raises(AssertionError):
        NC.assert_same_bits(rew, other, axis=1, allowed=NC.POISONED)
    other = rew.copy()
    other.view(np.uint32)[7, 32] ^= 1                     # in a poisoned env it is allowed, and only there
    NC.assert_same_bits(rew, other, axis=1, allowed=NC.POISONED)
    with pytest.raises(AssertionError):
        NC.assert_same_bits(rew, other, axis=1)
    with pytest.raises(AssertionError):                   # no env but the table's may be excused
        NC.assert_same_bits(rew, rew, axis=1, allowed=(40,))
    z = np.zeros((2, NC.N))
    assert NC.differing_envs(z, -z, axis=1) == list(range(NC.N))      # -0 is not +0


def test_helpers_report_a_nan_with_another_payload():
    a = np.full((NC.T, NC.N), NC.PNAN, dtype=np.float32)
    NC.assert_same_bits(a, a.copy(), axis=1)              # NaN equals itself, bit for bit
    b = a.copy()
    b.view(np.uint32)[3, 5] = NC.NAN_POS | 1
    c = a.copy()
    c.view(np.uint32)[3, 6] = NC.NAN_NEG
    assert np.isnan(b).all() and np.isnan(c).all()
    assert NC.differing_envs(a, b, axis=1) == [5] and NC.differing_envs(a, c, axis=1) == [6]
    for other in (b, c):
        with pytest.raises(AssertionError):
            NC.assert_same_bits(a, other, axis=1, allowed=NC.POISONED)
    d = np.full(4, NC.PNAN64)
    e = d.copy()
    e.view(np.uint64)[2] |= 1
    assert NC.differing_envs(d, e, axis=0) == [2]


def test_a_count_without_the_episodes_last_step_is_reported(runs):
    c = NC.CASES["nan_action"]
    short = 0
    for env in NC.POISONED:
        t0, t1, resets = NC.diverged(c, env)
        short += t1 - t0 + (0 if resets else 1)           # leaves out the step on which the env is reset
    assert short == NC.expected_nonfinite(c) - 5
    with pytest.raises(AssertionError):
        NC.assert_count(short, runs[("reach", "nan_action")]["q_bad"].sum())


def test_a_count_taken_from_the_observation_is_reported(runs):
    r = runs[("reach", "q7_exit1")]
    from_obs = r["obs_bad"].sum()
    assert from_obs == 0 and NC.expected_nonfinite(NC.CASES["q7_exit1"]) == 18
    with pytest.raises(AssertionError):
        NC.assert_count(from_obs, r["q_bad"].sum())
    g = runs[("reach", "goal")]                            # and the other way round: a NaN goal makes the observation NaN, not q
    with pytest.raises(AssertionError):
        NC.assert_count(g["obs_bad"].sum(), g["q_bad"].sum())


# ------------------------------------------------------------------ armenv_summary restated

def test_summary_restatement_sums_nan_and_skips_it_in_the_max():
    rng = np.random.default_rng(2)
    for n in (64, 133, 2048 + 64 + 5):
        dist = rng.integers(1, 1000, n).astype(np.float64)        # integers: every order of summation gives the same bits
        ret = -rng.integers(0, 500, n).astype(np.float64)
        ln = rng.integers(1, 6, n).astype(np.float64)
        su = rng.integers(0, 2, n).astype(np.float64)
        out = NC.summary_restated(dist, ret, ln, su)
        assert out.tolist() == [dist.sum(), dist.max(), ret.sum(), ln.sum(), su.sum(), float(n), 0.0, 0.0]
        bad = n - 2
        d2, r2 = dist.copy(), ret.copy()
        d2[bad] = np.nan
        r2[bad] = np.nan
        p = NC.summary_restated(d2, r2, ln, su)
        assert np.isnan(p[0]) and np.isnan(p[2])                  # the sums propagate it
        assert p[1] == np.delete(dist, bad).max()                 # fmax skips it
        assert p[3:].tolist() == out[3:].tolist()
        d2[bad] = np.inf
        assert NC.summary_restated(d2, ret, ln, su)[1] == np.inf  # an infinity is a value, not skipped


def test_policy_poison_table():
    rng = np.random.default_rng(3)
    sd = NC.mlp(rng, 9, 3)
    assert [sd[k].shape for k in NC.MLP_KEYS] == [(256, 9), (256,), (256, 256), (256,), (3, 256), (3,)]
    for name, v in NC.POLICY_VALUES.items():
        for place in NC.POLICY_PLACES:
            p = NC.poison_mlp(sd, v, place)
            changed = [k for k in NC.MLP_KEYS if not np.array_equal(NC.bits(p[k]), NC.bits(sd[k]))]
            assert changed == (list(NC.MLP_KEYS) if place == "all" else [place]), (name, place)
            assert all((NC.bits(p[k]) != NC.bits(sd[k])).sum() == 1 for k in changed)
    assert NC.POLICY_VALUES["above_f16"] > 65504 and np.isfinite(NC.POLICY_VALUES["above_f16"])
    assert NC.POLICY_VALUES["nan_pos"].view(np.uint32) == NC.NAN_POS and NC.POLICY_VALUES["nan_neg"].view(np.uint32) == NC.NAN_NEG
