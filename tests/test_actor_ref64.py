"""CPU tests of tests/actor_ref64.py and tests/actor_cases.py, the float64 restatement, derived bounds and case table that
tests/test_gpu_actor_ref64.py holds the fused policy forwards (exact-f32 actor, f16x3 actor, the four-net take_action pass) against:
the reference reproduces the recorded golden vectors and the C oracle at nominal scale; every case meets its conditions (outputs not
saturated, picks balanced and clear); a faithful numpy emulation of the f16x3 arithmetic stays inside the derived bound on every
output of every case; and every entry of actor_ref64.DEFECTS leaves it on some case of every agent it applies to -- so a kernel that
is wrong in one of those ways cannot pass the GPU file."""
import numpy as np
import pytest

from conftest import golden_npz
import actor_cases as K
import actor_ref64 as R


def _net(g, prefix=""):
    return {k: g[prefix + k.replace(".", "_")] for k in R.KEYS}


def test_forward64_reproduces_the_golden_actor_vectors(O):
    g = golden_npz("td3_actor_seed0.npz")
    net, bound = _net(g), float(g["action_bound"])
    out = R.forward64(net, g["states"], bound, False)["out"]
    assert np.abs(out - g["actions"]).max() < 1e-5
    assert np.abs(out - O.actor_forward(net, g["states"], bound)).max() < 1e-5
    g9 = golden_npz("td3_actor9_seed0.npz")                       # weights only: against the oracle on random push observations
    st = np.random.default_rng(0).uniform(-1, 1, (300, 9)).astype(np.float32)
    assert np.abs(R.forward64(_net(g9), st, 0.7, False)["out"] - O.actor_forward(_net(g9), st, 0.7)).max() < 1e-5
    gd = golden_npz("ddpg_take_action_seed0.npz")
    assert np.abs(R.forward64(_net(gd, "actor_"), gd["states"], float(gd["action_bound"]), False)["out"] - gd["actions"]).max() < 1e-5


@pytest.mark.parametrize("name", ["datd3_take_action_seed0", "datd3_take_action9_seed0", "darc_take_action_seed0",
                                  "daddpg_take_action_seed0", "daddpg_take_action9_seed0"])
def test_take_action64_reproduces_the_golden_choices(O, name):
    g = golden_npz(name + ".npz")
    if name.startswith("daddpg"):
        c = _net(g, "critic_")
        nets = (_net(g, "actor1_"), _net(g, "actor2_"), c, c)
    else:
        nets = tuple(_net(g, p + "_") for p in ("actor1", "actor2", "critic1", "critic2"))
    bound = float(g["action_bound"])
    t = R.take_action64(nets, g["states"], bound)
    assert np.abs(t["q1"] - g["q1"]).max() < 1e-5 and np.abs(t["q2"] - g["q2"]).max() < 1e-5
    clear = np.abs(g["q1"] - g["q2"]) > 1e-4
    assert clear.sum() > 200 and np.array_equal(t["picked"][clear], g["picked_actor"][clear].astype(np.uint8))
    assert np.abs(t["action"] - g["actions"])[clear].max() < 1e-5
    a, q1, q2, pk = O.datd3_take_action(nets, g["states"], bound)
    assert np.abs(t["q1"] - q1).max() < 1e-5 and np.abs(t["q2"] - q2).max() < 1e-5 and np.array_equal(t["picked"][clear], pk[clear])


def test_the_split_bounds_hold_on_every_f32_magnitude():
    """|v - hi| <= e1(v), |v - hi - lo| <= d(v), |lo| <= e1(v) + d(v) over magnitudes from below 2^-25 to 65504, the planted edges
    included; lo is an f16 subnormal for every |v| < 2^-3 that is not f16-representable"""
    rng = np.random.default_rng(1)
    v = (rng.uniform(1, 2, 200000) * 2.0 ** rng.integers(-30, 16, 200000) * rng.choice([-1, 1], 200000)).astype(np.float32)
    v = np.concatenate([v[np.abs(v) <= 65504], np.float32([65504, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 0.0]),
                        np.nextafter(np.float32([2.0 ** -14, 2.0 ** -24, 2.0 ** -25]), np.float32(1))])
    hi, lo = (a.astype(np.float64) for a in R.split16(v))
    av = np.abs(v.astype(np.float64))
    assert np.all(np.isfinite(hi)) and np.all(np.abs(v - hi) <= R._e1(av)) and np.all(np.abs(v - hi - lo) <= R._d(av))
    assert np.all(np.abs(lo) <= R._e1(av) + R._d(av))
    small = (av < 2.0 ** -3) & (lo != 0)
    assert small.any() and np.all(np.abs(lo[small]) < 2.0 ** -14)


# ----------------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("cid", [c["id"] for c in K.SINGLE])
def test_single_net_case_is_informative_and_the_emulation_is_inside_the_bound(cid):
    s = K.single(cid)
    z = np.abs(s["ref"]["z"])
    assert (z < 2).mean() >= K.SAT_MIN, (z < 2).mean()
    assert np.all(np.isfinite(s["b16"]["out"])) and np.all(s["b16"]["out"] > 0) and np.all(s["b32"]["out"] <= s["b16"]["out"])
    if K.by_id(cid)["kind"] == "domain-edge":
        assert 3e4 < s["ref"]["h1"].max() < 65504
    emu = R.emulate_f16x3(s["net"], s["x"], s["bound"], False)
    assert np.all(np.isfinite(emu))
    ratio = np.abs(emu - s["ref"]["out"]) / s["b16"]["out"]
    assert ratio.max() <= 1.0, ratio.max()


@pytest.mark.parametrize("cid", [c["id"] for c in K.FOUR])
def test_four_net_case_is_balanced_and_the_emulation_is_inside_the_bound(cid):
    f = K.four(cid)
    b, c = f["b"], K.by_id(cid)
    amb, rare = K.four_conditions(b)
    if c["kind"] == "identical-actors":
        assert f["nets"][1] is not f["nets"][0] and np.array_equal(b["ref"]["q1"], b["ref"]["q2"]) and not b["ref"]["picked"].any()
    else:
        assert amb <= K.AMB_MAX and rare >= K.PICK_MIN, (amb, rare)
    assert (c["agent"] == "daddpg") == (f["nets"][3] is f["nets"][2])
    for fw in b["ref"]["fwd"][:2]:
        assert (np.abs(fw["z"]) < 2).mean() >= K.SAT_MIN
    emu = R.emulate_take_action(f["nets"], f["x"], f["bound"])
    r = R.take_action_ratios(emu, b)
    assert r["picks_agree"] and max(r["q1"], r["q2"], r["action"]) <= 1.0, r
    if c["kind"] == "identical-actors":
        assert np.array_equal(emu["q1"], emu["q2"]) and not emu["picked"].any()


# ----------------------------------------------------------------------------------------------------------- defects
def _single_detects(cid, defect):
    s = K.single(cid)
    emu = R.emulate_f16x3(s["net"], s["x"], s["bound"], False, defect)
    return not np.all(np.abs(emu - s["ref"]["out"]) <= s["b16"]["out"])


def _four_detects(cid, defect):
    f = K.four(cid)
    r = R.take_action_ratios(R.emulate_take_action(f["nets"], f["x"], f["bound"], defect), f["b"])
    return not (r["picks_agree"] and max(r["q1"], r["q2"], r["action"]) <= 1.0)


def _coherent_first(cases):
    return sorted(cases, key=lambda c: not c["kind"].startswith("coherent"))


@pytest.mark.parametrize("defect", sorted(R.DEFECTS))
@pytest.mark.parametrize("agent", ["actor", "ddpg", "datd3", "darc", "daddpg"])
def test_every_defect_leaves_the_bound_on_a_case_of_every_agent(agent, defect):
    """(the single-net agents go through the f16x3 kind: the exact-f32 actor has no split to get wrong)"""
    four = agent in ("datd3", "darc", "daddpg")
    if R.DEFECTS[defect] == "two" and not four:
        return                                   # a four-net defect: nothing to read from another net
    cases = _coherent_first([c for c in (K.FOUR if four else K.SINGLE) if c["agent"] == agent])
    assert cases
    assert any((_four_detects if four else _single_detects)(c["id"], defect) for c in cases), "no %s case detects %s" % (agent, defect)


def test_mixed_scale_inputs_of_the_batch_and_fused_tests_are_informative():
    for D in (6, 9):
        net, x = K.mixed_single(D, 1024 + 192)
        assert (np.abs(R.forward64(net, x, K.BOUND, False)["z"]) < 2).mean() >= K.SAT_MIN
        for shared in (False, True):
            amb, rare = K.four_conditions(K.mixed_four(D, 1024 + 192, shared)["b"])
            assert amb <= K.AMB_MAX and rare >= K.PICK_MIN, (D, shared, amb, rare)
