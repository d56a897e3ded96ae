"""CPU tests of tests/learner_ref64.py for DADDPG, DATD3 and DARC, the float64 restatement of one update that the fused HIP updates are
tested against: it reproduces the reference's recorded runs (G16, G17, G18), equals torch autograd in float64 over
armenv.daddpg.DADDPG and armenv.datd3.DATD3 / DARC for both parities, every defect switch breaks that equality under hyper-parameters
that make it bind, and every case of tests/test_gpu_da_ref64.py (tests/learner_cases.py) keeps its share of ambiguous relu units
under the cap (the bodies shared with tests/test_td3_ref64.py are tests/learner_ref64_checks.py's).  Also: the case table as a
whole, TD3's cases included."""
import numpy as np
import pytest
import torch

from conftest import golden_npz
import learner_cases as K
import learner_ref64 as R
pytest.register_assert_rewrite("learner_ref64_checks")          # the shared bodies assert there
import learner_ref64_checks as X  # noqa: E402
from datd3_golden import KEYS, expected_losses, load_train_fixture

AGENTS = K.AGENTS[1:]
# an f32 gradient of the torch learner on the CPU against the float64 one, in units of 2^-24 M: M carries the magnitudes through the
# whole chain, so each rounding anywhere in it moves an element by at most 2^-24 M; six contractions, each summed in blocks (a few
# roundings deep at these widths), stay under 8 of them
C_TORCH = 8.0


def test_daddpg_reference_reproduces_the_golden_updates():
    """G16: the eight DADDPG_MLP.update calls of tests/golden/daddpg_train_seed0.npz (B = 64) from torch.manual_seed(0)'s initial
    weights, update n stepping actor 1 when n is even: the tolerances of test_reference_reproduces_the_golden_updates."""
    from armenv.daddpg import DADDPG
    g = golden_npz("daddpg_train_seed0.npz")
    torch.manual_seed(0)
    st = X.zeros("daddpg", DADDPG(6, 3, 0.7, device="cpu"))
    for i, want in enumerate(g["losses"]):
        b = {k: torch.from_numpy(g[f"b{i}_{k}"]).to(torch.float64) for k in KEYS}
        out = R.update("daddpg", st, b, None, X.HP_GOLDEN, k=1 if (i + 1) % 2 == 0 else 2)
        assert abs(out["loss"] - want) < 1e-5 * max(1.0, abs(want)), (i, out["loss"], want)
        st = R.advance(st, out)
    assert (st["critic_step"], st["actor1_step"], st["actor2_step"]) == (8, 4, 4)
    X.assert_golden_nets("daddpg", st, g)


@pytest.mark.parametrize("agent", ["datd3", "darc"])
def test_datd3_reference_reproduces_the_golden_updates(agent):
    """G17 / G18: four `train` calls (update k = 1 then k = 2 on the same batch) with the recorded noise: all eight losses and
    every parameter at the tolerances of test_reference_reproduces_the_golden_updates -- except G17's actor 2 and its target.  The
    recorded f32 run put a relu unit of update 4 (train call 2, k = 2) on the other side of zero than exact arithmetic does: the
    f32 torch learner replayed here reproduces the recording to 1e-7 in every element, its actor-2 gradient of that update lies
    5.4e-5 from the float64 one, inside C 2^-24 M + allowance and outside C 2^-24 M, and Adam turns that into lr-sized differences
    (1188 of actor 2's 68 355 elements beyond 1e-5, the largest 1.4e-3) that later updates of actor 2 keep.  Those two nets are held to
    the 7e-3 of test_fused_update_reproduces_the_golden_updates, and the test asserts the cause: up to that update the f32 gradients
    are within the bound with the allowance, that update's is beyond it without."""
    from armenv.datd3 import DARC, DATD3
    darc = agent == "darc"
    g = load_train_fixture(agent + "_train_seed0")
    torch.manual_seed(0)
    t = (DARC if darc else DATD3)(6, 3, 0.7, device="cpu")
    st = X.zeros(agent, t)
    want = expected_losses(g, darc)
    flips = []
    for i in range(4):
        b32 = {k: torch.from_numpy(g[f"b{i}_{k}"]) for k in KEYS}
        b = {k: v.to(torch.float64) for k, v in b32.items()}
        for k in (1, 2):
            n32 = torch.from_numpy(g["noise"][2 * i + k - 1])
            out = R.update(agent, st, b, n32.to(torch.float64), X.HP_GOLDEN, k=k)
            w = want[2 * i + k - 1]
            assert abs(out["loss"] - w) < 1e-5 * max(1.0, abs(w)), (i, k, out["loss"], w)
            st = R.advance(st, out)
            if not darc and not flips:                 # the f32 learner beside the reference, until their states part
                t.update(b32, k == 1, n32)
                g32 = [p.grad.to(torch.float64) for p in getattr(t, "actor%d" % k).parameters()]
                quad = list(zip(g32, out["actor_grad"], out["actor_grad_mag"], out["actor_grad_allow"]))
                assert sum(R.bad_elements(x, y, m, a, C_TORCH)[0] for x, y, m, a in quad) == 0, (i, k)
                if sum(R.bad_elements(x, y, m, torch.zeros_like(a), C_TORCH)[0] for x, y, m, a in quad):
                    flips.append((i, k))
    assert all(st[n + "_step"] == 4 for n in R.LEARNING[agent])
    assert flips == ([] if darc else [(1, 2)])
    X.assert_golden_nets(agent, st, g, flipped=() if darc else ("actor2", "target_actor2"))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("B,D", [(B, D) for B in (1, 5, 257) for D in (1, 6, 9)])
@pytest.mark.parametrize("agent", AGENTS)
def test_reference_equals_autograd_in_float64(agent, B, D, k):
    """both parities of DADDPG and both k of DATD3 / DARC, several chunks at B = 257"""
    X.check_reference_equals_autograd(agent, B, D, k, 7 * B + D)


@pytest.mark.parametrize("agent,defect", [(a, d) for a in AGENTS for d in R.DEFECTS[a]])
def test_every_defect_switch_breaks_the_autograd_comparison(agent, defect):
    X.check_defect_switch(agent, defect)


def test_defect_lists():
    """the eight common defects, two more for TD3, three for DADDPG, four for DATD3 and four more again for DARC"""
    assert len(R.COMMON_DEFECTS) == 8 and all(set(R.COMMON_DEFECTS) < set(R.DEFECTS[a]) for a in K.AGENTS)
    assert {a: len(set(d)) for a, d in R.DEFECTS.items()} == dict(td3=10, daddpg=11, datd3=12, darc=16)
    assert set(R.DEFECTS["td3"]) < set(R.DEFECTS["datd3"]) < set(R.DEFECTS["darc"])
    daddpg = next(c for c in K.GRAD_CASES if c["agent"] == "daddpg")
    with pytest.raises(AssertionError):
        K.reference(daddpg, K.build(daddpg), defect="no_noise_clip")      # a DADDPG case: it has no noise


def test_mix_weights_are_the_two_f32_values_of_the_kernel():
    w_min, w_max = R.mix_weights(dict(q_weight=float(np.float32(0.2))))
    assert w_min == float(np.float32(0.2)) and w_max == float(np.float32(1.0 - float(np.float32(0.2))))
    assert w_min + w_max != 1.0 and abs(w_min + w_max - 1.0) < 2.0 ** -24         # the mix is not the identity, to rounding only
    assert R.mix_weights(dict(q_weight=0.0)) == (0.0, 1.0) and R.mix_weights(dict(q_weight=1.0)) == (1.0, 0.0)


# ---- the GPU tests' inputs ----

def test_gpu_cases_are_distinct_and_cover_the_issue():
    ids = [K.case_id(c) for c in K.ALL_CASES]
    assert len(set(ids)) == len(ids)
    shapes = lambda agent, wa: {(c["B"], c["D"]) for c in K.GRAD_CASES if c["agent"] == agent and c["with_actor"] == wa}
    assert len(K.GRAD_SHAPES) == 22 and all(shapes(agent, True) == set(K.GRAD_SHAPES) for agent in AGENTS)
    assert shapes("td3", True) == shapes("td3", False) == set(K.GRAD_SHAPES) | {(65536, 6)} | {(2048, D) for D in (1, 3, 9, 12)}
    assert len(K.GRAD_CASES) == 6 * 22 + 2 * 27
    assert max(c["B"] for c in K.ALL_CASES) == 65536 and max(c["B"] for c in K.ALL_CASES if c["agent"] != "td3") == 4097
    for cases, kinds in ((K.ADAM_CASES, 8), (K.EDGE_CASES, 4), (K.EXACT_CASES, 4), (K.DEFECT_CASES, 2)):
        assert all(sum(c["agent"] == agent for c in cases) >= kinds for agent in K.AGENTS)
    assert [c["B"] for c in K.DEFECT_CASES if c["agent"] == "td3"] == [65, 257, 2048]
    assert K.NOISE_CASES[0]["hp"] != K.NOISE_CASES[-1]["hp"] and K.NOISE_CASES[0]["hp"]["action_bound"] == 8.0


@pytest.mark.parametrize("c", [c for c in K.ALL_CASES if c["agent"] != "td3"], ids=K.case_id)
def test_gpu_case_inputs_keep_ambiguity_rare(c):
    X.check_case_inputs(c)
