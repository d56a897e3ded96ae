"""The fused DADDPG, DATD3 and DARC updates (armenv_daddpg_update / armenv_datd3_update through FusedDADDPG.train, FusedDATD3.update
and FusedDARC.update) on cuda:0 against the float64 restatement of tests/learner_ref64.py, as tests/test_gpu_td3_ref64.py holds TD3:
per element, |g_hip - g_ref| <= C 2^-24 M_ref + allowance_ref.  Every input is a case of tests/learner_cases.py, built on the CPU and
moved to the device (tests/test_da_ref64.py checks the same inputs for ambiguity without a GPU); the harness, the C table and the
bodies that both modules hold are tests/learner_ref64_gpu.py's (profiles/learner_ref64_errors.txt records the largest measured ratios
over all four agents)."""
import pytest

pytest.register_assert_rewrite("learner_ref64_gpu")          # the shared bodies assert there
import learner_cases as K  # noqa: E402
import learner_ref64 as R  # noqa: E402
import learner_ref64_gpu as G  # noqa: E402

pytestmark = pytest.mark.gpu
AGENT_K = [x for x in K.AGENT_K if x[0] != "td3"]


def _da(cases):
    return [c for c in cases if c["agent"] != "td3"]


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    G.write_ratios()


@pytest.mark.parametrize("c", _da(K.GRAD_CASES), ids=K.case_id)
def test_gradients_and_loss_against_float64(c):
    """All 6 critic and 6 actor gradient tensors and the loss, element by element, within C 2^-24 M + allowance, for both parities
    of DADDPG and both k of DATD3 / DARC, at batch sizes around the 4 rows of a head block, the 64-row gemm tile, the 256-row
    weight-gradient slice and the 256-thread loss reduction, and at five state widths.  In the same run, everything that the update
    does not own -- the other actor with its moments and target, DATD3's / DARC's other critic with its moments and target, DADDPG's
    target critic on update 1 -- is bitwise unchanged."""
    G.against_float64(c)


@pytest.mark.parametrize("c", _da(K.DEFECT_CASES), ids=K.case_id)
def test_every_defect_fails_a_gpu_comparison(c):
    G.check_every_defect_fails(c)


@pytest.mark.parametrize("step", K.ADAM_STEPS)
@pytest.mark.parametrize("agent,k", AGENT_K)
def test_adam_and_soft_update_against_float64(agent, k, step):
    G.check_adam_and_soft_update(agent, k, step)


@pytest.mark.parametrize("agent,k", AGENT_K)
def test_lr_zero_and_tau_edges_are_exact(agent, k):
    G.check_lr_zero_and_tau_edges(agent, k)


@pytest.mark.parametrize("agent,k", AGENT_K)
def test_with_every_done_set_no_target_net_is_read(agent, k):
    G.check_every_done_set(agent, k)


@pytest.mark.parametrize("agent,k", [x for x in AGENT_K if x[0] != "daddpg"])
def test_noise_clip_zero_equals_no_noise_bit_for_bit(agent, k):
    G.check_noise_clip_zero_equals_no_noise(agent, k)


@pytest.mark.parametrize("q_weight", [0, 1])
@pytest.mark.parametrize("k", [1, 2])
def test_darc_without_regulariser_and_with_a_trivial_mix_is_datd3_bit_for_bit(k, q_weight):
    """FusedDARC with regularization_weight = 0 and q_weight 0 or 1 equals FusedDATD3 from the same state in every parameter, moment
    and target and in the loss: 0 T + 1 T, d3 + 0 (...) and red0 inv_b + 0 (...) are exact, and the loss column keeps its summation
    order between one column and two."""
    c = K.exact_case("darc", k, "as_datd3_q%d" % q_weight)
    built = K.build(c)
    got = G.update(G.make(c, built), c, built)
    c3 = dict(c, agent="datd3", hp={n: c["hp"][n] for n in R.HP_KEYS["datd3"]})
    got3 = G.update(G.make(c3, built), c3, built)
    assert got["loss"] == got3["loss"], (got["loss"], got3["loss"])
    assert G.differing(got["all"], got3["all"], sorted(got["all"])) == []
    assert G.differing(got["all"], G.snapshot(G.make(c, built), "darc"), G.owned(c)) == G.owned(c)          # everything owned has moved


@pytest.mark.parametrize("c", _da(K.EDGE_CASES), ids=K.case_id)
def test_hyper_parameter_edges_against_float64(c):
    G.check_hyper_parameter_edge(c)


@pytest.mark.parametrize("B,seed,draw", K.NOISE_PARAMS)
def test_in_kernel_noise_equals_the_host_restatement(B, seed, draw):
    G.check_in_kernel_noise("datd3", B, seed, draw)
