"""The fused TD3 update (armenv_td3_update through armenv.fused_td3.FusedTD3) on cuda:0 against the float64 restatement of
tests/learner_ref64.py, with tolerances derived from f32 rounding: per element, |g_hip - g_ref| <= C 2^-24 M_ref + allowance_ref,
where M is the contraction chain over absolute values and the allowance is what flows through relu units within rounding of zero.

The gradient the kernel applied is read exactly: with betas = (0, 0.999), Adam's first moment after the update IS the gradient.
Each stage is compared on its own (teacher forcing): the actor's gradient through the kernel's own stepped critic, the Adam steps
fed the kernel's own gradient.  Every input is a TD3 case of tests/learner_cases.py, built on the CPU and moved to the device
(tests/test_td3_ref64.py checks the same inputs for ambiguity without a GPU); the harness, the C table and the bodies that
tests/test_gpu_da_ref64.py holds too are tests/learner_ref64_gpu.py's (profiles/learner_ref64_errors.txt records the largest measured
ratios over all four agents)."""
import pytest
import torch

pytest.register_assert_rewrite("learner_ref64_gpu")          # the shared bodies assert there
import learner_cases as K  # noqa: E402
import learner_ref64_gpu as G  # noqa: E402
from learner_gpu import DEV  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    G.write_ratios()


@pytest.mark.parametrize("with_actor", [True, False])
@pytest.mark.parametrize("B,D", K.TD3_GRAD_SHAPES)
def test_gradients_and_loss_against_float64(B, D, with_actor):
    """All 12 critic and (with the actor step) 6 actor gradients and the loss, element by element, within C 2^-24 M + allowance;
    without the actor step (a policy_freq that never fires) the actor, both targets and the actor's moments are bitwise unchanged."""
    c = K.grad_case("td3", None, B, D, with_actor=with_actor)
    assert any(K.case_id(c) == K.case_id(x) for x in K.GRAD_CASES)
    G.against_float64(c)


def test_largest_batch_against_float64():
    """B = 2^20 (kMaxBatch): 4096 weight-gradient partials added in sequence, the loss block's threads adding 4096 rows each."""
    from armenv import _lib as L
    c = K.LARGEST_CASE
    need = L.load().armenv_td3_workspace_bytes(c["D"], 256, c["B"])
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    extra = 6 << 30                                   # batch, reference chunks, allocator slack
    if free < need + extra:
        pytest.skip("B = 2^20 needs %d bytes of device memory (workspace %d + %d); %d are free" % (need + extra, need, extra, free))
    G.against_float64(c, release=True)


@pytest.mark.parametrize("B", [65, 257, 2048])
def test_every_defect_fails_a_gpu_comparison(B):
    G.check_every_defect_fails(next(c for c in K.DEFECT_CASES if c["agent"] == "td3" and c["B"] == B))


@pytest.mark.parametrize("step", K.ADAM_STEPS)
def test_adam_and_soft_update_against_float64(step):
    G.check_adam_and_soft_update("td3", None, step)


def test_lr_zero_and_tau_edges_are_exact():
    G.check_lr_zero_and_tau_edges("td3", None)


def test_with_every_done_set_no_target_net_is_read():
    G.check_every_done_set("td3", None)


@pytest.mark.parametrize("case", ["dones_all_1", "dones_all_0", "gamma_0", "gamma_1", "clamp_binds"])
def test_hyper_parameter_edges_against_float64(case):
    G.check_hyper_parameter_edge(next(c for c in K.edge_cases("td3", None) if c["tag"] == "edge-" + case))


def test_noise_clip_zero_equals_no_noise_bit_for_bit():
    G.check_noise_clip_zero_equals_no_noise("td3", None)


@pytest.mark.parametrize("B,seed,draw", K.NOISE_PARAMS)
def test_in_kernel_noise_equals_the_host_restatement(B, seed, draw):
    G.check_in_kernel_noise("td3", B, seed, draw)


def test_update_on_a_side_stream_is_bitwise_equal():
    """B = 2048 with the in-kernel noise and default betas: the update on a side stream equals the one on the default stream"""
    c = K.grad_case("td3", None, 2048, 6)
    built = K.build(c)
    f, g = G.make(c, built, beta1=0.9, seed=3), G.make(c, built, beta1=0.9, seed=3)
    got_default = G.update(f, c, built, noise=None)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got_side = G.update(g, c, built, noise=None)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    assert got_side["loss"] == got_default["loss"]
    assert G.differing(got_side["all"], got_default["all"], sorted(got_default["all"])) == []
    assert G.differing(got_default["all"], G.snapshot(G.make(c, built), "td3"), G.owned(c)) == G.owned(c)       # everything has moved
