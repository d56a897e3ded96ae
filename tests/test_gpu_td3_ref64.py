"""The fused TD3 update (armenv_td3_update through armenv.fused_td3.FusedTD3) on cuda:0 against the float64 restatement of
tests/td3_ref64.py, with tolerances derived from f32 rounding: per element, |g_hip - g_ref| <= C 2^-24 M_ref + allowance_ref, where
M is the contraction chain over absolute values and the allowance is what flows through relu units within rounding of zero.

The gradient the kernel applied is read exactly: with betas = (0, 0.999), Adam's first moment after the update IS the gradient.
Each stage is compared on its own (teacher forcing): the actor's gradient through the kernel's own stepped critic, the Adam steps
fed the kernel's own gradient.  C is one constant per kind of quantity, calibrated on the MI355X (profiles/td3_fused_ref64_errors.txt
records the largest measured ratios; each C is at most 8x the largest)."""
import os

import numpy as np
import pytest
import torch

import td3_ref64 as R
from learner_gpu import DEV, Bounds, f64 as _f64

pytestmark = pytest.mark.gpu
NOISE_C = 0.015
U = R.U
C = dict(critic_grad=1.0, actor_grad=0.5, loss=0.05, adam=16.0, noise=NOISE_C)
AMB_MAX = 1e-3                   # at most this fraction of relu units may be ambiguous, or the allowance would make the test vacuous
NO_ACTOR = 1 << 40               # a policy_freq under which no update takes the actor step
BOUNDS = Bounds(C, AMB_MAX)
_check, _grad_failures, _adam_failures = BOUNDS.check, BOUNDS.grad_failures, BOUNDS.adam_failures
_ambiguity_is_rare = BOUNDS.ambiguity_is_rare


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    """ARMENV_TD3_REF64_RATIOS=<path>: write the largest measured ratio per kind and case there (calibration of C)"""
    yield
    BOUNDS.write(os.environ.get("ARMENV_TD3_REF64_RATIOS"))


def _f32(x):
    return float(np.float32(x))


def _hp(**kw):
    hp = dict(action_bound=0.7, gamma=0.98, tau=0.005, policy_noise=0.2, noise_clip=0.5, actor_lr=1e-3, critic_lr=1e-3, beta1=0.0,
              beta2=0.999, eps=1e-8)
    hp.update(kw)
    return {k: _f32(v) for k, v in hp.items()}      # the values the kernel sees


def _make(D, hp, seed=0, policy_freq=1, steps=(3, 3), noise_seed=0, target_actor_gain=1.0):
    """a FusedTD3 with every hyper-parameter of `hp` set before its first update, targets that differ from the networks, non-zero
    Adam moments and the given (critic, actor) step counters"""
    from armenv.fused_td3 import FusedTD3
    torch.manual_seed(seed)
    f = FusedTD3(D, 3, hp["action_bound"], actor_lr=hp["actor_lr"], critic_lr=hp["critic_lr"], tau=hp["tau"], gamma=hp["gamma"],
                 policy_noise=hp["policy_noise"], noise_clip=hp["noise_clip"], policy_freq=policy_freq, device=DEV, seed=noise_seed)
    f.betas, f.eps = (hp["beta1"], hp["beta2"]), hp["eps"]
    g = torch.Generator(device=DEV).manual_seed(seed + 1000)
    with torch.no_grad():
        for tn in (f.target_actor, f.target_critic):
            for p in tn.parameters():
                p.add_(torch.randn(p.shape, device=DEV, generator=g) * 0.02 * p.abs().mean())
        f.target_actor.fc3.weight.mul_(target_actor_gain)
        for m, v in zip(f.critic_m + f.actor_m, f.critic_v + f.actor_v):
            m.copy_(torch.randn(m.shape, device=DEV, generator=g) * 1e-3)
            v.copy_(torch.rand(v.shape, device=DEV, generator=g) * 1e-6)
    f.critic_step, f.actor_step = steps
    return f


def _clone(f, D, hp, **kw):
    """a second learner with f's exact state (parameters, moments, counters)"""
    g = _make(D, hp, **kw)
    with torch.no_grad():
        for a, b in zip([p for n in g._nets() for p in n.parameters()] + g.critic_m + g.critic_v + g.actor_m + g.actor_v,
                        [p for n in f._nets() for p in n.parameters()] + f.critic_m + f.critic_v + f.actor_m + f.actor_v):
            a.copy_(b)
    g.critic_step, g.actor_step, g.total_it = f.critic_step, f.actor_step, f.total_it
    return g


def _batch(B, D, seed, done_p=0.1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return dict(states=torch.rand(B, D, device=DEV, generator=g), actions=torch.rand(B, 3, device=DEV, generator=g) * 1.4 - 0.7,
                next_states=torch.rand(B, D, device=DEV, generator=g), rewards=torch.rand(B, device=DEV, generator=g) - 0.5,
                dones=(torch.rand(B, device=DEV, generator=g) < done_p).to(torch.uint8))


def _b64(batch):
    return {k: v.to(torch.float64) for k, v in batch.items()}


def _state(f):
    return R.state_from(f.actor, f.critic, f.target_actor, f.target_critic, f.actor_m, f.actor_v, f.critic_m, f.critic_v,
                        f.actor_step, f.critic_step, device=DEV)


def _kernel_update(f, batch, noise):
    """one fused update; returns (state before, with_actor, loss, the kernel's outputs in float64)"""
    st = _state(f)
    with_actor = (f.total_it + 1) % f.policy_freq == 0
    loss = float(f.train(batch, noise=noise))
    got = dict(loss=loss, critic=_f64(f.critic), critic_m=_f64(f.critic_m), critic_v=_f64(f.critic_v),
               target_critic=_f64(f.target_critic), actor=_f64(f.actor), actor_m=_f64(f.actor_m), actor_v=_f64(f.actor_v),
               target_actor=_f64(f.target_actor))
    return st, with_actor, loss, got


GRAD_SHAPES = [(B, 6) for B in (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 1000, 2048, 4097, 65536)] + \
              [(B, D) for D in (1, 3, 9, 12) for B in (257, 2048)]


@pytest.mark.parametrize("with_actor", [True, False])
@pytest.mark.parametrize("B,D", GRAD_SHAPES)
def test_gradients_and_loss_against_float64(B, D, with_actor):
    """All 12 critic and (with the actor step) 6 actor gradients and the loss, element by element, within C 2^-24 M + allowance."""
    hp = _hp()
    f = _make(D, hp, seed=B + D, policy_freq=1 if with_actor else NO_ACTOR)
    batch = _batch(B, D, seed=7 * B + D)
    noise = torch.randn(B, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B))
    st, wa, _, got = _kernel_update(f, batch, noise)
    assert wa == with_actor
    out = R.td3_update(st, _b64(batch), noise.to(torch.float64), hp, with_actor, stepped_critic=got["critic"])
    _ambiguity_is_rare(out)
    assert _grad_failures("B=%d D=%d" % (B, D), got, out, with_actor) == []


def test_largest_batch_against_float64():
    """B = 2^20 (kMaxBatch): 4096 weight-gradient partials added in sequence, the loss block's threads adding 4096 rows each."""
    from armenv import _lib as L
    B, D = 1 << 20, 6
    need = L.load().armenv_td3_workspace_bytes(D, 256, B)
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    extra = 6 << 30                                   # batch, reference chunks, allocator slack
    if free < need + extra:
        pytest.skip("B = 2^20 needs %d bytes of device memory (workspace %d + %d); %d are free" % (need + extra, need, extra, free))
    hp = _hp()
    f = _make(D, hp, seed=20)
    batch = _batch(B, D, seed=20)
    noise = torch.randn(B, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(20))
    st, wa, _, got = _kernel_update(f, batch, noise)
    f._ws = None
    torch.cuda.empty_cache()
    out = R.td3_update(st, _b64(batch), noise.to(torch.float64), hp, True, stepped_critic=got["critic"])
    _ambiguity_is_rare(out)
    assert _grad_failures("B=2^20 D=6", got, out, True) == []


# hyper-parameters under which every defect of td3_ref64.DEFECTS changes something: noise clip and action clamp bind on many
# elements (target actions of order one through target_actor_gain), and a third of the rows are terminal
HP_DEFECT = dict(action_bound=0.25, policy_noise=0.4, noise_clip=0.1)


@pytest.mark.parametrize("B", [65, 257, 2048])
def test_every_defect_fails_a_gpu_comparison(B):
    hp = _hp(**HP_DEFECT)
    f = _make(6, hp, seed=B, target_actor_gain=30.0, steps=(0, 0))
    batch = _batch(B, 6, seed=B, done_p=0.3)
    noise = torch.randn(B, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B + 1))
    st, wa, _, got = _kernel_update(f, batch, noise)
    b64, n64 = _b64(batch), noise.to(torch.float64)

    def failures(defect):
        out = R.td3_update(st, b64, n64, hp, True, stepped_critic=got["critic"], critic_grad=got["critic_m"],
                           actor_grad=got["actor_m"], defect=defect)
        rec = defect is None
        return _grad_failures("defects B=%d" % B, got, out, True, record=rec) + _adam_failures("defects B=%d" % B, got, out, True,
                                                                                               record=rec)
    assert failures(None) == []
    for defect in R.DEFECTS:
        assert failures(defect), defect


@pytest.mark.parametrize("step", [1, 2, 10, 10 ** 6])
def test_adam_and_soft_update_against_float64(step):
    """Default betas.  The float64 Adam takes the kernel's own gradient, read from a beta1 = 0 twin of the same state: the critic's
    (its gradient does not depend on the betas), then the actor's with critic_lr = 0 (so that both twins' actor losses see the same
    critic).  Parameters, moments and targets within C_adam 2^-24 of |p| + |step| (and of the moments' own magnitudes)."""
    B, D = 257, 6
    batch = _batch(B, D, seed=step % 1000)
    noise = torch.randn(B, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    for side, kw in (("critic", {}), ("actor", dict(critic_lr=0.0))):
        hp, hp0 = _hp(beta1=0.9, **kw), _hp(**kw)
        f = _make(D, hp, seed=step % 997, steps=(step - 1, step - 1))
        f0 = _clone(f, D, hp0, seed=step % 997, steps=(step - 1, step - 1))
        st, _, _, got = _kernel_update(f, batch, noise)
        _, _, _, got0 = _kernel_update(f0, batch, noise)
        out = R.td3_update(st, _b64(batch), noise.to(torch.float64), hp, True, critic_grad=got0["critic_m"], actor_grad=got0["actor_m"])
        assert _adam_failures("step=%d" % step, got, out, True, sides=(side,)) == [], side
        if side == "actor":                                  # critic_lr = 0: the critic did not move, bit for bit
            assert all(torch.equal(a, b) for a, b in zip(got["critic"], st["critic"]))


def test_lr_zero_and_tau_edges_are_exact():
    """lr = 0 leaves every parameter unchanged; tau = 0 leaves the targets unchanged; tau = 1 makes them equal the parameters."""
    B, D = 65, 6
    batch = _batch(B, D, seed=1)
    noise = torch.randn(B, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    f = _make(D, _hp(actor_lr=0.0, critic_lr=0.0, beta1=0.9))
    st, _, _, got = _kernel_update(f, batch, noise)
    for name in ("actor", "critic"):
        assert all(torch.equal(a, b) for a, b in zip(got[name], st[name])), name
    f = _make(D, _hp(tau=0.0, beta1=0.9))
    st, _, _, got = _kernel_update(f, batch, noise)
    for name in ("target_actor", "target_critic"):
        assert all(torch.equal(a, b) for a, b in zip(got[name], st[name])), name
    f = _make(D, _hp(tau=1.0, beta1=0.9))
    st, _, _, got = _kernel_update(f, batch, noise)
    assert not all(torch.equal(a, b) for a, b in zip(got["critic"], st["critic"]))
    for name in ("actor", "critic"):
        assert all(torch.equal(a, b) for a, b in zip(got["target_" + name], got[name])), name


@pytest.mark.parametrize("case", ["dones_all_1", "dones_all_0", "gamma_0", "gamma_1", "clamp_binds"])
def test_hyper_parameter_edges_against_float64(case):
    B, D = 257, 6
    hp = _hp(**{"gamma_0": dict(gamma=0.0), "gamma_1": dict(gamma=1.0), "clamp_binds": dict(action_bound=0.05)}.get(case, {}))
    batch = _batch(B, D, seed=11)
    if case.startswith("dones"):
        batch["dones"].fill_(1 if case == "dones_all_1" else 0)
    noise = torch.randn(B, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    f = _make(D, hp, seed=11)
    f_other = _clone(f, D, hp, seed=11)
    st, _, _, got = _kernel_update(f, batch, noise)
    out = R.td3_update(st, _b64(batch), noise.to(torch.float64), hp, True, stepped_critic=got["critic"])
    assert _grad_failures("edge " + case, got, out, True) == []
    if case == "clamp_binds":                             # the clamp really binds on most target actions
        a2 = _target_action(st, _b64(batch), noise.to(torch.float64), hp)
        assert float((a2.abs() == hp["action_bound"]).double().mean()) > 0.5
    if case == "dones_all_1":
        assert torch.equal(out["target"], _b64(batch)["rewards"])
        # other target networks: the critic's gradient, its stepped parameters and the loss do not change, bit for bit
        with torch.no_grad():
            for p in list(f_other.target_critic.parameters()) + list(f_other.target_actor.parameters()):
                p.mul_(-3.0).add_(0.25)
        _, _, _, got2 = _kernel_update(f_other, batch, noise)
        assert got2["loss"] == got["loss"]
        for name in ("critic", "critic_m", "critic_v"):
            assert all(torch.equal(a, b) for a, b in zip(got2[name], got[name])), name


def _target_action(st, b, noise, hp):
    TA = st["target_actor"]
    h = torch.relu(torch.relu(b["next_states"] @ TA[0].T + TA[1]) @ TA[2].T + TA[3])
    a = hp["action_bound"] * torch.tanh(h @ TA[4].T + TA[5]) + (noise * hp["policy_noise"]).clamp(-hp["noise_clip"], hp["noise_clip"])
    return a.clamp(-hp["action_bound"], hp["action_bound"])


def test_noise_clip_zero_equals_no_noise_bit_for_bit():
    B, D = 257, 6
    batch = _batch(B, D, seed=4)
    noise = torch.randn(B, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    got = []
    for kw in (dict(noise_clip=0.0), dict(policy_noise=0.0)):
        _, _, _, g = _kernel_update(_make(D, _hp(**kw), seed=4), batch, noise)
        got.append(g)
    assert got[0]["loss"] == got[1]["loss"]
    for name in ("critic", "critic_m", "actor", "actor_m", "target_critic", "target_actor"):
        assert all(torch.equal(a, b) for a, b in zip(got[0][name], got[1][name])), name


# the noise reaches a2 unclipped and unclamped: |z| <= sqrt(-2 ln 2^-24) = 5.8, so |noise| <= 2.9 < noise_clip, and
# |bound tanh(u) + noise| < bound for the small u of a fresh target actor
HP_NOISE = dict(action_bound=8.0, policy_noise=0.5, noise_clip=5.0)


@pytest.mark.parametrize("draw", [1, (1 << 32) + 1])
@pytest.mark.parametrize("seed", [0, (1 << 32) + 5])
@pytest.mark.parametrize("B", [1, 65, 2048])
def test_in_kernel_noise_equals_the_host_restatement(B, seed, draw):
    """train(batch) with the in-kernel Philox noise against train(batch, noise=td3_ref64.kernel_noise(...)) from the same state.
    The critic's gradients and the loss may differ by C_noise 2^-24 (S + M): S, the root-sum-square sensitivity to a noise change of
    one f32 rounding of the Box-Muller radius per element (td3_ref64.noise_sensitivity), and M, the magnitude that bounds the f32
    rounding of the update itself.  State feature 0 is zero except on row B // 2, so that the column of the fc1 weight gradients that
    it feeds is that row's alone.  Controls: the previous draw's noise, and row B // 2's noise moved by 1e-3, both fail the bound."""
    D, hp = 6, _hp(**HP_NOISE)
    batch = _batch(B, D, seed=B, done_p=0.0)
    batch["states"][:, 0] = 0.0
    batch["states"][B // 2, 0] = 1.0
    z, radius = R.kernel_noise(seed, draw, np.arange(B), with_radius=True)
    host = torch.from_numpy(z).to(DEV)

    def run(noise):
        f = _make(D, hp, seed=B, policy_freq=NO_ACTOR, noise_seed=seed)
        f.total_it = draw - 1
        st, wa, _, got = _kernel_update(f, batch, noise if noise is None else noise.to(torch.float32))
        assert not wa
        return st, got
    st, got_k = run(None)
    _, got_h = run(host)
    b64 = _b64(batch)
    sens, lsens = R.noise_sensitivity(st, b64, host, torch.from_numpy(radius).to(DEV), hp)
    out = R.td3_update(st, b64, host, hp, False)

    def beyond(got, record):
        n = 0
        for k in range(12):
            n += _check("noise", "B=%d" % B, got["critic_m"][k], got_k["critic_m"][k], sens[k] + out["critic_grad_mag"][k],
                        record=record)
        lt = lambda x: torch.tensor([x], dtype=torch.float64)
        n += _check("noise", "B=%d loss" % B, lt(got["loss"]), lt(got_k["loss"]), lt(lsens + out["loss_mag"]), record=record)
        return n
    assert beyond(got_h, True) == 0
    prev = torch.from_numpy(R.kernel_noise(seed, draw - 1, np.arange(B))).to(DEV)
    assert beyond(run(prev)[1], False) > 0
    moved = host.clone()
    moved[B // 2] += 1e-3
    assert beyond(run(moved)[1], False) > 0


def test_update_on_a_side_stream_is_bitwise_equal():
    B, D = 2048, 6
    hp = _hp(beta1=0.9)
    batch = _batch(B, D, seed=9)
    f = _make(D, hp, seed=9, noise_seed=3)
    g = _clone(f, D, hp, seed=9, noise_seed=3)
    _, _, _, got_default = _kernel_update(f, batch, None)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        loss = g.train(batch)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    assert float(loss) == got_default["loss"]
    for name, xs in (("critic", g.critic), ("actor", g.actor), ("target_critic", g.target_critic), ("target_actor", g.target_actor),
                     ("critic_m", g.critic_m), ("critic_v", g.critic_v), ("actor_m", g.actor_m), ("actor_v", g.actor_v)):
        assert all(torch.equal(a, b) for a, b in zip(_f64(xs), got_default[name])), name
