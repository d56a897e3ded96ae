"""CPU tests of tests/da_ref64.py, the float64 restatements of one DADDPG, DATD3 and DARC update that the fused HIP updates are tested
against: they reproduce the reference's recorded runs (G16, G17, G18), equal torch autograd in float64 over armenv.daddpg.DADDPG and
armenv.datd3.DATD3 / DARC for both parities, every defect switch breaks that equality under hyper-parameters that make it bind, and
every case of tests/test_gpu_da_ref64.py (tests/da_cases.py) keeps its share of ambiguous relu units under the cap."""
import numpy as np
import pytest
import torch

from conftest import golden_npz
import da_cases as K
import da_ref64 as R
from datd3_golden import KEYS, expected_losses, load_train_fixture
from td3_ref64 import adam_state, random_batch

HP_GOLDEN = dict(K.HP, beta1=0.9)
# against autograd: a q_weight whose 1 - q_weight is an f32 value, so that the kernel's two f32 weights ARE the torch learner's
HP = dict(HP_GOLDEN, q_weight=0.25)
# an f32 gradient of the torch learner on the CPU against the float64 one, in units of 2^-24 M: M carries the magnitudes through the
# whole chain, so each rounding anywhere in it moves an element by at most 2^-24 M; six contractions, each summed in blocks (a few
# roundings deep at these widths), stay under 8 of them
C_TORCH = 8.0
TOL = 1e-12 / R.U               # 1e-12 of a quantity's magnitude, in bad_elements' units of 2^-24


def _zeros(agent, learner):
    nets = {n: getattr(learner, n) for n in R.NETS[agent]}
    moments = {n: ([torch.zeros_like(p) for p in nets[n].parameters()],) * 2 for n in R.LEARNING[agent]}
    return R.state_from(agent, nets, moments, {n: 0 for n in R.LEARNING[agent]})


def _assert_golden_nets(agent, st, g, flipped=()):
    """every element within 1e-5 of the recorded parameters; the nets `flipped`: within 7e-3 (see the DATD3 test)"""
    for name in R.NETS[agent]:
        for suffix, v in zip(("fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias", "fc3_weight", "fc3_bias"), st[name]):
            ref = g[f"{name}__{suffix}"]
            assert np.abs(v.numpy() - ref).max() < (7e-3 if name in flipped else 1e-5), (name, suffix, np.abs(v.numpy() - ref).max())


def test_daddpg_reference_reproduces_the_golden_updates():
    """G16: the eight DADDPG_MLP.update calls of tests/golden/daddpg_train_seed0.npz (B = 64) from torch.manual_seed(0)'s initial
    weights, update n stepping actor 1 when n is even: the tolerances of test_reference_reproduces_the_golden_updates."""
    from armenv.daddpg import DADDPG
    g = golden_npz("daddpg_train_seed0.npz")
    torch.manual_seed(0)
    st = _zeros("daddpg", DADDPG(6, 3, 0.7, device="cpu"))
    for i, want in enumerate(g["losses"]):
        b = {k: torch.from_numpy(g[f"b{i}_{k}"]).to(torch.float64) for k in KEYS}
        a1 = (i + 1) % 2 == 0
        out = R.daddpg_update(st, b, HP_GOLDEN, a1)
        assert abs(out["loss"] - want) < 1e-5 * max(1.0, abs(want)), (i, out["loss"], want)
        st = R.advance(st, out, "critic", soft_critic=not a1)
    assert (st["critic_step"], st["actor1_step"], st["actor2_step"]) == (8, 4, 4)
    _assert_golden_nets("daddpg", st, g)


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
    st = _zeros(agent, t)
    want = expected_losses(g, darc)
    flips = []
    for i in range(4):
        b32 = {k: torch.from_numpy(g[f"b{i}_{k}"]) for k in KEYS}
        b = {k: v.to(torch.float64) for k, v in b32.items()}
        for k in (1, 2):
            n32 = torch.from_numpy(g["noise"][2 * i + k - 1])
            out = R.datd3_update(st, b, n32.to(torch.float64), HP_GOLDEN, k, darc)
            w = want[2 * i + k - 1]
            assert abs(out["loss"] - w) < 1e-5 * max(1.0, abs(w)), (i, k, out["loss"], w)
            st = R.advance(st, out, "critic%d" % k)
            if not darc and not flips:                 # the f32 learner beside the reference, until their states part
                t.update(b32, k == 1, n32)
                g32 = [p.grad.to(torch.float64) for p in getattr(t, "actor%d" % k).parameters()]
                quad = list(zip(g32, out["actor_grad"], out["actor_grad_mag"], out["actor_grad_allow"]))
                assert sum(R.bad_elements(x, y, m, a, C_TORCH)[0] for x, y, m, a in quad) == 0, (i, k)
                if sum(R.bad_elements(x, y, m, torch.zeros_like(a), C_TORCH)[0] for x, y, m, a in quad):
                    flips.append((i, k))
    assert all(st[n + "_step"] == 4 for n in R.LEARNING[agent])
    assert flips == ([] if darc else [(1, 2)])
    _assert_golden_nets(agent, st, g, flipped=() if darc else ("actor2", "target_actor2"))


# ---- equality with float64 autograd ----

def _torch_state(agent, t):
    adam = {name: adam_state(getattr(t, name), getattr(t, name + "_opt")) for name in R.LEARNING[agent]}
    return R.state_from(agent, {n: getattr(t, n) for n in R.NETS[agent]}, {n: mvs[:2] for n, mvs in adam.items()},
                        {n: mvs[2] for n, mvs in adam.items()})


_AUTOGRAD = {}


def _autograd_case(agent, B, D, k, seed, hp, gain=1.0):
    """The torch learner's networks and Adam in float64 (torch autograd), two priming updates (k = 1, then k = 2), then update k.
    Returns (state before it, batch, noise, state after it, the gradients the update applied, its critic loss).  `gain` scales the
    target actors' last layers (pre-tanh outputs of order one, so that target actions reach the clamp)."""
    key = (agent, B, D, k, seed, tuple(sorted(hp.items())), gain)
    if key in _AUTOGRAD:
        return _AUTOGRAD[key]
    from armenv.daddpg import DADDPG
    from armenv.datd3 import DARC, DATD3
    torch.manual_seed(seed)
    kw = dict(device="cpu", actor_lr=hp["actor_lr"], critic_lr=hp["critic_lr"], tau=hp["tau"], gamma=hp["gamma"])
    if agent == "daddpg":
        t = DADDPG(D, 3, hp["action_bound"], **kw)
    else:
        kw.update(policy_noise=hp["policy_noise"], noise_clip=hp["noise_clip"])
        if agent == "darc":
            kw.update(q_weight=hp["q_weight"], regularization_weight=hp["regularization_weight"])
        t = (DARC if agent == "darc" else DATD3)(D, 3, hp["action_bound"], **kw)
    for n in t._nets():
        n.double()
    with torch.no_grad():
        t.target_actor1.fc3.weight.mul_(gain)
        t.target_actor2.fc3.weight.mul_(gain)
        if gain != 1.0 and agent != "daddpg":              # twin target critics: the min picks either proposal on many rows
            for p2, p1 in zip(t.target_critic2.parameters(), t.target_critic1.parameters()):
                p2.copy_(p1 * (1 + 0.02 * torch.randn(p1.shape, dtype=p1.dtype)))
    gen = torch.Generator().manual_seed(seed + 1)

    def update(batch, noise, kk):
        args = (batch["states"], batch["actions"], batch["rewards"].view(-1, 1), batch["next_states"], batch["dones"].view(-1, 1), kk == 1)
        return float(t._update(*args) if agent == "daddpg" else t._update(*args, noise))
    for kk in (1, 2):
        update(random_batch(gen, B, D), torch.randn(B, 3, generator=gen, dtype=torch.float64), kk)
    st = _torch_state(agent, t)
    assert all(st[n + "_step"] == 1 for n in R.LEARNING[agent] if n != "critic") and st.get("critic_step", 2) == 2
    batch, noise = random_batch(gen, B, D), torch.randn(B, 3, generator=gen, dtype=torch.float64)
    loss = float(update(batch, noise, k))
    after = _torch_state(agent, t)
    grads = {n: [p.grad.detach().clone() for p in getattr(t, n).parameters()] for n in R.LEARNING[agent]}
    _AUTOGRAD[key] = (st, batch, noise, after, grads, loss)
    return _AUTOGRAD[key]


def _reference(agent, st, batch, noise, hp, k, **kw):
    if agent == "daddpg":
        return R.daddpg_update(st, batch, hp, k == 1, **kw)
    return R.datd3_update(st, batch, noise, hp, k, agent == "darc", **kw)


def _autograd_failures(agent, k, out, after, grads, loss, forced=None):
    """names of the quantities of `out` that differ from the float64 autograd learner by more than 1e-12 of their magnitude (plus
    the allowance): the loss, gradients, stepped parameters and targets, and from `forced` (the reference fed autograd's gradients:
    a moment's magnitude b1 |m| + (1 - b1) |g| says nothing about a gradient that was itself summed from larger terms) both moments"""
    bad = []
    if abs(out["loss"] - loss) > 1e-12 * out["loss_mag"]:
        bad.append("loss")
    critic = "critic" if agent == "daddpg" else "critic%d" % k
    for generic, net in (("critic", critic), ("actor", "actor%d" % k)):
        quantities = [(generic + "_grad", grads[net], out[generic + "_grad_mag"], out[generic + "_grad_allow"])]
        quantities += [(generic, after[net], out[generic + "_mag"], None),
                       ("target_" + generic, after["target_" + net], out["target_" + generic + "_mag"], None)]
        for name, want, mag, allow in quantities:
            for i, w in enumerate(want):
                if R.bad_elements(w, out[name][i], mag[i], torch.zeros_like(w) if allow is None else allow[i], TOL)[0]:
                    bad.append("%s%d" % (name, i))
        for name in ((generic, generic + "_m", generic + "_v") if forced is not None else ()):
            for i, w in enumerate(after[net + name[len(generic):]]):
                if R.bad_elements(w, forced[name][i], forced[name + "_mag"][i], torch.zeros_like(w), TOL)[0]:
                    bad.append("forced %s%d" % (name, i))
    return bad


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("B,D", [(B, D) for B in (1, 5, 257) for D in (1, 6, 9)])
@pytest.mark.parametrize("agent", K.AGENTS)
def test_reference_equals_autograd_in_float64(agent, B, D, k):
    """Loss, gradients, Adam-stepped parameters, moments and targets equal those of the torch learner's update run in float64 with
    torch autograd and torch.optim.Adam, from primed (non-zero) Adam moments, to 1e-12 of their magnitudes -- for both parities of
    DADDPG and both k of DATD3 / DARC; what the update does not own is returned as it was."""
    st, batch, noise, after, grads, loss = _autograd_case(agent, B, D, k, 7 * B + D, HP)
    out = _reference(agent, st, batch, noise, HP, k, chunk=64)           # several chunks at B = 257
    critic = "critic" if agent == "daddpg" else "critic%d" % k
    forced = _reference(agent, st, batch, noise, HP, k, critic_grad=grads[critic], actor_grad=grads["actor%d" % k])
    assert _autograd_failures(agent, k, out, after, grads, loss, forced) == []
    assert out["ambiguous"] < 1e-3 * out["units"]
    if agent == "daddpg" and k == 1:                                     # update 1 leaves the target critic alone
        assert all(torch.equal(a, b) for a, b in zip(out["target_critic"], st["target_critic"]))
        assert all(torch.equal(a, b) for a, b in zip(after["target_critic"], st["target_critic"]))


HP_DEFECT = dict(HP, **K.HP_DEFECT)


@pytest.mark.parametrize("agent,defect", [(a, d) for a in K.AGENTS for d in R.DEFECTS[a]])
def test_every_defect_switch_breaks_the_autograd_comparison(agent, defect):
    """For both k: the undefective reference equals autograd, the defective one does not.  The switches bind: a third of the rows is
    terminal, the noise clip changes more than half the noise elements, the clamp more than a third of both target actions (a saturated action
    is pushed over the bound by noise of its own sign only, so a half is the ceiling), the two values
    under the min differ, and the regulariser is of the TD term's order."""
    for k in (1, 2):
        st, batch, noise, after, grads, loss = _autograd_case(agent, 257, 6, k, 4, HP_DEFECT, gain=100.0)
        good = _reference(agent, st, batch, noise, HP_DEFECT, k)
        assert _autograd_failures(agent, k, good, after, grads, loss) == []
        assert 0.2 < float(batch["dones"].mean()) < 0.5
        assert 0.1 < K.pick_share(agent, st, batch, noise, HP_DEFECT) < 0.9
        if agent != "daddpg":
            assert float(((noise * HP_DEFECT["policy_noise"]).abs() > HP_DEFECT["noise_clip"]).double().mean()) > 0.5
            for a, raw in zip(K.target_actions(st, batch, noise, HP_DEFECT), K.target_actions(st, batch, noise, HP_DEFECT, clamp=False)):
                assert float((a != raw).double().mean()) > 1 / 3
        if agent == "darc":
            td = R.datd3_update(st, batch, noise, HP_DEFECT, k, True, defect="no_regulariser", with_actor=False)["loss"]
            assert 0.1 * td < good["loss"] - td < 10 * td, (td, good["loss"])
        bad = _autograd_failures(agent, k, _reference(agent, st, batch, noise, HP_DEFECT, k, defect=defect), after, grads, loss)
        assert bad, (defect, k)


def test_defect_lists():
    """the eight common defects, three for DADDPG, four more for DATD3 and four more again for DARC"""
    assert len(R.COMMON_DEFECTS) == 8 and len(set(R.DARC_DEFECTS)) == 16 and len(set(R.DADDPG_DEFECTS)) == 11
    assert set(R.DATD3_DEFECTS) < set(R.DARC_DEFECTS) and len(R.DATD3_DEFECTS) == 12
    with pytest.raises(AssertionError):
        K.reference(K.GRAD_CASES[0], K.build(K.GRAD_CASES[0]), defect="no_noise_clip")      # a DADDPG case: it has no noise


def test_mix_weights_are_the_two_f32_values_of_the_kernel():
    w_min, w_max = R.mix_weights(dict(q_weight=float(np.float32(0.2))))
    assert w_min == float(np.float32(0.2)) and w_max == float(np.float32(1.0 - float(np.float32(0.2))))
    assert w_min + w_max != 1.0 and abs(w_min + w_max - 1.0) < 2.0 ** -24         # the mix is not the identity, to rounding only
    assert R.mix_weights(dict(q_weight=0.0)) == (0.0, 1.0) and R.mix_weights(dict(q_weight=1.0)) == (1.0, 0.0)


# ---- the GPU tests' inputs ----

def test_gpu_cases_are_distinct_and_cover_the_issue():
    ids = [K.case_id(c) for c in K.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert len(K.GRAD_CASES) == 6 * 22 and {(c["B"], c["D"]) for c in K.GRAD_CASES} == set(K.GRAD_SHAPES)
    assert max(c["B"] for c in K.ALL_CASES) == 4097


@pytest.mark.parametrize("c", K.ALL_CASES, ids=K.case_id)
def test_gpu_case_inputs_keep_ambiguity_rare(c):
    """the reference on exactly the inputs that the GPU test of this case moves to the device: at most AMB_MAX of the relu units
    are within rounding of zero, so that the allowance cannot make the comparison vacuous; the inputs are f32 values"""
    built = K.build(c)
    assert all(t.dtype == torch.float32 for ts in built["nets"].values() for t in ts)
    out = K.reference(c, built, with_actor=True) if c["agent"] != "daddpg" else K.reference(c, built)
    assert out["units"] > 0 and out["ambiguous"] <= K.AMB_MAX * out["units"], (out["ambiguous"], out["units"])
    assert all(bool(torch.isfinite(t).all()) for t in out["critic_grad"] + out["actor_grad"])
    if c["tag"] == "edge-clamp_binds":
        st, b, n = K.state64(c, built), K.batch64(built), K.noise64(built)
        assert all(float((a.abs() == c["hp"]["action_bound"]).double().mean()) > 0.5 for a in K.target_actions(st, b, n, c["hp"]))
    if c["tag"] == "edge-dones_all_1":
        assert torch.equal(out["target"], K.batch64(built)["rewards"])
