"""What tests/test_td3_ref64.py and tests/test_da_ref64.py share (test infrastructure): the float64 autograd learners that
tests/learner_ref64.py is held to, written once for the four agents, and the bodies of the tests that both modules hold."""
from unittest import mock

import numpy as np
import torch

import learner_cases as K
import learner_ref64 as R

HP_GOLDEN = dict(K.HP, beta1=0.9)
# against autograd: a q_weight whose 1 - q_weight is an f32 value, so that the kernel's two f32 weights ARE the torch learner's
HP = dict(HP_GOLDEN, q_weight=0.25)
HP_DEFECT = dict(HP, **K.HP_DEFECT)
TOL = 2.0 ** -18                # 2^-42 (a few hundred float64 roundings) of a quantity's magnitude, in bad_elements' units of 2^-24


def zeros(agent, learner):
    """the state of a fresh torch learner: its nets, zero moments, zero counters"""
    nets = {n: getattr(learner, n) for n in R.NETS[agent]}
    moments = {n: ([torch.zeros_like(p) for p in nets[n].parameters()],) * 2 for n in R.LEARNING[agent]}
    return R.state_from(agent, nets, moments, {n: 0 for n in R.LEARNING[agent]})


def assert_golden_nets(agent, st, g, flipped=()):
    """every element within 1e-5 of the recorded parameters; the nets `flipped`: within 7e-3 (see the DATD3 test)"""
    for name in R.NETS[agent]:
        suffixes = ["fc%d_%s" % (i + 1, wb) for i in range(len(st[name]) // 2) for wb in ("weight", "bias")]
        for suffix, v in zip(suffixes, st[name]):
            ref = g[f"{name}__{suffix}"]
            assert np.abs(v.numpy() - ref).max() < (7e-3 if name in flipped else 1e-5), (name, suffix, np.abs(v.numpy() - ref).max())


def _torch_state(agent, t):
    adam = {name: R.adam_state(getattr(t, name), getattr(t, name + "_opt")) for name in R.LEARNING[agent]}
    return R.state_from(agent, {n: getattr(t, n) for n in R.NETS[agent]}, {n: mvs[:2] for n, mvs in adam.items()},
                        {n: mvs[2] for n, mvs in adam.items()})


_AUTOGRAD = {}


def autograd_case(agent, B, D, k, seed, hp, gain=1.0, with_actor=True):
    """The torch learner's networks and Adam in float64 (torch autograd), two priming updates (k = 1, then k = 2; TD3: both with the
    actor step), then update k (TD3: with or without the actor step).  Returns (state before it, batch, noise, state after it, the
    gradients the update applied, its critic loss).  `gain` scales the target actors' last layers (pre-tanh outputs of order one, so
    that target actions reach the clamp)."""
    key = (agent, B, D, k, seed, tuple(sorted(hp.items())), gain, with_actor)
    if key in _AUTOGRAD:
        return _AUTOGRAD[key]
    from armenv.daddpg import DADDPG
    from armenv.datd3 import DARC, DATD3
    from armenv.td3 import TD3
    torch.manual_seed(seed)
    kw = dict(device="cpu", actor_lr=hp["actor_lr"], critic_lr=hp["critic_lr"], tau=hp["tau"], gamma=hp["gamma"])
    if agent != "daddpg":
        kw.update(policy_noise=hp["policy_noise"], noise_clip=hp["noise_clip"])
    if agent == "td3":
        kw.update(policy_freq=1)
    if agent == "darc":
        kw.update(q_weight=hp["q_weight"], regularization_weight=hp["regularization_weight"])
    t = dict(td3=TD3, daddpg=DADDPG, datd3=DATD3, darc=DARC)[agent](D, 3, hp["action_bound"], **kw)
    for n in t._nets():
        n.double()
    with torch.no_grad():
        for name in R.NETS[agent]:
            if name.startswith("target_actor"):
                getattr(t, name).fc3.weight.mul_(gain)
        if gain != 1.0 and agent in ("datd3", "darc"):     # twin target critics: the min picks either proposal on many rows
            for p2, p1 in zip(t.target_critic2.parameters(), t.target_critic1.parameters()):
                p2.copy_(p1 * (1 + 0.02 * torch.randn(p1.shape, dtype=p1.dtype)))
    gen = torch.Generator().manual_seed(seed + 1)

    def update(batch, noise, kk, wa=True):
        args = (batch["states"], batch["actions"], batch["rewards"].view(-1, 1), batch["next_states"], batch["dones"].view(-1, 1))
        if agent == "td3":                                 # TD3 draws its noise itself
            with mock.patch.object(torch, "randn_like", lambda x: noise.clone()):
                return float(t._update(*args, wa))
        return float(t._update(*args, kk == 1) if agent == "daddpg" else t._update(*args, kk == 1, noise))
    for kk in (1, 2):
        update(R.random_batch(gen, B, D), torch.randn(B, 3, generator=gen, dtype=torch.float64), kk)
    st = _torch_state(agent, t)
    assert all(st[n + "_step"] == (2 if agent == "td3" or n == "critic" else 1) for n in R.LEARNING[agent])
    batch, noise = R.random_batch(gen, B, D), torch.randn(B, 3, generator=gen, dtype=torch.float64)
    loss = float(update(batch, noise, k, with_actor))
    after = _torch_state(agent, t)
    grads = {n: [p.grad.detach().clone() for p in getattr(t, n).parameters()] for n in R.LEARNING[agent]}
    _AUTOGRAD[key] = (st, batch, noise, after, grads, loss)
    return _AUTOGRAD[key]


def reference(agent, st, batch, noise, hp, k, **kw):
    return R.update(agent, st, batch, None if agent == "daddpg" else noise, hp, k=k, **kw)


def autograd_failures(out, after, grads, loss, forced=None):
    """names of the quantities of `out` that differ from the float64 autograd learner by more than 2^-42 of their magnitude (plus
    the allowance): the loss, and of every net that `out` stepped the gradients, stepped parameters and targets, and from `forced`
    (the reference fed autograd's gradients: a moment's magnitude b1 |m| + (1 - b1) |g| says nothing about a gradient that was itself
    summed from larger terms) both moments"""
    bad = []
    if abs(out["loss"] - loss) > TOL * R.U * out["loss_mag"]:
        bad.append("loss")
    for generic in ("critic", "actor"):
        net = out.get(generic + "_net")
        if net is None:
            continue
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


def check_reference_equals_autograd(agent, B, D, k, seed, with_actor=True):
    """Loss, gradients, Adam-stepped parameters, moments and targets equal those of the torch learner's update run in float64 with
    torch autograd and torch.optim.Adam, from primed (non-zero) Adam moments, to 2^-42 of their magnitudes; what the update does not
    own is returned as it was."""
    st, batch, noise, after, grads, loss = autograd_case(agent, B, D, k, seed, HP, with_actor=with_actor)
    out = reference(agent, st, batch, noise, HP, k, with_actor=with_actor, chunk=64)           # several chunks
    critic, actor = out["critic_net"], out.get("actor_net")
    forced = reference(agent, st, batch, noise, HP, k, with_actor=with_actor, critic_grad=grads[critic], actor_grad=grads.get(actor))
    assert autograd_failures(out, after, grads, loss, forced) == []
    assert out["ambiguous"] < 1e-3 * out["units"]
    if agent == "td3":
        assert out["units"] == B * 256 * (10 + (4 if with_actor else 0))
    if (agent == "daddpg" and k == 1) or not with_actor:   # DADDPG's update 1 and TD3's critic-only update leave the target critic alone
        assert all(torch.equal(a, b) for a, b in zip(out["target_critic"], st["target_critic"]))
        assert all(torch.equal(a, b) for a, b in zip(after["target_critic"], st["target_critic"]))


def check_defect_switch(agent, defect):
    """For both k: the undefective reference equals autograd, the defective one does not.  The switches bind: a third of the rows is
    terminal, the noise clip changes more than half the noise elements, the clamp more than a third of the target actions (a saturated
    action is pushed over the bound by noise of its own sign only, so a half is the ceiling), the two values under the min differ,
    and the regulariser is of the TD term's order.  (TD3 at the shape and target-actor gain it has always had here.)"""
    B, gain = (300, 30.0) if agent == "td3" else (257, 100.0)
    for k in (None,) if agent == "td3" else (1, 2):
        st, batch, noise, after, grads, loss = autograd_case(agent, B, 6, k, 4, HP_DEFECT, gain=gain)
        good = reference(agent, st, batch, noise, HP_DEFECT, k)
        assert autograd_failures(good, after, grads, loss) == []
        assert 0.2 < float(batch["dones"].mean()) < 0.5
        if agent != "td3":                                 # (two independent target heads: one may lie under the other on every row)
            assert 0.1 < K.pick_share(agent, st, batch, noise, HP_DEFECT) < 0.9
        if agent != "daddpg":
            assert float(((noise * HP_DEFECT["policy_noise"]).abs() > HP_DEFECT["noise_clip"]).double().mean()) > 0.5
            for a, raw in zip(K.target_actions(st, batch, noise, HP_DEFECT), K.target_actions(st, batch, noise, HP_DEFECT, clamp=False)):
                assert float((a != raw).double().mean()) > 1 / 3
        if agent == "darc":
            td = reference(agent, st, batch, noise, HP_DEFECT, k, defect="no_regulariser", with_actor=False)["loss"]
            assert 0.1 * td < good["loss"] - td < 10 * td, (td, good["loss"])
        bad = autograd_failures(reference(agent, st, batch, noise, HP_DEFECT, k, defect=defect), after, grads, loss)
        assert bad, (defect, k)


def check_case_inputs(c):
    """the reference on exactly the inputs that the GPU test of this case moves to the device: at most AMB_MAX of the relu units
    are within rounding of zero (K.amb_capped: all but TD3's noise cases), so that the allowance cannot make the comparison vacuous;
    the inputs are f32 values"""
    built = K.build(c)
    assert all(t.dtype == torch.float32 for ts in built["nets"].values() for t in ts)
    out = K.reference(c, built)
    assert out["units"] > 0 and (out["ambiguous"] <= K.AMB_MAX * out["units"] or not K.amb_capped(c)), (out["ambiguous"], out["units"])
    assert all(bool(torch.isfinite(t).all()) for t in out["critic_grad"] + out.get("actor_grad", []))
    if c["tag"] == "edge-clamp_binds":
        st, b, n = K.state64(c, built), K.batch64(built), K.noise64(built)
        assert all(float((a.abs() == c["hp"]["action_bound"]).double().mean()) > 0.5 for a in K.target_actions(st, b, n, c["hp"]))
    if c["tag"] == "edge-dones_all_1":
        assert torch.equal(out["target"], K.batch64(built)["rewards"])
