"""The fused DADDPG, DATD3 and DARC updates (armenv_daddpg_update / armenv_datd3_update through FusedDADDPG.train, FusedDATD3.update
and FusedDARC.update) on cuda:0 against the float64 restatements of tests/da_ref64.py, as tests/test_gpu_td3_ref64.py holds TD3: per
element, |g_hip - g_ref| <= C 2^-24 M_ref + allowance_ref, where M is the contraction chain over absolute values and the allowance
is what flows through relu units within rounding of zero.

The gradient the kernel applied is read exactly: with betas = (0, 0.999), Adam's first moment after the update IS the gradient.
Each stage is compared on its own (teacher forcing): the actor's gradient through the kernel's own stepped critic, the Adam steps
fed the kernel's own gradient.  Every input is built on the CPU (tests/da_cases.py) and moved to the device; tests/test_da_ref64.py
checks the same inputs for ambiguity without a GPU.  C is one constant per kind of quantity, calibrated on the MI355X
(profiles/da_ref64_errors.txt records the largest measured ratios; each C is at most 8x the largest, and TD3's value where that
already satisfies the rule)."""
import copy
import os

import numpy as np
import pytest
import torch

import da_cases as K
import da_ref64 as R
from learner_gpu import DEV, Bounds, f64 as _f64

pytestmark = pytest.mark.gpu
C = dict(critic_grad=1.0, actor_grad=0.5, loss=0.05, adam=16.0, noise=0.015)
BOUNDS = Bounds(C, K.AMB_MAX)
_check, _grad_failures, _adam_failures = BOUNDS.check, BOUNDS.grad_failures, BOUNDS.adam_failures
_ambiguity_is_rare = BOUNDS.ambiguity_is_rare


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    """ARMENV_DA_REF64_RATIOS=<path>: write the largest measured ratio per kind and case there (calibration of C)"""
    yield
    BOUNDS.write(os.environ.get("ARMENV_DA_REF64_RATIOS"))


def _critic_net(c):
    return "critic" if c["agent"] == "daddpg" else "critic%d" % c["k"]


def _make(c, built, beta1=None, seed=0):
    """the fused learner of case `c` on the device with every hyper-parameter set before its first update and the state `built`:
    parameters, targets, Adam moments and step counters; the next update steps actor (and critic) c["k"]"""
    from armenv.fused_daddpg import FusedDADDPG
    from armenv.fused_datd3 import FusedDARC, FusedDATD3
    agent, hp = c["agent"], c["hp"]
    kw = dict(actor_lr=hp["actor_lr"], critic_lr=hp["critic_lr"], tau=hp["tau"], gamma=hp["gamma"], device=DEV)
    if agent != "daddpg":
        kw.update(policy_noise=hp["policy_noise"], noise_clip=hp["noise_clip"], seed=seed)
    if agent == "darc":
        kw.update(q_weight=hp["q_weight"], regularization_weight=hp["regularization_weight"])
    f = dict(daddpg=FusedDADDPG, datd3=FusedDATD3, darc=FusedDARC)[agent](c["D"], 3, hp["action_bound"], **kw)
    f.betas, f.eps = (hp["beta1"] if beta1 is None else beta1, hp["beta2"]), hp["eps"]
    with torch.no_grad():
        for name in R.NETS[agent]:
            for p, t in zip(getattr(f, name).parameters(), built["nets"][name]):
                p.copy_(t)
        for name in R.LEARNING[agent]:
            for mv, ts in zip(("_m", "_v"), built["moments"][name]):
                for p, t in zip(getattr(f, name + mv), ts):
                    p.copy_(t)
            setattr(f, name + "_step", built["steps"][name])
    if agent == "daddpg":
        f.total_it = 1 if c["k"] == 1 else 0          # update n steps actor 1 when n is even
    return f


def _snapshot(f, agent):
    """every tensor an update may write, by name, as it is now"""
    out = {name: [p.detach().clone() for p in getattr(f, name).parameters()] for name in R.NETS[agent]}
    for name in R.LEARNING[agent]:
        out[name + "_m"], out[name + "_v"] = [t.clone() for t in getattr(f, name + "_m")], [t.clone() for t in getattr(f, name + "_v")]
    return out


def _owned(c):
    critic, actor = _critic_net(c), "actor%d" % c["k"]
    names = [critic, critic + "_m", critic + "_v", actor, actor + "_m", actor + "_v", "target_" + actor]
    if c["agent"] != "daddpg" or c["k"] == 2:
        names.append("target_" + critic)
    return names


def _update(f, c, built, noise="case"):
    """one fused update of case `c`; returns the kernel's outputs in float64 under da_ref64's generic names, the loss, and `all`:
    the snapshot of every tensor after the update"""
    batch = {k: v.to(DEV) for k, v in built["batch"].items()}
    if c["agent"] == "daddpg":
        loss = f.train(batch)
    else:
        n = built["noise"] if isinstance(noise, str) else noise
        loss = f.update(batch, c["k"] == 1, None if n is None else n.to(DEV, torch.float32))
    snap = _snapshot(f, c["agent"])
    critic, actor = _critic_net(c), "actor%d" % c["k"]
    got = dict(loss=float(loss), all=snap)
    for generic, net in (("critic", critic), ("actor", actor)):
        for suffix in ("", "_m", "_v"):
            got[generic + suffix] = _f64(snap[net + suffix])
        got["target_" + generic] = _f64(snap["target_" + net])
    return got


def _unowned_changes(c, built, got):
    """names of the tensors that update c["k"] does not own and that differ, bit for bit, from what was installed"""
    before = dict(built["nets"])
    for name in R.LEARNING[c["agent"]]:
        before[name + "_m"], before[name + "_v"] = built["moments"][name]
    owned = _owned(c)
    assert len(before) - len(owned) == (4 if c["agent"] == "daddpg" else 8) + (1 if c["agent"] == "daddpg" and c["k"] == 1 else 0)
    return [name for name, ts in before.items() if name not in owned
            and not all(torch.equal(a.to(DEV), b) for a, b in zip(ts, got["all"][name]))]


def _against_float64(c):
    """the update of case `c` against the reference: gradients and loss per element, and nothing unowned written"""
    built = K.build(c)
    got = _update(_make(c, built), c, built)
    out = K.reference(c, built, DEV, stepped_critic=got["critic"])
    _ambiguity_is_rare(out)
    assert _grad_failures(K.case_id(c), got, out) == []
    assert _unowned_changes(c, built, got) == []
    return built, got, out


@pytest.mark.parametrize("c", K.GRAD_CASES, ids=K.case_id)
def test_gradients_and_loss_against_float64(c):
    """All 6 critic and 6 actor gradient tensors and the loss, element by element, within C 2^-24 M + allowance, for both parities
    of DADDPG and both k of DATD3 / DARC, at batch sizes around the 4 rows of a head block, the 64-row gemm tile, the 256-row
    weight-gradient slice and the 256-thread loss reduction, and at five state widths.  In the same run, everything that the update
    does not own -- the other actor with its moments and target, DATD3's / DARC's other critic with its moments and target, DADDPG's
    target critic on update 1 -- is bitwise unchanged."""
    _against_float64(c)


@pytest.mark.parametrize("c", K.DEFECT_CASES, ids=K.case_id)
def test_every_defect_fails_a_gpu_comparison(c):
    """With both gradients teacher-forced: the undefective reference passes every comparison, each planted defect fails one."""
    built = K.build(c)
    got = _update(_make(c, built), c, built)

    def failures(defect):
        out = K.reference(c, built, DEV, stepped_critic=got["critic"], critic_grad=got["critic_m"], actor_grad=got["actor_m"],
                          defect=defect)
        rec = defect is None
        return _grad_failures(K.case_id(c), got, out, record=rec) + _adam_failures(K.case_id(c), got, out, record=rec)
    assert failures(None) == []
    for defect in R.DEFECTS[c["agent"]]:
        assert failures(defect), defect


@pytest.mark.parametrize("step", K.ADAM_STEPS)
@pytest.mark.parametrize("agent,k", K.AGENT_K)
def test_adam_and_soft_update_against_float64(agent, k, step):
    """Default betas, every optimiser of every agent (the critic of both DADDPG parities; critic k and actor k).  The float64 Adam
    takes the kernel's own gradient, read from a beta1 = 0 twin of the same state: the critic's (its gradient does not depend on the
    betas), then the actor's with critic_lr = 0 (so that both twins' actor losses see the same critic).  Parameters, moments and the
    targets that the update soft-updates within C_adam 2^-24 of |p| + |step| (and of the moments' own magnitudes)."""
    for side in ("critic", "actor"):
        c = K.adam_case(agent, k, step, side)
        assert any(K.case_id(c) == K.case_id(x) for x in K.ADAM_CASES)
        built = K.build(c)
        got, got0 = _update(_make(c, built), c, built), _update(_make(c, built, beta1=0.0), c, built)
        out = K.reference(c, built, DEV, critic_grad=got0["critic_m"], actor_grad=got0["actor_m"])
        assert _adam_failures(K.case_id(c), got, out, sides=(side,)) == [], side
        assert not all(torch.equal(a, b) for a, b in zip(got[side], K.state64(c, built, DEV)[_critic_net(c) if side == "critic" else "actor%d" % k]))
        if side == "actor":                                  # critic_lr = 0: the critic did not move, bit for bit
            assert all(torch.equal(a, b) for a, b in zip(got["critic"], K.state64(c, built, DEV)[_critic_net(c)]))


def _differing(a, b, names):
    """the names of `names` under which a and b are not bitwise equal"""
    return [n for n in names if not all(torch.equal(x, y) for x, y in zip(a[n], b[n]))]


@pytest.mark.parametrize("agent,k", K.AGENT_K)
def test_lr_zero_and_tau_edges_are_exact(agent, k):
    """lr = 0 leaves every parameter unchanged; tau = 0 leaves the targets unchanged; tau = 1 makes the soft-updated targets equal
    their nets; bit for bit."""
    def run(name):
        c = K.exact_case(agent, k, name)
        built = K.build(c)
        return c, K.state64(c, built, DEV), _update(_make(c, built), c, built)
    c, st, got = run("lr_0")
    critic, actor = _critic_net(c), "actor%d" % k
    assert all(torch.equal(a, b) for a, b in zip(got["critic"] + got["actor"], st[critic] + st[actor]))
    c, st, got = run("tau_0")
    assert all(torch.equal(a, b) for a, b in zip(got["target_critic"] + got["target_actor"], st["target_" + critic] + st["target_" + actor]))
    assert not all(torch.equal(a, b) for a, b in zip(got["critic"] + got["actor"], st[critic] + st[actor]))
    c, st, got = run("tau_1")
    assert not all(torch.equal(a, b) for a, b in zip(got["critic"] + got["actor"], st[critic] + st[actor]))
    assert all(torch.equal(a, b) for a, b in zip(got["target_actor"], got["actor"]))
    if "target_" + critic in _owned(c):
        assert all(torch.equal(a, b) for a, b in zip(got["target_critic"], got["critic"]))
    else:                                                    # DADDPG's update 1 leaves the target critic alone at any tau
        assert all(torch.equal(a, b) for a, b in zip(got["target_critic"], st["target_critic"]))


@pytest.mark.parametrize("agent,k", K.AGENT_K)
def test_with_every_done_set_no_target_net_is_read(agent, k):
    """Every done set: the target is the rewards, and the loss and the critic's step are bitwise the same under other target nets
    (all of them scaled and shifted)."""
    c = K.exact_case(agent, k, "all_done")
    built = K.build(c)
    got = _update(_make(c, built), c, built)
    other = copy.deepcopy(built)
    for name in R.NETS[agent]:
        if name.startswith("target_"):
            other["nets"][name] = [t * -3.0 + 0.25 for t in other["nets"][name]]
    got2 = _update(_make(c, other), c, other)
    assert got2["loss"] == got["loss"]
    assert _differing(got, got2, ("critic", "critic_m", "critic_v")) == []
    assert _differing(got, got2, ("target_actor",)) == ["target_actor"]                # the other targets were really installed
    out = K.reference(c, built, DEV, stepped_critic=got["critic"])
    assert torch.equal(out["target"], K.batch64(built, DEV)["rewards"])


@pytest.mark.parametrize("agent,k", [x for x in K.AGENT_K if x[0] != "daddpg"])
def test_noise_clip_zero_equals_no_noise_bit_for_bit(agent, k):
    got = []
    for name in ("noise_clip_0", "policy_noise_0"):
        c = K.exact_case(agent, k, name)
        built = K.build(c)
        got.append(_update(_make(c, built), c, built))
    assert got[0]["loss"] == got[1]["loss"]
    assert _differing(got[0], got[1], ("critic", "critic_m", "critic_v", "actor", "actor_m", "actor_v", "target_critic", "target_actor")) == []


@pytest.mark.parametrize("q_weight", [0, 1])
@pytest.mark.parametrize("k", [1, 2])
def test_darc_without_regulariser_and_with_a_trivial_mix_is_datd3_bit_for_bit(k, q_weight):
    """FusedDARC with regularization_weight = 0 and q_weight 0 or 1 equals FusedDATD3 from the same state in every parameter, moment
    and target and in the loss: 0 T + 1 T, d3 + 0 (...) and red0 inv_b + 0 (...) are exact, and the loss column keeps its summation
    order between one column and two."""
    c = K.exact_case("darc", k, "as_datd3_q%d" % q_weight)
    built = K.build(c)
    got = _update(_make(c, built), c, built)
    c3 = dict(c, agent="datd3", hp={n: c["hp"][n] for n in R.HP_KEYS["datd3"]})
    got3 = _update(_make(c3, built), c3, built)
    assert got["loss"] == got3["loss"], (got["loss"], got3["loss"])
    assert _differing(got["all"], got3["all"], sorted(got["all"])) == []
    assert _differing(got["all"], _snapshot(_make(c, built), "darc"), _owned(c)) == _owned(c)          # everything owned has moved


@pytest.mark.parametrize("c", K.EDGE_CASES, ids=K.case_id)
def test_hyper_parameter_edges_against_float64(c):
    """gamma 0 and 1, no done and every done set, a clamp that binds on more than half of both proposals, and a DARC regulariser as
    large as the TD term: gradients and loss per element."""
    built, got, out = _against_float64(c)
    if c["tag"] == "edge-clamp_binds":
        acts = K.target_actions(K.state64(c, built, DEV), K.batch64(built, DEV), K.noise64(built, DEV), c["hp"])
        assert all(float((a.abs() == c["hp"]["action_bound"]).double().mean()) > 0.5 for a in acts)
    if c["tag"] == "edge-reg_1":                             # control: the reference without the regulariser fails
        plain = K.reference(c, built, DEV, stepped_critic=got["critic"], defect="no_regulariser")
        assert plain["loss"] < out["loss"] and _grad_failures(K.case_id(c), got, plain, record=False)


@pytest.mark.parametrize("B,seed,draw", K.NOISE_PARAMS)
def test_in_kernel_noise_equals_the_host_restatement(B, seed, draw):
    """FusedDATD3.train(batch) with the in-kernel Philox noise against train(batch, noise=(z(draw), z(draw + 1))) with
    z = td3_ref64.kernel_noise(seed, draw, rows) from the same state: the first update's draw is its number (total_it), the second
    update's the next.  tau = 0, so that update 2 (critic 2) reads nothing that update 1 wrote.  The gradients of critic k and its loss
    may differ by C_noise 2^-24 (S + M): S, the root-sum-square sensitivity to a noise change of one f32 rounding of the Box-Muller
    radius per element (da_ref64.noise_sensitivity: two proposals under one draw), and M, the magnitude that bounds the f32 rounding
    of the update itself.  State feature 0 is zero except on row B // 2, so that the column of the fc1 weight gradients that it feeds
    is that row's alone.  Controls: the previous draws' noise fails the bound for both k; row B // 2's noise moved by 1e-3 fails it (for a
    single k the three moved components may cancel in the target's derivative, so the count is over both updates)."""
    cases = [K.noise_case(B, seed, draw, k) for k in (1, 2)]
    assert all(any(K.case_id(c) == K.case_id(x) for x in K.NOISE_CASES) for c in cases)
    builts = [K.build(c) for c in cases]
    host = [b["noise"].to(DEV) for b in builts]
    batch = {k: v.to(DEV) for k, v in builts[0]["batch"].items()}

    def run(noise):
        f = _make(cases[0], builts[0], seed=seed)
        f.total_it = draw - 1
        losses = f.train(batch, noise=None if noise is None else tuple(n.to(torch.float32) for n in noise))
        assert f.total_it == draw + 1
        return [dict(loss=float(losses[k - 1]), critic_m=_f64(getattr(f, "critic%d_m" % k))) for k in (1, 2)]
    got_k, got_h = run(None), run(host)
    bounds = []
    for c, built, h in zip(cases, builts, host):
        raw = K.target_actions(K.state64(c, built, DEV), K.batch64(built, DEV), h, c["hp"], clamp=False)     # neither clipped nor clamped
        assert float((h * c["hp"]["policy_noise"]).abs().max()) < c["hp"]["noise_clip"]
        assert all(float(a.abs().max()) < c["hp"]["action_bound"] for a in raw)
        radius = torch.from_numpy(R.kernel_noise(seed, c["noise"][2], np.arange(B), with_radius=True)[1]).to(DEV)
        sens, lsens = R.noise_sensitivity(K.state64(c, built, DEV), K.batch64(built, DEV), h, radius, c["hp"], c["k"], False)
        out = K.reference(c, built, DEV, with_actor=False)
        bounds.append(([s + m for s, m in zip(sens, out["critic_grad_mag"])], lsens + out["loss_mag"]))

    def beyond(got, k, record):
        mags, lmag = bounds[k - 1]
        case = K.case_id(cases[k - 1])
        n = sum(_check("noise", case, got[k - 1]["critic_m"][i], got_k[k - 1]["critic_m"][i], mags[i], record=record) for i in range(6))
        lt = lambda x: torch.tensor([x], dtype=torch.float64)
        return n + _check("noise", case + " loss", lt(got[k - 1]["loss"]), lt(got_k[k - 1]["loss"]), lt(lmag), record=record)
    assert [beyond(got_h, k, True) for k in (1, 2)] == [0, 0]
    prev = run([torch.from_numpy(R.kernel_noise(seed, draw - 1 + j, np.arange(B))).to(DEV) for j in (0, 1)])
    assert all(beyond(prev, k, False) > 0 for k in (1, 2))
    moved = [h.clone() for h in host]
    for m in moved:
        m[B // 2] += 1e-3
    got_m = run(moved)
    assert sum(beyond(got_m, k, False) for k in (1, 2)) > 0
