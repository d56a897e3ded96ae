"""The float64 comparisons of tests/test_gpu_td3_ref64.py and tests/test_gpu_da_ref64.py (test infrastructure), written once for the
four agents over the cases of tests/learner_cases.py: one harness (make, update, owned / unowned_changes, against_float64), one C
table and Bounds, and the body of every test that both modules hold.  The two modules register this one for pytest's assertion
rewriting before they import it."""
import copy
import os

import torch

import learner_cases as K
import learner_ref64 as R
from learner_gpu import DEV, Bounds, f64

C = dict(critic_grad=1.0, actor_grad=0.5, loss=0.05, adam=16.0, noise=0.015)
NO_ACTOR = 1 << 40               # a policy_freq under which no TD3 update takes the actor step
BOUNDS = Bounds(C, K.AMB_MAX)


def write_ratios():
    """ARMENV_REF64_RATIOS=<path>: write the largest measured ratio per kind and case there (calibration of C); both modules call
    it when they end, the later call holds both modules' ratios"""
    BOUNDS.write(os.environ.get("ARMENV_REF64_RATIOS"))


def make(c, built, beta1=None, seed=0):
    """the fused learner of case `c` on the device with every hyper-parameter set before its first update and the state `built`:
    parameters, targets, Adam moments (TD3's twin critic: twelve tensors each, in parameters() order) and step counters; the next
    update steps actor (and critic) c["k"], TD3's takes the actor step or not as c["with_actor"] says"""
    from armenv.fused_daddpg import FusedDADDPG
    from armenv.fused_datd3 import FusedDARC, FusedDATD3
    from armenv.fused_td3 import FusedTD3
    agent, hp = c["agent"], c["hp"]
    kw = dict(actor_lr=hp["actor_lr"], critic_lr=hp["critic_lr"], tau=hp["tau"], gamma=hp["gamma"], device=DEV)
    if agent != "daddpg":
        kw.update(policy_noise=hp["policy_noise"], noise_clip=hp["noise_clip"], seed=seed)
    if agent == "td3":
        kw.update(policy_freq=1 if c["with_actor"] else NO_ACTOR)
    if agent == "darc":
        kw.update(q_weight=hp["q_weight"], regularization_weight=hp["regularization_weight"])
    f = dict(td3=FusedTD3, daddpg=FusedDADDPG, datd3=FusedDATD3, darc=FusedDARC)[agent](c["D"], 3, hp["action_bound"], **kw)
    f.betas, f.eps = (hp["beta1"] if beta1 is None else beta1, hp["beta2"]), hp["eps"]
    with torch.no_grad():
        for name in R.NETS[agent]:
            for p, t in zip(getattr(f, name).parameters(), built["nets"][name], strict=True):
                p.copy_(t)
        for name in R.LEARNING[agent]:
            for mv, ts in zip(("_m", "_v"), built["moments"][name]):
                for p, t in zip(getattr(f, name + mv), ts, strict=True):
                    p.copy_(t)
            setattr(f, name + "_step", built["steps"][name])
    if agent == "daddpg":
        f.total_it = 1 if c["k"] == 1 else 0          # update n steps actor 1 when n is even
    return f


def snapshot(f, agent):
    """every tensor an update may write, by name, as it is now"""
    out = {name: [p.detach().clone() for p in getattr(f, name).parameters()] for name in R.NETS[agent]}
    for name in R.LEARNING[agent]:
        out[name + "_m"], out[name + "_v"] = [t.clone() for t in getattr(f, name + "_m")], [t.clone() for t in getattr(f, name + "_v")]
    return out


def owned(c):
    critic, actor = K.stepped(c)
    names = [critic, critic + "_m", critic + "_v"]
    if c["with_actor"]:
        names += [actor, actor + "_m", actor + "_v", "target_" + actor]
    if c["with_actor"] and (c["agent"] != "daddpg" or c["k"] == 2):
        names.append("target_" + critic)
    return names


def update(f, c, built, noise="case"):
    """one fused update of case `c`; returns the kernel's outputs in float64 under learner_ref64's generic names, the loss, and
    `all`: the snapshot of every tensor after the update"""
    b = {k: v.to(DEV) for k, v in built["batch"].items()}
    if c["agent"] == "daddpg":
        loss = f.train(b)
    else:
        n = built["noise"] if isinstance(noise, str) else noise
        n = None if n is None else n.to(DEV, torch.float32)
        loss = f.train(b, noise=n) if c["agent"] == "td3" else f.update(b, c["k"] == 1, n)
    snap = snapshot(f, c["agent"])
    got = dict(loss=float(loss), all=snap)
    for generic, net in zip(("critic", "actor"), K.stepped(c)):
        for suffix in ("", "_m", "_v"):
            got[generic + suffix] = f64(snap[net + suffix])
        got["target_" + generic] = f64(snap["target_" + net])
    return got


def unowned_changes(c, built, got):
    """names of the tensors that the update of case `c` does not own and that differ, bit for bit, from what was installed"""
    before = dict(built["nets"])
    for name in R.LEARNING[c["agent"]]:
        before[name + "_m"], before[name + "_v"] = built["moments"][name]
    unowned = dict(td3=0 if c["with_actor"] else 5, daddpg=5 if c["k"] == 1 else 4).get(c["agent"], 8)
    assert len(before) - len(owned(c)) == unowned
    return [name for name, ts in before.items() if name not in owned(c)
            and not all(torch.equal(a.to(DEV), b) for a, b in zip(ts, got["all"][name]))]


def differing(a, b, names):
    """the names of `names` under which a and b are not bitwise equal"""
    return [n for n in names if not all(torch.equal(x, y) for x, y in zip(a[n], b[n]))]


def against_float64(c, release=False):
    """the update of case `c` against the reference: gradients and loss per element, and nothing unowned written (`release`: the
    learner's workspace is freed before the reference runs)"""
    built = K.build(c)
    f = make(c, built)
    got = update(f, c, built)
    if release:
        f._ws = None
        torch.cuda.empty_cache()
    out = K.reference(c, built, DEV, stepped_critic=got["critic"])
    BOUNDS.ambiguity_is_rare(out)
    assert BOUNDS.grad_failures(K.case_id(c), got, out, c["with_actor"]) == []
    assert unowned_changes(c, built, got) == []
    return built, got, out


def check_every_defect_fails(c):
    """With both gradients teacher-forced: the undefective reference passes every comparison, each planted defect fails one."""
    built = K.build(c)
    got = update(make(c, built), c, built)

    def failures(defect):
        out = K.reference(c, built, DEV, stepped_critic=got["critic"], critic_grad=got["critic_m"], actor_grad=got["actor_m"],
                          defect=defect)
        rec = defect is None
        return BOUNDS.grad_failures(K.case_id(c), got, out, record=rec) + BOUNDS.adam_failures(K.case_id(c), got, out, record=rec)
    assert failures(None) == []
    for defect in R.DEFECTS[c["agent"]]:
        assert failures(defect), defect


def check_adam_and_soft_update(agent, k, step):
    """Default betas, every optimiser of the agent.  The float64 Adam takes the kernel's own gradient, read from a beta1 = 0 twin of
    the same state: the critic's (its gradient does not depend on the betas), then the actor's with critic_lr = 0 (so that both twins'
    actor losses see the same critic).  Parameters, moments and the targets that the update soft-updates within C_adam 2^-24 of
    |p| + |step| (and of the moments' own magnitudes)."""
    for side in ("critic", "actor"):
        c = K.adam_case(agent, k, step, side)
        assert any(K.case_id(c) == K.case_id(x) for x in K.ADAM_CASES)
        built = K.build(c)
        got, got0 = update(make(c, built), c, built), update(make(c, built, beta1=0.0), c, built)
        out = K.reference(c, built, DEV, critic_grad=got0["critic_m"], actor_grad=got0["actor_m"])
        assert BOUNDS.adam_failures(K.case_id(c), got, out, sides=(side,)) == [], side
        before = dict(zip(("critic", "actor"), (K.state64(c, built, DEV)[n] for n in K.stepped(c))))
        assert not all(torch.equal(a, b) for a, b in zip(got[side], before[side]))
        if side == "actor":                                  # critic_lr = 0: the critic did not move, bit for bit
            assert all(torch.equal(a, b) for a, b in zip(got["critic"], before["critic"]))


def check_lr_zero_and_tau_edges(agent, k):
    """lr = 0 leaves every parameter unchanged; tau = 0 leaves the targets unchanged; tau = 1 makes the soft-updated targets equal
    their nets; bit for bit."""
    def run(name):
        c = K.exact_case(agent, k, name)
        built = K.build(c)
        return c, K.state64(c, built, DEV), update(make(c, built), c, built)
    c, st, got = run("lr_0")
    critic, actor = K.stepped(c)
    assert all(torch.equal(a, b) for a, b in zip(got["critic"] + got["actor"], st[critic] + st[actor]))
    c, st, got = run("tau_0")
    assert all(torch.equal(a, b) for a, b in zip(got["target_critic"] + got["target_actor"], st["target_" + critic] + st["target_" + actor]))
    assert not all(torch.equal(a, b) for a, b in zip(got["critic"] + got["actor"], st[critic] + st[actor]))
    c, st, got = run("tau_1")
    assert not all(torch.equal(a, b) for a, b in zip(got["critic"] + got["actor"], st[critic] + st[actor]))
    assert all(torch.equal(a, b) for a, b in zip(got["target_actor"], got["actor"]))
    if "target_" + critic in owned(c):
        assert all(torch.equal(a, b) for a, b in zip(got["target_critic"], got["critic"]))
    else:                                                    # DADDPG's update 1 leaves the target critic alone at any tau
        assert all(torch.equal(a, b) for a, b in zip(got["target_critic"], st["target_critic"]))


def no_target_net_is_read(c, built, got):
    """the loss and the critic's step of the update `got` of case `c`, whose every done is set, are bitwise the same under other
    target nets (all of them scaled and shifted)"""
    other = copy.deepcopy(built)
    for name in R.NETS[c["agent"]]:
        if name.startswith("target_"):
            other["nets"][name] = [t * -3.0 + 0.25 for t in other["nets"][name]]
    got2 = update(make(c, other), c, other)
    assert got2["loss"] == got["loss"]
    assert differing(got, got2, ("critic", "critic_m", "critic_v")) == []
    assert differing(got, got2, ("target_actor",)) == ["target_actor"]                # the other targets were really installed


def check_every_done_set(agent, k):
    """Every done set: the target is the rewards, and the loss and the critic's step do not depend on the target nets."""
    c = K.exact_case(agent, k, "all_done")
    built = K.build(c)
    got = update(make(c, built), c, built)
    no_target_net_is_read(c, built, got)
    out = K.reference(c, built, DEV, stepped_critic=got["critic"])
    assert torch.equal(out["target"], K.batch64(built, DEV)["rewards"])


def check_noise_clip_zero_equals_no_noise(agent, k):
    got = []
    for name in ("noise_clip_0", "policy_noise_0"):
        c = K.exact_case(agent, k, name)
        built = K.build(c)
        got.append(update(make(c, built), c, built))
    assert got[0]["loss"] == got[1]["loss"]
    assert differing(got[0], got[1], ("critic", "critic_m", "critic_v", "actor", "actor_m", "actor_v", "target_critic", "target_actor")) == []


def check_hyper_parameter_edge(c):
    """gamma 0 and 1, no done and every done set (then the target is the rewards, and TD3 reads no target net), a clamp that binds on
    more than half of every proposal, and a DARC regulariser as large as the TD term: gradients and loss per element."""
    built, got, out = against_float64(c)
    if c["tag"] == "edge-clamp_binds":
        acts = K.target_actions(K.state64(c, built, DEV), K.batch64(built, DEV), K.noise64(built, DEV), c["hp"])
        assert all(float((a.abs() == c["hp"]["action_bound"]).double().mean()) > 0.5 for a in acts)
    if c["tag"] == "edge-dones_all_1":
        assert torch.equal(out["target"], K.batch64(built, DEV)["rewards"])
        if c["agent"] == "td3":
            no_target_net_is_read(c, built, got)
    if c["tag"] == "edge-reg_1":                             # control: the reference without the regulariser fails
        plain = K.reference(c, built, DEV, stepped_critic=got["critic"], defect="no_regulariser")
        assert plain["loss"] < out["loss"] and BOUNDS.grad_failures(K.case_id(c), got, plain, record=False)


def check_in_kernel_noise(agent, B, seed, draw):
    """train(batch) with the in-kernel Philox noise against train(batch, noise=z) with z = learner_ref64.kernel_noise(seed, draw,
    rows) from the same state.  TD3: one update without the actor step, its draw is its number (total_it).  DATD3: the two updates of
    one train, noise=(z(draw), z(draw + 1)); tau = 0, so that update 2 (critic 2) reads nothing that update 1 wrote.  The gradients of
    the regressing heads and the loss may differ by C_noise 2^-24 (S + M): S, the root-sum-square sensitivity to a noise change of
    one f32 rounding of the Box-Muller radius per element (learner_ref64.noise_sensitivity), and M, the magnitude that bounds the f32
    rounding of the update itself.  State feature 0 is zero except on row B // 2, so that the column of the fc1 weight gradients that
    it feeds is that row's alone.  Controls: the previous draws' noise fails the bound for every update; row B // 2's noise moved by
    1e-3 fails it (for a single k of DATD3 the three moved components may cancel in the target's derivative, so the count is over
    both updates)."""
    import numpy as np
    cases = K.noise_cases(agent, B, seed, draw)
    assert all(any(K.case_id(c) == K.case_id(x) for x in K.NOISE_CASES) for c in cases)
    builts = [K.build(c) for c in cases]
    host = [b["noise"].to(DEV) for b in builts]
    b = {k: v.to(DEV) for k, v in builts[0]["batch"].items()}
    moments = [K.stepped(c)[0] + "_m" for c in cases]

    def run(noise):
        f = make(cases[0], builts[0], seed=seed)
        f.total_it = draw - 1
        noise = noise if noise is None else [n.to(torch.float32) for n in noise]
        losses = f.train(b, noise=noise if noise is None else noise[0] if agent == "td3" else tuple(noise))
        assert f.total_it == draw - 1 + len(cases)
        return [dict(loss=float(loss), critic_m=f64(getattr(f, m))) for loss, m in zip([losses] if agent == "td3" else losses, moments)]
    got_k, got_h = run(None), run(host)
    bounds = []
    for c, built, h in zip(cases, builts, host):
        raw = K.target_actions(K.state64(c, built, DEV), K.batch64(built, DEV), h, c["hp"], clamp=False)     # neither clipped nor clamped
        assert float((h * c["hp"]["policy_noise"]).abs().max()) < c["hp"]["noise_clip"]
        assert all(float(a.abs().max()) < c["hp"]["action_bound"] for a in raw)
        radius = torch.from_numpy(R.kernel_noise(seed, c["noise"][2], np.arange(B), with_radius=True)[1]).to(DEV)
        sens, lsens = R.noise_sensitivity(agent, K.state64(c, built, DEV), K.batch64(built, DEV), h, radius, c["hp"], c["k"])
        out = K.reference(c, built, DEV, with_actor=False)
        bounds.append(([s + m for s, m in zip(sens, out["critic_grad_mag"])], lsens + out["loss_mag"]))

    def beyond(got, i, record):
        mags, lmag = bounds[i]
        case = K.case_id(cases[i])
        assert len(got[i]["critic_m"]) == len(mags) == (12 if agent == "td3" else 6)
        n = sum(BOUNDS.check("noise", case, x, y, m, record=record) for x, y, m in zip(got[i]["critic_m"], got_k[i]["critic_m"], mags))
        lt = lambda x: torch.tensor([x], dtype=torch.float64)
        return n + BOUNDS.check("noise", case + " loss", lt(got[i]["loss"]), lt(got_k[i]["loss"]), lt(lmag), record=record)
    ups = range(len(cases))
    assert [beyond(got_h, i, True) for i in ups] == [0] * len(cases)
    prev = run([torch.from_numpy(R.kernel_noise(seed, draw - 1 + i, np.arange(B))).to(DEV) for i in ups])
    assert all(beyond(prev, i, False) > 0 for i in ups)
    moved = [h.clone() for h in host]
    for m in moved:
        m[B // 2] += 1e-3
    got_m = run(moved)
    assert sum(beyond(got_m, i, False) for i in ups) > 0
