"""The fused TD3 update (armenv_td3_update through armenv.fused_td3.FusedTD3) on cuda:0 against the torch learner armenv.td3.TD3,
which restates TD3_MLP.train (the reference's algo/TD3/TD3_mlp.py:114-161): the reference's golden run, gradients from identical
states, free-running agreement, batch / state sizes, determinism, and the training loop with learner="hip"."""
import json

import numpy as np
import pytest
import torch

from conftest import golden_npz
from learner_gpu import DEV, assert_grads as _assert_grads, batch as _batch, to_numpy as _np

pytestmark = pytest.mark.gpu


def test_fused_td3_reproduces_the_golden_updates():
    """G8 on the fused path: the reference's six TD3_MLP.train updates (B = 64) from torch.manual_seed(0)'s initial weights, the
    target-policy noise of the golden run (torch.manual_seed(123), one randn(64, 3) per update) fed through noise_dev; tolerances of
    test_td3_learner_golden_on_the_gpu."""
    from armenv.fused_td3 import FusedTD3
    from armenv.td3 import TD3
    g = golden_npz("td3_train_seed0.npz")
    torch.manual_seed(0)
    cpu = TD3(6, 3, 0.7, device="cpu")
    torch.manual_seed(0)
    agent = FusedTD3(6, 3, 0.7, device=DEV)
    for a, b in zip(agent._nets(), cpu._nets()):                 # same constructor order: same initial weights
        for k, v in a.state_dict().items():
            assert torch.equal(v.cpu(), b.state_dict()[k]), k
    torch.manual_seed(123)
    for i, want in enumerate(g["losses"]):
        b = {k: torch.from_numpy(g[f"b{i}_{k}"]).to(DEV) for k in ("states", "actions", "next_states", "rewards", "dones")}
        noise = torch.randn(64, 3).to(DEV)
        loss = float(agent.train(b, noise=noise))
        assert abs(loss - want) < 2e-5 * max(1.0, abs(want)), (i, loss, want)
    assert agent.total_it == 6 and agent.critic_step == 6 and agent.actor_step == 2
    ref = TD3(6, 3, 0.7, device=DEV)
    for name, net, rnet in (("actor", agent.actor, ref.actor), ("critic", agent.critic, ref.critic),
                            ("target_actor", agent.target_actor, ref.target_actor), ("target_critic", agent.target_critic, ref.target_critic)):
        rnet.load_state_dict({k: torch.from_numpy(g[f"{name}__{k.replace('.', '_')}"]) for k in net.state_dict()})
        for k, v in net.state_dict().items():
            d = np.abs(_np(v) - g[f"{name}__{k.replace('.', '_')}"])
            assert (d < 2e-5).mean() > 0.999 and d.max() < 7e-3, (name, k, (d < 2e-5).mean(), d.max())
    s0, a0 = torch.from_numpy(g["b0_states"]).to(DEV), torch.from_numpy(g["b0_actions"]).to(DEV)
    with torch.no_grad():
        assert (agent.actor(s0) - ref.actor(s0)).abs().max().item() < 1e-4
        assert (agent.target_actor(s0) - ref.target_actor(s0)).abs().max().item() < 1e-4
        for x, y in zip(agent.critic(s0, a0) + agent.target_critic(s0, a0), ref.critic(s0, a0) + ref.target_critic(s0, a0)):
            assert (x - y).abs().max().item() < 1e-4


def _one_update_from_identical_state(t, f, batch, noise, monkeypatch):
    """f.load_from(t), one update of each on the same batch and noise; returns (torch loss, fused loss, with_actor, gradient pairs)
    with the fused gradient recovered from the first moments: (m_new - beta1 m_old) / (1 - beta1)"""
    f.load_from(t)
    b1 = f.betas[0]
    m_old = [m.clone() for m in f.critic_m + f.actor_m]
    monkeypatch.setattr(torch, "randn_like", lambda x: noise.clone())
    lt = float(t.train(batch))
    monkeypatch.undo()
    lf = float(f.train(batch, noise=noise))
    with_actor = t.total_it % t.policy_freq == 0
    params = list(t.critic.parameters()) + (list(t.actor.parameters()) if with_actor else [])
    pairs = []
    for p, m0, m1 in zip(params, m_old, f.critic_m + f.actor_m):
        pairs.append((p.grad, (m1 - b1 * m0) / (1 - b1)))
    return lt, lf, with_actor, pairs


def test_fused_gradients_equal_torch_from_identical_state(monkeypatch):
    """40 consecutive updates at B = 2048 (13 of them with the actor step): before each, the fused learner takes the torch learner's
    parameters, moments and step counters; both see the same batch and noise.  The gradient the fused update applied equals the
    torch learner's .grad per tensor to 1e-4 of that tensor's largest element on at least 36 of the 40 updates, and within 5e-2 on all
    (relu boundaries, learner_gpu.assert_grads), and the losses agree to 1e-5 relative.  Gradients, not parameters: Adam's normalisation
    turns last-bit gradient differences into lr-sized parameter differences."""
    from armenv.fused_td3 import FusedTD3
    from armenv.td3 import TD3
    torch.manual_seed(0)
    t = TD3(6, 3, 0.7, device=DEV)
    f = FusedTD3(6, 3, 0.7, device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(5)
    actor_steps = tight = 0
    for it in range(40):
        batch = _batch(gen, 2048)
        noise = torch.randn(2048, 3, device=DEV, generator=gen)
        lt, lf, with_actor, pairs = _one_update_from_identical_state(t, f, batch, noise, monkeypatch)
        assert abs(lt - lf) <= 1e-5 * abs(lt), (it, lt, lf)
        tight += _assert_grads(pairs, it)
        actor_steps += with_actor
    assert actor_steps == 13
    assert tight >= 36, tight


def test_fused_td3_follows_eager_torch_free_running():
    """30 updates of each learner from the same start without the target-policy noise (its random streams differ): the tolerances of
    test_td3_update_as_hipgraph_equals_eager on the losses, Q values and actions of a held-out batch, and the actor really moved."""
    from armenv.fused_td3 import FusedTD3
    from armenv.td3 import TD3
    torch.manual_seed(3)
    a = TD3(6, 3, 0.7, device=DEV, policy_noise=0.0)
    b = FusedTD3(6, 3, 0.7, device=DEV, policy_noise=0.0)
    b.load_from(a)
    start = FusedTD3(6, 3, 0.7, device=DEV)
    start.load_from(a)
    gen = torch.Generator(device=DEV); gen.manual_seed(11)
    for it in range(30):
        batch = _batch(gen, 512)
        la, lb = float(a.train(batch)), float(b.train(batch))
        assert abs(la - lb) < 2e-3 * max(1.0, abs(la)), (it, la, lb)
    assert a.total_it == b.total_it == 30 and b.actor_step == 10
    held = _batch(gen, 512)
    with torch.no_grad():
        qa, qb = a.critic(held["states"], held["actions"]), b.critic(held["states"], held["actions"])
        assert float((qa[0] - qb[0]).abs().max()) < 5e-3 and float((qa[1] - qb[1]).abs().max()) < 5e-3
        assert float((a.actor(held["states"]) - b.actor(held["states"])).abs().max()) < 5e-3
        assert float((a.target_actor(held["states"]) - b.target_actor(held["states"])).abs().max()) < 5e-3
        tqa, tqb = a.target_critic(held["states"], held["actions"]), b.target_critic(held["states"], held["actions"])
        assert float((tqa[0] - tqb[0]).abs().max()) < 5e-3
        assert float((b.actor(held["states"]) - start.actor(held["states"])).abs().max()) > 1e-2


@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [64, 1000, 2048])
def test_fused_update_shapes(B, D, monkeypatch):
    """One update with the actor step from identical state (after two torch updates, so that the moments are not zero) for batches
    that are and are not multiples of the kernels' tiles and for the reach and push state sizes: loss to 1e-5, gradients as above."""
    from armenv.fused_td3 import FusedTD3
    from armenv.td3 import TD3
    torch.manual_seed(1)
    t = TD3(D, 3, 0.4, device=DEV)
    f = FusedTD3(D, 3, 0.4, device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(B + D)
    for _ in range(2):
        t.train(_batch(gen, B, D))
    lt, lf, with_actor, pairs = _one_update_from_identical_state(t, f, _batch(gen, B, D), torch.randn(B, 3, device=DEV, generator=gen),
                                                                 monkeypatch)
    assert with_actor and len(pairs) == 18
    assert abs(lt - lf) <= 1e-5 * abs(lt), (lt, lf)
    _assert_grads(pairs, (B, D))


def test_fused_update_is_deterministic():
    """Two fused learners with the in-kernel noise and the same seed are bitwise equal after 30 updates; another seed differs."""
    from armenv.fused_td3 import FusedTD3
    agents = []
    for seed in (7, 7, 8):
        torch.manual_seed(2)
        agents.append(FusedTD3(6, 3, 0.7, device=DEV, seed=seed))
    gen = torch.Generator(device=DEV); gen.manual_seed(3)
    losses = [[], [], []]
    for _ in range(30):
        batch = _batch(gen, 2048)
        for k, ag in enumerate(agents):
            losses[k].append(ag.train(batch))
    params = [[p for n in ag._nets() for p in n.parameters()] + ag.critic_m + ag.critic_v + ag.actor_m + ag.actor_v for ag in agents]
    assert all(torch.equal(x, y) for x, y in zip(params[0], params[1]))
    assert all(torch.equal(x, y) for x, y in zip(losses[0], losses[1]))
    assert not all(torch.equal(x, y) for x, y in zip(params[0], params[2]))
    assert all(bool(torch.isfinite(x).all()) for x in params[0])


def test_training_loop_learns_reach_with_the_fused_learner():
    """train_reach(learner="hip"): the bar of test_training_loop_learns_the_reach_task (>= 90 % success over the last log window,
    more than 5000 episodes); and train_push(learner="hip") runs with finite parameters."""
    from armenv.fused_td3 import FusedTD3
    from armenv.train import train_push, train_reach
    hist = []
    agent, _ = train_reach(iterations=140, log_every=20, log=lambda s_: hist.append(json.loads(s_)), learner="hip")
    assert isinstance(agent, FusedTD3) and agent.total_it > 0
    assert hist[-1]["success_rate"] >= 0.9 and hist[-1]["episodes"] > 5000, [round(h["success_rate"], 2) for h in hist]
    agent, hist = train_push(num_envs=256, iterations=8, rollout_steps=16, updates=4, batch_size=256, window_steps=64, max_steps=20,
                             log_every=4, log=lambda s_: None, learner="hip")
    assert isinstance(agent, FusedTD3) and agent.total_it > 0 and len(hist) == 2
    assert all(bool(torch.isfinite(p).all()) for n in agent._nets() for p in n.parameters())
    with pytest.raises(ValueError):
        train_reach(iterations=1, learner="hip", algo="daddpg")
