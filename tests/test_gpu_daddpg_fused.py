"""The fused DADDPG update (armenv_daddpg_update through armenv.fused_daddpg.FusedDADDPG) on cuda:0 against the torch learner
armenv.daddpg.DADDPG, which restates DADDPG_MLP.update (the reference's algo/DADDPG/DADDPG_mlp.py:117-171): the reference's golden
run (G16), the alternation of the two actors bit for bit, gradients against float64 autograd, free-running agreement, batch / state
sizes, determinism across runs and streams, and the training loop with learner="fused"."""
import json

import numpy as np
import pytest
import torch

import learner_gpu as G
from conftest import golden_npz
from learner_gpu import DEV, assert_grads as _assert_grads, batch as _batch, f64_net as _f64, to_numpy as _np

pytestmark = pytest.mark.gpu
NETS = ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic")


def _state(f):
    return G.state(f, NETS, NETS[:3])


def test_fused_daddpg_reproduces_the_golden_updates():
    """G16 on the fused path: the reference's eight DADDPG_MLP.update calls (B = 64) from torch.manual_seed(0)'s initial weights;
    the tolerances of test_fused_td3_reproduces_the_golden_updates; the three optimisers' step counters."""
    from armenv.daddpg import DADDPG
    from armenv.fused_daddpg import FusedDADDPG
    g = golden_npz("daddpg_train_seed0.npz")
    torch.manual_seed(0)
    cpu = DADDPG(6, 3, 0.7, device="cpu")
    torch.manual_seed(0)
    agent = FusedDADDPG(6, 3, 0.7, device=DEV)
    for a, b in zip(agent._nets(), cpu._nets()):                 # same constructor order: same initial weights
        for k, v in a.state_dict().items():
            assert torch.equal(v.cpu(), b.state_dict()[k]), k
    for i, want in enumerate(g["losses"]):
        b = {k: torch.from_numpy(g[f"b{i}_{k}"]).to(DEV) for k in ("states", "actions", "next_states", "rewards", "dones")}
        loss = float(agent.train(b))
        assert abs(loss - want) < 2e-5 * max(1.0, abs(want)), (i, loss, want)
    assert agent.total_it == 8 and agent.critic_step == 8 and agent.actor1_step == 4 and agent.actor2_step == 4
    ref = DADDPG(6, 3, 0.7, device=DEV)
    names = ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic")
    for name in names:
        net, rnet = getattr(agent, name), getattr(ref, name)
        rnet.load_state_dict({k: torch.from_numpy(g[f"{name}__{k.replace('.', '_')}"]) for k in net.state_dict()})
        for k, v in net.state_dict().items():
            d = np.abs(_np(v) - g[f"{name}__{k.replace('.', '_')}"])
            assert (d < 2e-5).mean() > 0.999 and d.max() < 7e-3, (name, k, (d < 2e-5).mean(), d.max())
    s0, a0 = torch.from_numpy(g["b0_states"]).to(DEV), torch.from_numpy(g["b0_actions"]).to(DEV)
    with torch.no_grad():
        for name in ("actor1", "actor2", "target_actor1", "target_actor2"):
            assert (getattr(agent, name)(s0) - getattr(ref, name)(s0)).abs().max().item() < 1e-4, name
        for name in ("critic", "target_critic"):
            assert (getattr(agent, name)(s0, a0) - getattr(ref, name)(s0, a0)).abs().max().item() < 1e-4, name


def test_fused_daddpg_alternates_the_actors_exactly():
    """Update n (total_it after the increment) steps actor 1 when n is even and actor 2 when n is odd: everything the other branch
    owns is bitwise unchanged by the update -- actor 2, its moments, target_actor2 and target_critic on even updates; actor 1, its
    moments and target_actor1 on odd ones -- and what the branch owns has moved."""
    from armenv.fused_daddpg import FusedDADDPG
    torch.manual_seed(4)
    f = FusedDADDPG(6, 3, 0.7, device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(4)
    for _ in range(6):
        before = _state(f)
        f.train(_batch(gen, 512))
        after = _state(f)
        even = f.total_it % 2 == 0
        still = ("actor2.", "actor2_m.", "actor2_v.", "target_actor2.", "target_critic.") if even else \
                ("actor1.", "actor1_m.", "actor1_v.", "target_actor1.")
        moved = ("actor1.", "actor1_m.", "target_actor1.") if even else ("actor2.", "actor2_m.", "target_actor2.", "target_critic.")
        for k in before:
            if k.startswith(still):
                assert torch.equal(before[k], after[k]), (f.total_it, k)
            if k.startswith(moved + ("critic.", "critic_m.", "critic_v.")):
                assert not torch.equal(before[k], after[k]), (f.total_it, k)
    assert f.critic_step == 6 and f.actor1_step == 3 and f.actor2_step == 3


def test_fused_daddpg_gradients_equal_float64_autograd():
    """With beta1 = 0 the first moments after an update ARE the gradients it applied.  Six updates at B = 2048, three of each
    parity, from a state with non-trivial parameters and moments: the critic's gradient equals float64 autograd of
    mean((critic(s, a) - target)^2) over the parameters before the update, and the stepped actor's equals float64 autograd of
    -mean(critic'(s, actor(s))) with the critic the fused update stepped (critic') -- per tensor to 1e-4 of its largest element except
    at relu-boundary flips (_assert_grads: within 5e-2 always, 1e-4 on at least four of the six updates); losses to 1e-5 relative."""
    from armenv.daddpg import DADDPG
    from armenv.fused_daddpg import FusedDADDPG
    torch.manual_seed(0)
    t = DADDPG(6, 3, 0.7, device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(9)
    for _ in range(3):
        t.train(_batch(gen, 2048))
    f = FusedDADDPG(6, 3, 0.7, device=DEV)
    f.load_from(t)
    f.betas = (0.0, 0.999)
    tight, parities = 0, set()
    for it in range(6):
        batch = _batch(gen, 2048)
        before = {n: _f64(getattr(f, n)) for n in ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic")}
        lf = float(f.train(batch))
        k = 1 if f.total_it % 2 == 0 else 2
        parities.add(k)
        s, a, s2 = (batch[x].double() for x in ("states", "actions", "next_states"))
        r, d = batch["rewards"].double().view(-1, 1), batch["dones"].double().view(-1, 1)
        with torch.no_grad():
            tq = torch.min(before["target_critic"](s2, before["target_actor1"](s2)), before["target_critic"](s2, before["target_actor2"](s2)))
            target = r + (1 - d) * f.gamma * tq
        closs = ((before["critic"](s, a) - target) ** 2).mean()
        lt = float(closs.detach())
        assert abs(lt - lf) <= 1e-5 * abs(lt), (it, lt, lf)
        pairs = list(zip(torch.autograd.grad(closs, list(before["critic"].parameters())), f.critic_m))
        stepped = _f64(f.critic)
        actor = before["actor%d" % k]
        aloss = -stepped(s, actor(s)).mean()
        pairs += list(zip(torch.autograd.grad(aloss, list(actor.parameters())), getattr(f, "actor%d_m" % k)))
        tight += _assert_grads([(g64, gf.double()) for g64, gf in pairs], (it, k))
    assert parities == {1, 2} and tight >= 4, tight


def test_fused_daddpg_follows_eager_torch_free_running():
    """40 updates of each learner at B = 2048 from the same start: losses within 5e-3, and the six nets within 1e-2 on a held-out
    batch (the tolerances of test_training_loop_daddpg_default_agent: Adam turns last-bit gradient differences into lr-sized parameter
    differences); the actors really moved."""
    from armenv.daddpg import DADDPG
    from armenv.fused_daddpg import FusedDADDPG
    torch.manual_seed(3)
    a = DADDPG(6, 3, 0.7, device=DEV)
    b = FusedDADDPG(6, 3, 0.7, device=DEV)
    b.load_from(a)
    start = FusedDADDPG(6, 3, 0.7, device=DEV)
    start.load_from(a)
    gen = torch.Generator(device=DEV); gen.manual_seed(11)
    for it in range(40):
        batch = _batch(gen, 2048)
        la, lb = float(a.train(batch)), float(b.train(batch))
        assert abs(la - lb) < 5e-3 * max(1.0, abs(la)), (it, la, lb)
    assert a.total_it == b.total_it == 40 and b.critic_step == 40 and b.actor1_step == b.actor2_step == 20
    held = _batch(gen, 2048)
    s, act = held["states"], held["actions"]
    with torch.no_grad():
        for name in ("actor1", "actor2", "target_actor1", "target_actor2"):
            assert float((getattr(a, name)(s) - getattr(b, name)(s)).abs().max()) < 1e-2, name
        for name in ("critic", "target_critic"):
            assert float((getattr(a, name)(s, act) - getattr(b, name)(s, act)).abs().max()) < 1e-2, name
        for name in ("actor1", "actor2"):
            assert float((getattr(b, name)(s) - getattr(start, name)(s)).abs().max()) > 1e-2, name


@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [1, 64, 1000, 2048, 4097])
def test_fused_daddpg_update_shapes(B, D):
    """One update from identical state (after one or two torch updates: both parities occur, moments are not zero) for batches that
    are and are not multiples of the kernels' tiles and slices, and for the reach and push state sizes: loss to 1e-5 relative, the
    applied gradients against the torch learner's .grad as in _assert_grads.  Both learners keep beta1 = 0.9 (the actor's gradient
    depends on the STEPPED critic), so the fused gradient is recovered from the first moments: (m_new - beta1 m_old) / (1 - beta1)."""
    from armenv.daddpg import DADDPG
    from armenv.fused_daddpg import FusedDADDPG
    torch.manual_seed(1)
    t = DADDPG(D, 3, 0.4, device=DEV)
    f = FusedDADDPG(D, 3, 0.4, device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(B + D)
    for _ in range(2 if B % 2 else 1):
        t.train(_batch(gen, B, D))
    f.load_from(t)
    b1 = f.betas[0]
    k = 1 if (t.total_it + 1) % 2 == 0 else 2
    m_old = [m.clone() for m in f.critic_m + getattr(f, "actor%d_m" % k)]
    batch = _batch(gen, B, D)
    lt, lf = float(t.train(batch)), float(f.train(batch))
    assert abs(lt - lf) <= 1e-5 * max(abs(lt), 1e-6), (lt, lf)
    params = list(t.critic.parameters()) + list(getattr(t, "actor%d" % k).parameters())
    pairs = [(p.grad, (m1 - b1 * m0) / (1 - b1)) for p, m0, m1 in zip(params, m_old, f.critic_m + getattr(f, "actor%d_m" % k))]
    assert len(pairs) == 12
    _assert_grads(pairs, (B, D, k))


def test_fused_daddpg_is_deterministic_across_runs_and_streams():
    """Three learners from the same state, ten updates on the same batches, two on the default stream and one on a side stream:
    parameters, moments and losses are bitwise equal."""
    from armenv.fused_daddpg import FusedDADDPG
    agents = []
    for _ in range(3):
        torch.manual_seed(2)
        agents.append(FusedDADDPG(6, 3, 0.7, device=DEV))
    side = torch.cuda.Stream(device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(3)
    losses = [[], [], []]
    for _ in range(10):
        batch = _batch(gen, 2048)
        for k in (0, 1):
            losses[k].append(agents[k].train(batch))
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            losses[2].append(agents[2].train(batch))
            for v in batch.values():
                v.record_stream(side)
        torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    states = [_state(ag) for ag in agents]
    for k in (1, 2):
        assert all(torch.equal(states[0][n], states[k][n]) for n in states[0]), k
        assert all(torch.equal(x, y) for x, y in zip(losses[0], losses[k])), k
    assert all(bool(torch.isfinite(v).all()) for v in states[0].values())


def test_training_loop_learns_reach_with_the_fused_daddpg_learner():
    """train_reach(algo="daddpg", learner="fused"): the bar of test_training_loop_learns_the_reach_task (>= 90 % success over the
    last log window, more than 5000 episodes); and train_push(algo="daddpg", learner="fused") runs with finite parameters."""
    from armenv.fused_daddpg import FusedDADDPG
    from armenv.train import train_push, train_reach
    hist = []
    agent, _ = train_reach(iterations=140, log_every=20, log=lambda s_: hist.append(json.loads(s_)), algo="daddpg", learner="fused")
    assert isinstance(agent, FusedDADDPG) and agent.total_it > 0
    assert hist[-1]["success_rate"] >= 0.9 and hist[-1]["episodes"] > 5000, [round(h["success_rate"], 2) for h in hist]
    agent, hist = train_push(num_envs=256, iterations=8, rollout_steps=16, updates=4, batch_size=256, window_steps=64, max_steps=20,
                             log_every=4, log=lambda s_: None, algo="daddpg", learner="fused")
    assert isinstance(agent, FusedDADDPG) and agent.total_it > 0 and len(hist) == 2
    assert all(bool(torch.isfinite(p).all()) for n in agent._nets() for p in n.parameters())
