"""The fused DATD3 / DARC update (armenv_datd3_update through armenv.fused_datd3.FusedDATD3 / FusedDARC) on cuda:0 against the torch
learners armenv.datd3.DATD3 / DARC, which restate DATD3_MLP.update / DARC_MLP.update (the reference's algo/DATD3/DATD3_mlp.py:146-211,
algo/DARC/DARC_mlp.py:140-222): the reference's recorded runs (G17, G18), gradients against float64 autograd (with a control that
the regulariser is exercised), which tensors an update owns bit for bit, the in-kernel noise, free-running agreement, batch / state
sizes, determinism across runs and streams, the call under hipGraph capture, and the training loop with all three learner paths.
Each test is its counterpart in test_gpu_daddpg_fused.py with the same tolerances unless its docstring says otherwise."""
import copy
import json

import numpy as np
import pytest
import torch

import learner_gpu as G
from datd3_golden import KEYS, NETS, expected_losses, load_train_fixture
from learner_gpu import DEV, assert_grads as _assert_grads, batch as _batch, f64_net as _f64, to_numpy as _np

pytestmark = pytest.mark.gpu
ALGOS = ["datd3", "darc"]
REACH_ITERATIONS = 140


def _learners(algo):
    from armenv.datd3 import DARC, DATD3
    from armenv.fused_datd3 import FusedDARC, FusedDATD3
    return (DARC, FusedDARC) if algo == "darc" else (DATD3, FusedDATD3)


def _noise(gen, B):
    return torch.randn(B, 3, device=DEV, generator=gen)


def _state(f):
    return G.state(f, NETS, NETS[:4])


def _steps(f):
    return (f.critic1_step, f.critic2_step, f.actor1_step, f.actor2_step)


@pytest.mark.parametrize("algo", ALGOS)
def test_fused_update_reproduces_the_golden_updates(algo):
    """G17 / G18 on the fused path with the recorded noise through noise_dev: the reference's eight updates (B = 64) from
    torch.manual_seed(0)'s initial weights: losses 2e-5 relative, >= 99.9 % of each tensor's elements within 2e-5 and none beyond
    7e-3, forward values of all eight nets on batch 0 within 1e-4, the four optimisers' step counters 4 / 4 / 4 / 4."""
    T, F = _learners(algo)
    darc = algo == "darc"
    g = load_train_fixture(algo + "_train_seed0")
    torch.manual_seed(0)
    cpu = T(6, 3, 0.7, device="cpu")
    torch.manual_seed(0)
    agent = F(6, 3, 0.7, device=DEV)
    for a, b in zip(agent._nets(), cpu._nets()):                 # same constructor order: same initial weights
        for k, v in a.state_dict().items():
            assert torch.equal(v.cpu(), b.state_dict()[k]), k
    got = []
    for i in range(4):
        b = {k: torch.from_numpy(g[f"b{i}_{k}"]).to(DEV) for k in KEYS}
        noise = tuple(torch.from_numpy(g["noise"][2 * i + j]).to(DEV) for j in (0, 1))
        got += [float(x) for x in agent.train(b, noise=noise)]
    for i, (have, want) in enumerate(zip(got, expected_losses(g, darc))):
        print(algo, "update", i, "loss", have, "recorded", want)
        assert abs(have - want) < 2e-5 * max(1.0, abs(want)), (i, have, want)
    assert agent.total_it == 8 and _steps(agent) == (4, 4, 4, 4)
    ref = T(6, 3, 0.7, device=DEV)
    for name in NETS:
        net, rnet = getattr(agent, name), getattr(ref, name)
        rnet.load_state_dict({k: torch.from_numpy(g[f"{name}__{k.replace('.', '_')}"]) for k in net.state_dict()})
        for k, v in net.state_dict().items():
            d = np.abs(_np(v) - g[f"{name}__{k.replace('.', '_')}"])
            print(algo, name, k, "within 2e-5:", (d < 2e-5).mean(), "max", d.max())
            assert (d < 2e-5).mean() >= 0.999 and d.max() <= 7e-3, (name, k, (d < 2e-5).mean(), d.max())
    s0, a0 = torch.from_numpy(g["b0_states"]).to(DEV), torch.from_numpy(g["b0_actions"]).to(DEV)
    with torch.no_grad():
        for name in NETS:
            x = (s0,) if "actor" in name else (s0, a0)
            err = (getattr(agent, name)(*x) - getattr(ref, name)(*x)).abs().max().item()
            print(algo, name, "forward error on batch 0", err)
            assert err < 1e-4, (name, err)


def _critic_loss64(before, f, batch, noise, k, darc, w):
    """float64 autograd restatement of the stepped critic's loss over the nets `before` the update"""
    s, a, s2 = (batch[x].double() for x in ("states", "actions", "next_states"))
    r, d = batch["rewards"].double().view(-1, 1), batch["dones"].double().view(-1, 1)
    with torch.no_grad():
        nz = (noise.double() * f.policy_noise).clamp(-f.noise_clip, f.noise_clip)
        a2 = [(before["target_actor%d" % j](s2) + nz).clamp(-f.action_bound, f.action_bound) for j in (1, 2)]
        t = torch.min(before["target_critic1"](s2, a2[0]), before["target_critic2"](s2, a2[1]))
        if darc:
            t = f.q_weight * t + (1.0 - f.q_weight) * t
        target = r + (1 - d) * f.gamma * t
    q = before["critic%d" % k](s, a)
    loss = ((q - target) ** 2).mean()
    if w:
        loss = loss + w * ((q - before["critic%d" % (3 - k)](s, a).detach()) ** 2).mean()
    return loss


def _grad_run(algo, w, ref_w):
    """Eight updates (k = 1, 2, 1, 2, ...) at B = 2048 with beta1 = 0, so the first moments after an update ARE the gradients it
    applied; the float64 reference uses regulariser weight `ref_w`.  Returns (number of updates whose every tensor is within the tight
    bound, number of updates).  _assert_grads raises when a tensor is beyond the loose bound."""
    T, F = _learners(algo)
    darc = algo == "darc"
    kw = dict(regularization_weight=w) if darc else {}
    torch.manual_seed(0)
    t = T(6, 3, 0.7, device=DEV, **kw)
    gen = torch.Generator(device=DEV); gen.manual_seed(9)
    for _ in range(2):
        t.train(_batch(gen, 2048))
    f = F(6, 3, 0.7, device=DEV, **kw)
    f.load_from(t)
    f.betas = (0.0, 0.999)
    tight = 0
    for it in range(8):
        k = 1 + it % 2
        batch, noise = _batch(gen, 2048), _noise(gen, 2048)
        before = {n: _f64(getattr(f, n)) for n in NETS}
        lf = float(f.update(batch, k == 1, noise))
        closs = _critic_loss64(before, f, batch, noise, k, darc, ref_w)
        lt = float(closs.detach())
        if ref_w == w:
            assert abs(lt - lf) <= 1e-5 * abs(lt), (it, lt, lf)
        pairs = list(zip(torch.autograd.grad(closs, list(before["critic%d" % k].parameters())), getattr(f, "critic%d_m" % k)))
        stepped = _f64(getattr(f, "critic%d" % k))
        actor = before["actor%d" % k]
        s = batch["states"].double()
        aloss = -stepped(s, actor(s)).mean()
        pairs += list(zip(torch.autograd.grad(aloss, list(actor.parameters())), getattr(f, "actor%d_m" % k)))
        assert len(pairs) == 12
        tight += _assert_grads([(g64, gf.double()) for g64, gf in pairs], (algo, it, k))
    return tight, 8


@pytest.mark.parametrize("algo", ALGOS)
def test_fused_gradients_equal_float64_autograd(algo):
    """Gradients from identical states for k = 1 and k = 2 at B = 2048, darc 0 and 1, against float64 autograd over the parameters
    before the update (the actor's with the critic the fused update stepped): the DADDPG test's bounds -- per tensor to 1e-4 of its
    largest element except at relu-boundary flips (_assert_grads: within 5e-2 always, 1e-4 on at least two thirds of the updates, as
    DADDPG's four of six) -- and losses to 1e-5 relative."""
    w = 0.005 if algo == "darc" else 0.0          # DATD3 has no regulariser
    tight, n = _grad_run(algo, w, w)
    print(algo, "updates within the tight bound:", tight, "of", n)
    assert 3 * tight >= 2 * n, tight


def test_darc_regulariser_is_exercised_by_the_gradient_check():
    """Control: the float64 reference WITHOUT the regulariser must FAIL the comparison the test above passes (fewer than two thirds
    of the updates within the tight bound, or a tensor outside the loose one), at the default weight w = 0.005: 2 w / B (q - q_other)
    against 2 / B (q - y) is a share of w |q - q_other| / |q - y| of the critic's delta, far above the bound's 1e-4 once the two
    critics differ by a few percent of the TD error, which two differently initialised critics do."""
    w = 0.005
    try:
        tight, n = _grad_run("darc", w, 0.0)
    except AssertionError:
        return                       # beyond the loose bound: failed, as it must
    print("darc, float64 reference without the regulariser at w =", w, ": updates within the tight bound:", tight, "of", n)
    assert 3 * tight < 2 * n, tight


@pytest.mark.parametrize("algo", ALGOS)
def test_fused_update_owns_its_actor_and_critic_only(algo):
    """update(k) leaves everything of the other index bitwise unchanged -- the other actor, the other critic (DARC reads it), their
    moments and their targets -- and what it owns has moved; the step counters follow."""
    _, F = _learners(algo)
    torch.manual_seed(4)
    f = F(6, 3, 0.7, device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(4)
    for k in (1, 2, 2, 1, 1, 2):
        before = _state(f)
        f.update(_batch(gen, 512), k == 1)
        after = _state(f)
        o = 3 - k
        names = ("actor%d.", "actor%d_m.", "actor%d_v.", "critic%d.", "critic%d_m.", "critic%d_v.", "target_actor%d.", "target_critic%d.")
        still, moved = tuple(n % o for n in names), tuple(n % k for n in names)
        for key in before:
            if key.startswith(still):
                assert torch.equal(before[key], after[key]), (k, key)
            if key.startswith(moved):
                assert not torch.equal(before[key], after[key]), (k, key)
    assert f.total_it == 6 and _steps(f) == (3, 3, 3, 3)


def test_in_kernel_noise_is_keyed_by_seed_and_draw_and_shared_by_both_proposals():
    """Same (seed, draw) -> bitwise equal updates, another seed differs.  That both proposals of a row received the same noise is
    read off the update itself: with zeroed target-actor fc3 layers, a large action_bound and a wide clip the proposals ARE the noise
    each received, a2_j = n_j.  Target critic 1 values proposal 1 and target critic 2 proposal 2, so T = min(X(n_1), Y(n_2)) with the
    target critics X, Y -- and min(Y(n_1), X(n_2)) with the two exchanged.  The two are equal in every row exactly when n_1 = n_2
    (X and Y are different random nets), and then the loss, critic 1, its moments and actor 1 after update 1 are bitwise equal
    between the two arrangements.  The noise is really applied: policy_noise = 0 gives another loss."""
    from armenv.fused_datd3 import FusedDATD3
    agents = []
    for seed in (7, 7, 8):
        torch.manual_seed(2)
        agents.append(FusedDATD3(6, 3, 0.7, device=DEV, seed=seed))
    gen = torch.Generator(device=DEV); gen.manual_seed(3)
    for _ in range(5):
        batch = _batch(gen, 1000)
        for ag in agents:
            ag.train(batch)
    s = [_state(ag) for ag in agents]
    assert all(torch.equal(s[0][n], s[1][n]) for n in s[0])
    assert any(not torch.equal(s[0][n], s[2][n]) for n in s[0] if n.startswith("critic1."))

    B = 777
    batch = _batch(gen, B)

    def run(exchanged, policy_noise=1.0):
        torch.manual_seed(5)
        f = FusedDATD3(6, 3, 100.0, device=DEV, seed=11, noise_clip=50.0, policy_noise=policy_noise)
        with torch.no_grad():
            for n in (f.target_actor1, f.target_actor2):
                n.fc3.weight.zero_(); n.fc3.bias.zero_()
            if exchanged:
                x, y = copy.deepcopy(f.target_critic1.state_dict()), copy.deepcopy(f.target_critic2.state_dict())
                f.target_critic1.load_state_dict(y); f.target_critic2.load_state_dict(x)
        loss = f.update(batch, True)
        return loss, _state(f)
    (la, a), (lb, b) = run(False), run(True)
    assert not torch.equal(a["target_critic2.fc1.weight"], b["target_critic2.fc1.weight"])       # the exchange took place
    assert torch.equal(la, lb)
    own = ("critic1.", "critic1_m.", "critic1_v.", "actor1.", "actor1_m.", "actor1_v.", "target_actor1.")
    assert all(torch.equal(a[n], b[n]) for n in a if n.startswith(own))
    assert not torch.equal(run(False, policy_noise=0.0)[0], la)


@pytest.mark.parametrize("algo", ALGOS)
def test_fused_learner_follows_eager_torch_free_running(algo):
    """40 train calls (80 updates) of each learner at B = 2048 from the same start with shared noise: losses within 5e-3, the eight
    nets within 1e-2 on a held-out batch (test_fused_daddpg_follows_eager_torch_free_running's tolerances); the actors really moved."""
    T, F = _learners(algo)
    torch.manual_seed(3)
    a = T(6, 3, 0.7, device=DEV)
    b = F(6, 3, 0.7, device=DEV)
    b.load_from(a)
    start = F(6, 3, 0.7, device=DEV)
    start.load_from(a)
    gen = torch.Generator(device=DEV); gen.manual_seed(11)
    for it in range(40):
        batch, noise = _batch(gen, 2048), (_noise(gen, 2048), _noise(gen, 2048))
        la, lb = a.train(batch, noise=noise), b.train(batch, noise=noise)
        for x, y in zip(la, lb):
            assert abs(float(x) - float(y)) < 5e-3 * max(1.0, abs(float(x))), (it, float(x), float(y))
    assert a.total_it == b.total_it == 80 and _steps(b) == (40, 40, 40, 40)
    held = _batch(gen, 2048)
    s, act = held["states"], held["actions"]
    with torch.no_grad():
        for name in NETS:
            x = (s,) if "actor" in name else (s, act)
            assert float((getattr(a, name)(*x) - getattr(b, name)(*x)).abs().max()) < 1e-2, name
        for name in ("actor1", "actor2"):
            assert float((getattr(b, name)(s) - getattr(start, name)(s)).abs().max()) > 1e-2, name


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [1, 64, 1000, 2048, 4097])
def test_fused_update_shapes(B, D, algo):
    """One train (k = 1 then k = 2) from identical state (after one torch train: moments are not zero) for batches that are and are
    not multiples of the kernels' tiles and slices, and for the reach and push state sizes: losses to 1e-5 relative, the applied
    gradients against the torch learner's .grad as in _assert_grads.  Both learners keep beta1 = 0.9, so the fused gradient is
    recovered from the first moments: (m_new - beta1 m_old) / (1 - beta1).  Before update 2 the fused learner takes the torch
    learner's state again, so each update is compared from identical states."""
    T, F = _learners(algo)
    torch.manual_seed(1)
    t = T(D, 3, 0.4, device=DEV)
    f = F(D, 3, 0.4, device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(B + D)
    t.train(_batch(gen, B, D))
    b1 = f.betas[0]
    batch = _batch(gen, B, D)
    for k in (1, 2):
        f.load_from(t)
        noise = _noise(gen, B)
        m_old = [m.clone() for m in getattr(f, "critic%d_m" % k) + getattr(f, "actor%d_m" % k)]
        lt, lf = float(t.update(batch, k == 1, noise)), float(f.update(batch, k == 1, noise))
        assert abs(lt - lf) <= 1e-5 * max(abs(lt), 1e-6), (k, lt, lf)
        params = list(getattr(t, "critic%d" % k).parameters()) + list(getattr(t, "actor%d" % k).parameters())
        m_new = getattr(f, "critic%d_m" % k) + getattr(f, "actor%d_m" % k)
        pairs = [(p.grad, (m1 - b1 * m0) / (1 - b1)) for p, m0, m1 in zip(params, m_old, m_new)]
        assert len(pairs) == 12
        _assert_grads(pairs, (B, D, k))


@pytest.mark.parametrize("algo", ALGOS)
def test_fused_update_is_deterministic_across_runs_and_streams(algo):
    """Three learners from the same state, ten train calls on the same batches with the in-kernel noise, two on the default stream
    and one on a side stream: parameters, moments and losses are bitwise equal."""
    _, F = _learners(algo)
    agents = []
    for _ in range(3):
        torch.manual_seed(2)
        agents.append(F(6, 3, 0.7, device=DEV, seed=5))
    side = torch.cuda.Stream(device=DEV)
    gen = torch.Generator(device=DEV); gen.manual_seed(3)
    losses = [[], [], []]
    for _ in range(10):
        batch = _batch(gen, 2048)
        for k in (0, 1):
            losses[k] += list(agents[k].train(batch))
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            losses[2] += list(agents[2].train(batch))
            for v in batch.values():
                v.record_stream(side)
        torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    states = [_state(ag) for ag in agents]
    for k in (1, 2):
        assert all(torch.equal(states[0][n], states[k][n]) for n in states[0]), k
        assert all(torch.equal(x, y) for x, y in zip(losses[0], losses[k])), k
    assert all(bool(torch.isfinite(v).all()) for v in states[0].values())


@pytest.mark.parametrize("algo", ALGOS)
def test_fused_update_captured_in_a_graph_equals_direct_calls(algo):
    """armenv_datd3_update (k = 1) captured into a torch.cuda.graph and replayed twice equals two direct calls with the same
    arguments, bit for bit: the call only enqueues kernels (one serial chain: no parallel branches).  The captured arguments are fixed
    (step numbers 1 / 1, draw 1), so the direct calls repeat them."""
    import ctypes as C
    from armenv import _lib as L
    _, F = _learners(algo)
    gen = torch.Generator(device=DEV); gen.manual_seed(6)
    batch = _batch(gen, 2048)
    noise = _noise(gen, 2048)
    lib = L.load()

    def prepared():
        torch.manual_seed(8)
        f = F(6, 3, 0.7, device=DEV)
        inputs = f._inputs(batch)
        s, a, r, s2, d = inputs
        args = f._static_args()
        ws = f._workspace(2048)
        loss = torch.zeros((), device=DEV)
        args.batch, args.update_actor, args.critic_step, args.actor_step, args.draw = 2048, 1, 1, 1, 1
        args.noise_dev = noise.data_ptr()
        args.states_dev, args.actions_dev, args.next_states_dev = s.data_ptr(), a.data_ptr(), s2.data_ptr()
        args.rewards_dev, args.dones_dev, args.loss_dev = r.data_ptr(), d.data_ptr(), loss.data_ptr()
        args.workspace_dev, args.workspace_bytes = ws.data_ptr(), ws.numel()
        call = lambda: L.check(lib.armenv_datd3_update(C.byref(args), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
        return f, call, loss, inputs

    direct, call_d, loss_d, keep_d = prepared()
    call_d(); call_d()
    graphed, call_g, loss_g, keep_g = prepared()
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    before = _state(graphed)
    with torch.cuda.graph(g):
        call_g()
    torch.cuda.synchronize(DEV)
    after = _state(graphed)
    assert all(torch.equal(before[n], after[n]) for n in before)       # capture enqueues nothing
    g.replay(); g.replay()
    torch.cuda.synchronize(DEV)
    a, b = _state(direct), _state(graphed)
    assert all(torch.equal(a[n], b[n]) for n in a) and torch.equal(loss_d, loss_g)
    assert not torch.equal(before["critic1.fc1.weight"], b["critic1.fc1.weight"])


def _reach(algo, learner):
    from armenv.train import train_reach
    hist = []
    agent, _ = train_reach(iterations=REACH_ITERATIONS, log_every=20, log=lambda s_: hist.append(json.loads(s_)), algo=algo,
                           learner=learner)
    print(algo, learner, [round(h["success_rate"], 3) for h in hist])
    assert agent.total_it > 0
    assert hist[-1]["success_rate"] >= 0.9 and hist[-1]["episodes"] > 5000, [round(h["success_rate"], 2) for h in hist]
    return agent


@pytest.mark.parametrize("algo", ALGOS)
def test_training_loop_learns_reach_with_the_fused_learner(algo):
    """train_reach(algo, learner="fused"): the bar of the TD3 / DADDPG learning tests (>= 90 % success over the last log window of
    140 iterations, more than 5000 episodes); and train_push runs with finite parameters."""
    from armenv.train import train_push
    _, F = _learners(algo)
    assert isinstance(_reach(algo, "fused"), F)
    agent, hist = train_push(num_envs=256, iterations=8, rollout_steps=16, updates=4, batch_size=256, window_steps=64, max_steps=20,
                             log_every=4, log=lambda s_: None, algo=algo, learner="fused")
    assert isinstance(agent, F) and agent.total_it > 0 and len(hist) == 2
    assert all(bool(torch.isfinite(p).all()) for n in agent._nets() for p in n.parameters())


@pytest.mark.parametrize("algo", ALGOS)
def test_training_loop_learns_reach_with_the_graphed_torch_learner(algo):
    """train_reach(algo, learner="torch") with the update replayed from hipGraphs (two replays per train_graphed): the same bar."""
    T, _ = _learners(algo)
    assert isinstance(_reach(algo, "torch"), T)
