"""The population TD3 update (armenv_td3_pop_update through armenv.fused_td3_pop.FusedTD3Population) on cuda:0.  Its oracle is the
single-learner update: every sum of the update has one fixed order that does not depend on the grid, so member p of a population
update equals armenv_td3_update (armenv.fused_td3.FusedTD3) on member p's tensors BIT FOR BIT -- no tolerance anywhere below."""
import ctypes as C
import json

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NETS = ("actor", "q1", "q2", "target_actor", "target_q1", "target_q2", "actor_m", "actor_v", "q1_m", "q1_v", "q2_m", "q2_v")


def _batch(gen, P, B, D):
    r = lambda *shape: torch.rand(*shape, device=DEV, generator=gen)
    return dict(states=r(P, B, D), actions=r(P, B, 3) * 1.4 - 0.7, next_states=r(P, B, D), rewards=r(P, B) - 0.5,
                dones=(r(P, B) < 0.1).to(torch.uint8))


def _member_batch(batch, p):
    return {k: v[p] for k, v in batch.items()}


def _randomise(pop, gen):
    """different random nets, targets and (valid: v >= 0) moments for every member"""
    for name in NETS:
        for t in pop.stacks[name]:
            x = torch.randn(t.shape, device=DEV, generator=gen) * 0.1
            t.copy_(x.abs() * 1e-3 if name.endswith("_v") else x * (0.01 if name.endswith("_m") else 1.0))


def _state(pop, p):
    return pop._member_state(p)


def _single_state(agent):
    from armenv.fused_td3_pop import FusedTD3Population
    return FusedTD3Population._single_state(agent)


def _population(P, D, gen, seed=11, **kw):
    from armenv.fused_td3_pop import FusedTD3Population
    pop = FusedTD3Population(P, D, 3, 0.7, device=DEV, seed=seed, **kw)
    if gen is not None:
        _randomise(pop, gen)
    pop.total_it, pop.critic_step, pop.actor_step = 4, 4, 1        # mid-run: bias corrections that are not those of step 1
    return pop


@pytest.mark.parametrize("given_noise", [True, False], ids=["noise_given", "noise_in_kernel"])
@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [1, 64, 257, 1000])
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_every_member_equals_the_single_update_bit_for_bit(P, B, D, given_noise):
    """Six consecutive updates (total_it 5..10: two with the actor step) of P members with different random nets, moments and
    batches.  After every update each of member p's 72 tensors and loss[p] equals a FusedTD3 that started from member p's state,
    has seed + p, and was stepped by armenv_td3_update on member p's batch (and member p's noise, when given)."""
    gen = torch.Generator(device=DEV); gen.manual_seed(1000 * P + B + D)
    pop = _population(P, D, gen)
    singles = [pop.export_member(p) for p in range(P)]
    assert [s.seed for s in singles] == [11 + p for p in range(P)] and singles[0].total_it == 4
    actor_steps = 0
    for it in range(6):
        batch = _batch(gen, P, B, D)
        noise = torch.randn(P, B, 3, device=DEV, generator=gen) if given_noise else None
        loss = pop.train(batch, noise=noise)
        assert tuple(loss.shape) == (P,)
        actor_steps += pop.total_it % pop.policy_freq == 0
        for p, single in enumerate(singles):
            ls = single.train(_member_batch(batch, p), noise=None if noise is None else noise[p])
            assert torch.equal(ls, loss[p]), (it, p, float(ls), float(loss[p]))
            bad = [k for k, (x, y) in enumerate(zip(_state(pop, p), _single_state(single))) if not torch.equal(x, y)]
            assert not bad, (it, p, bad)
    assert actor_steps == 2 and pop.actor_step == 3 and pop.critic_step == 10
    assert all(bool(torch.isfinite(t).all()) for six in pop.stacks.values() for t in six)
    if P > 1:
        assert not torch.equal(pop.stacks["actor"][0][0], pop.stacks["actor"][0][1])


def _run(P, B, D, batches, noises, seed_gen=3):
    gen = torch.Generator(device=DEV); gen.manual_seed(seed_gen)
    pop = _population(P, D, gen)
    losses = [pop.train(b, noise=n) for b, n in zip(batches, noises)]
    return pop, torch.stack(losses)


def test_members_do_not_leak_into_each_other():
    """Three updates twice, the second time with member 1's batch perturbed: members 0 and 2 are bit-identical to the first run and
    member 1 is not."""
    P, B, D = 3, 257, 6
    gen = torch.Generator(device=DEV); gen.manual_seed(21)
    batches = [_batch(gen, P, B, D) for _ in range(3)]
    noises = [torch.randn(P, B, 3, device=DEV, generator=gen) for _ in range(3)]
    a, la = _run(P, B, D, batches, noises)
    perturbed = [{k: v.clone() for k, v in b.items()} for b in batches]
    for b in perturbed:
        b["states"][1] += 0.125
        b["rewards"][1] -= 0.5
    c, lc = _run(P, B, D, perturbed, noises)
    for p in (0, 2):
        assert all(torch.equal(x, y) for x, y in zip(_state(a, p), _state(c, p))), p
        assert torch.equal(la[:, p], lc[:, p])
    assert not torch.equal(la[:, 1], lc[:, 1])
    assert not all(torch.equal(x, y) for x, y in zip(_state(a, 1)[:36], _state(c, 1)[:36]))


def test_nothing_is_written_outside_the_stacks_and_the_workspace():
    """A canary of 64 floats on both sides of every stack, of every batch array, of the loss and of the workspace survives three
    updates (the third with the actor step)."""
    from armenv import _lib as L
    P, B, D, PAD = 3, 257, 9, 64
    gen = torch.Generator(device=DEV); gen.manual_seed(31)
    pop = _population(P, D, gen)
    CANARY = 12345.0

    def padded(t):
        """a copy of t inside a buffer with PAD canary floats (or bytes, for uint8) before and after it"""
        buf = torch.full((t.numel() + 2 * PAD,), CANARY if t.dtype == torch.float32 else 77, dtype=t.dtype, device=DEV)
        inner = buf[PAD:PAD + t.numel()].view(t.shape)
        inner.copy_(t)
        return buf, inner

    bufs = []
    for name in NETS:
        for k, t in enumerate(pop.stacks[name]):
            buf, inner = padded(t)
            bufs.append(buf)
            pop.stacks[name][k] = inner
    lib = L.load()
    ws_bytes = lib.armenv_td3_pop_workspace_bytes(D, 256, B, P)
    ws_buf = torch.full((ws_bytes // 4 + 2 * PAD,), CANARY, device=DEV)
    bufs.append(ws_buf)
    pop._ws = ws_buf[PAD:PAD + ws_bytes // 4].view(torch.uint8)
    assert pop._ws.numel() == ws_bytes and pop._ws.data_ptr() % 16 == 0
    before = [t.clone() for t in _state(pop, 1)]
    for _ in range(3):
        batch = _batch(gen, P, B, D)
        held = {}
        for k, t in batch.items():
            buf, inner = padded(t)
            bufs.append(buf)
            held[k] = inner
        pop.train(held, noise=None)
    torch.cuda.synchronize(DEV)
    assert pop.total_it == 7 and pop.actor_step == 2
    for buf in bufs:
        edge = torch.cat([buf[:PAD], buf[-PAD:]])
        assert bool((edge == (CANARY if buf.dtype == torch.float32 else 77)).all())
    assert not all(torch.equal(x, y) for x, y in zip(before, _state(pop, 1)))      # ... and the update did run on the padded stacks


def test_one_member_equals_the_single_update_on_the_same_tensors():
    """P = 1: armenv_td3_pop_update and armenv_td3_update called on THE SAME tensors (a copy of the state, the very same argument
    struct as `one`) give the same bits, with and without the actor step."""
    from armenv import _lib as L
    lib = L.load()
    gen = torch.Generator(device=DEV); gen.manual_seed(41)
    B, D = 257, 6
    batch = _batch(gen, 1, B, D)
    for with_actor in (0, 1):
        pops = []
        for use_pop in (True, False):
            g2 = torch.Generator(device=DEV); g2.manual_seed(42)
            pop = _population(1, D, g2)
            pa = pop._static_args()
            one = pa.one
            ws = torch.empty(lib.armenv_td3_workspace_bytes(D, 256, B), dtype=torch.uint8, device=DEV)
            loss = torch.zeros(1, device=DEV)
            one.batch, one.with_actor, one.critic_step, one.actor_step, one.draw = B, with_actor, 5, 2, 5
            one.states_dev, one.actions_dev, one.next_states_dev = (batch[k].data_ptr() for k in ("states", "actions", "next_states"))
            one.rewards_dev, one.dones_dev, one.loss_dev = batch["rewards"].data_ptr(), batch["dones"].data_ptr(), loss.data_ptr()
            one.workspace_dev, one.workspace_bytes = ws.data_ptr(), ws.numel()
            stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
            L.check(lib.armenv_td3_pop_update(C.byref(pa), stream) if use_pop else lib.armenv_td3_update(C.byref(one), stream))
            torch.cuda.synchronize(DEV)
            pops.append((pop, loss))
        (a, la), (b, lb) = pops
        assert torch.equal(la, lb) and float(la) > 0.0
        assert all(torch.equal(x, y) for x, y in zip(_state(a, 0), _state(b, 0))), with_actor


def test_population_update_is_deterministic_across_runs_and_streams():
    """Three populations from the same state, six train calls on the same batches with the in-kernel noise, two on the default
    stream and one on a side stream: all tensors and losses are bitwise equal."""
    P, B, D = 3, 257, 6
    gen = torch.Generator(device=DEV); gen.manual_seed(51)
    batches = [_batch(gen, P, B, D) for _ in range(6)]
    pops = []
    for _ in range(3):
        g2 = torch.Generator(device=DEV); g2.manual_seed(52)
        pops.append(_population(P, D, g2))
    side = torch.cuda.Stream(device=DEV)
    losses = [[], [], []]
    for batch in batches:
        for k in (0, 1):
            losses[k].append(pops[k].train(batch))
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            losses[2].append(pops[2].train(batch))
        torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    for k in (1, 2):
        for p in range(P):
            assert all(torch.equal(x, y) for x, y in zip(_state(pops[0], p), _state(pops[k], p))), (k, p)
        assert all(torch.equal(x, y) for x, y in zip(losses[0], losses[k])), k


def test_population_update_captured_in_a_graph_equals_direct_calls():
    """armenv_td3_pop_update (with the actor step) captured into a torch.cuda.graph on one stream and replayed three times equals
    three direct calls with the same arguments, bit for bit: the call only enqueues kernels, one serial chain."""
    from armenv import _lib as L
    lib = L.load()
    P, B, D = 3, 257, 6
    gen = torch.Generator(device=DEV); gen.manual_seed(61)
    batch = _batch(gen, P, B, D)
    noise = torch.randn(P, B, 3, device=DEV, generator=gen)

    def prepared():
        g2 = torch.Generator(device=DEV); g2.manual_seed(62)
        pop = _population(P, D, g2)
        pa = pop._static_args()
        one = pa.one
        ws = torch.empty(lib.armenv_td3_pop_workspace_bytes(D, 256, B, P), dtype=torch.uint8, device=DEV)
        loss = torch.zeros(P, device=DEV)
        one.batch, one.with_actor, one.critic_step, one.actor_step, one.draw = B, 1, 5, 2, 5
        one.noise_dev = noise.data_ptr()
        one.states_dev, one.actions_dev, one.next_states_dev = (batch[k].data_ptr() for k in ("states", "actions", "next_states"))
        one.rewards_dev, one.dones_dev, one.loss_dev = batch["rewards"].data_ptr(), batch["dones"].data_ptr(), loss.data_ptr()
        one.workspace_dev, one.workspace_bytes = ws.data_ptr(), ws.numel()
        call = lambda: L.check(lib.armenv_td3_pop_update(C.byref(pa), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
        return pop, call, loss, ws

    direct, call_d, loss_d, _ws_d = prepared()
    for _ in range(3):
        call_d()
    graphed, call_g, loss_g, _ws_g = prepared()
    torch.cuda.synchronize(DEV)
    before = [t.clone() for p in range(P) for t in _state(graphed, p)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call_g()
    torch.cuda.synchronize(DEV)
    assert all(torch.equal(x, y) for x, y in zip(before, [t for p in range(P) for t in _state(graphed, p)]))   # capture runs nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize(DEV)
    for p in range(P):
        assert all(torch.equal(x, y) for x, y in zip(_state(direct, p), _state(graphed, p))), p
    assert torch.equal(loss_d, loss_g)
    assert not torch.equal(before[0], _state(graphed, 0)[0])


def test_zero_learning_rates_and_tau_leave_every_member_unchanged():
    P, B, D = 3, 64, 6
    gen = torch.Generator(device=DEV); gen.manual_seed(71)
    pop = _population(P, D, gen, actor_lr=0.0, critic_lr=0.0, tau=0.0)
    before = [[t.clone() for t in _state(pop, p)[:36]] for p in range(P)]          # the six nets; the moments do move
    for _ in range(3):
        loss = pop.train(_batch(gen, P, B, D))
    assert pop.actor_step == 2 and bool(torch.isfinite(loss).all())
    for p in range(P):
        assert all(torch.equal(x, y) for x, y in zip(before[p], _state(pop, p)[:36])), p


def test_load_and_export_member_round_trip():
    from armenv.fused_td3 import FusedTD3
    gen = torch.Generator(device=DEV); gen.manual_seed(81)
    pop = _population(2, 6, gen)
    torch.manual_seed(4)
    single = FusedTD3(6, 3, 0.7, device=DEV, seed=3)
    for _ in range(4):
        single.train(_member_batch(_batch(gen, 1, 64, 6), 0))
    pop.load_member(1, single)
    assert (pop.total_it, pop.critic_step, pop.actor_step) == (4, 4, 1)
    assert all(torch.equal(x, y) for x, y in zip(_state(pop, 1), _single_state(single)))
    back = pop.export_member(1)
    assert back.seed == 11 + 1 and (back.total_it, back.critic_step, back.actor_step) == (4, 4, 1)
    assert all(torch.equal(x, y) for x, y in zip(_single_state(back), _single_state(single)))
    s = torch.rand(6).tolist()
    assert (pop.member(1).take_action(s) == single.take_action(s)).all()


def test_population_training_loop_learns_reach_for_every_member():
    """train_reach_population(members=3) at the size, iteration count and bar of test_training_loop_learns_reach_with_the_fused_learner
    (each member is that run with its own seed): >= 90 % success over the last log window for every member; the members' curves
    are not identical, their seeds being independent."""
    from armenv.fused_td3_pop import FusedTD3Population
    from armenv.train_pop import train_reach_population
    hist = []
    pop, _ = train_reach_population(members=3, num_envs=1024, iterations=140, updates=48, batch_size=2048, log_every=20,
                                    log=lambda s_: hist.append(json.loads(s_)))
    assert isinstance(pop, FusedTD3Population) and pop.total_it > 0 and len(hist) == 7
    rates = hist[-1]["success_rate"]
    print("success rates per log window:", [[round(r, 3) for r in h["success_rate"]] for h in hist])
    assert len(rates) == 3 and min(rates) >= 0.9, [[round(r, 2) for r in h["success_rate"]] for h in hist]
    assert min(hist[-1]["episodes"]) > 5000
    curves = [[h["success_rate"][p] for h in hist] for p in range(3)]
    assert curves[0] != curves[1] and curves[1] != curves[2] and curves[0] != curves[2]
