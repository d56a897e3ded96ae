"""Per-member hyper-parameters of the population updates (armenv_td3_pop_update_hyper, armenv_daddpg_pop_update_hyper,
armenv_datd3_pop_update_hyper through the populations of armenv.fused_*_pop) on cuda:0.  The oracle is the single-learner update:
member p of a population update equals the SINGLE entry point on member p's tensors with member p's hyper-parameters and seed + p,
BIT FOR BIT -- no tolerance anywhere below.  The single-learner kernels are themselves pinned to float64 references and the
reference's golden updates by the rest of the suite."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import pop_common as pc

pytestmark = pytest.mark.gpu
DEV = pc.DEV
KINDS = ("td3", "daddpg", "datd3", "darc")
# (low, high) of the random draws; gamma, tau and q_weight live in [0, 1], the others are >= 0
RANGES = dict(actor_lr=(1e-4, 3e-3), critic_lr=(1e-4, 3e-3), tau=(1e-3, 5e-2), gamma=(0.9, 0.999), policy_noise=(0.05, 0.4),
              noise_clip=(0.2, 0.8), q_weight=(0.1, 0.9), regularization_weight=(1e-3, 5e-2))
# the edges of the ranges, one set per member (rotated by the case, so that one-member populations meet them too)
EDGES = (dict(gamma=0.0, tau=1.0, q_weight=0.0), dict(gamma=1.0, tau=0.0, policy_noise=0.0, q_weight=1.0), dict(actor_lr=0.0),
         dict(critic_lr=0.0, regularization_weight=0.0), dict())


def _member_values(kind, P, rng, rotate=0, edges=True):
    """{name: [P values]}: distinct per member and per field, member p holding the edge values of EDGES[(p + rotate) % 5]"""
    names = pc.classes(kind)[0].sweepable()
    values = {n: [float(np.float32(rng.uniform(*RANGES[n]))) for _ in range(P)] for n in names}
    for p in range(P if edges else 0):
        for n, v in EDGES[(p + rotate) % len(EDGES)].items():
            if n in values:
                values[n][p] = v
    return values


def _population(kind, P, D, gen, values, seed=11, force=True):
    """a population with random state, counters set mid-run and the members' `values`, on the per-member entry point"""
    pop = pc.population(kind, P, D, gen, seed=seed, **values)
    pop.always_hyper = force
    assert pop.entry_point.endswith("_pop_update_hyper") or not force
    return pop


def _noise(kind, gen, P, B, given):
    return pc.train_noises(kind, gen, P, B, 1)[0] if given else None


def _member_noise(noise, p):
    if noise is None:
        return None
    return noise[p] if torch.is_tensor(noise) else tuple(n[p] for n in noise)


def _equal(xs, ys):
    return all(torch.equal(x, y) for x, y in zip(xs, ys))


# trains per case and which of them are given their noise (the others draw it in the kernel).  TD3: total_it 5..9, the actor stepped
# at 6 (given noise) and 9 (drawn), not stepped at 5 (given) and 7, 8 (drawn).  DADDPG: four updates, both actors stepped twice.
# DATD3 / DARC: two trains = four updates.
TRAINS = dict(td3=(True, True, False, False, False), daddpg=(False,) * 4, datd3=(True, False), darc=(True, False))


@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_every_member_equals_the_single_update_with_its_own_values_bit_for_bit(kind, P, B, D):
    """P members with different random nets, moments, batches AND hyper-parameters (the ranges' edges among them: gamma 0 and 1, tau
    0 and 1, policy_noise 0, q_weight 0 and 1, a zero learning rate).  After every train each tensor of member p and its losses equal
    a single learner that started from member p's state, holds member p's values and seed + p, and was stepped by the single entry
    point on member p's batch."""
    rotate = (B > 1) * 2 + (D > 6)
    rng = np.random.default_rng(1000 * P + B + D)
    gen = pc.generator(1000 * P + B + D)
    values = _member_values(kind, P, rng, rotate)
    pop = _population(kind, P, D, gen, values)
    singles = [pop.export_member(p) for p in range(P)]
    for p, single in enumerate(singles):
        assert all(getattr(single, n) == values[n][p] for n in values), p
        assert single.total_it == pc.MID_RUN[kind]["total_it"] and (kind == "daddpg" or single.seed == 11 + p)
    for it, given in enumerate(TRAINS[kind]):
        b = pc.batch(gen, P, B, D)
        noise = _noise(kind, gen, P, B, given)
        losses = pc.train(kind, pop, b, noise)
        for p, single in enumerate(singles):
            ls = pc.train(kind, single, pc.member_batch(b, p), _member_noise(noise, p))
            assert all(torch.equal(x, y[p]) for x, y in zip(ls, losses)), (it, p)
            bad = [k for k, (x, y) in enumerate(zip(pc.state(pop, p), pop._single_state(single))) if not torch.equal(x, y)]
            assert not bad, (it, p, bad)
    assert all(getattr(pop, c) == getattr(singles[0], c) for c in pop._COUNTERS)
    if kind == "td3":
        assert pop.total_it == 9 and pop.actor_step == 3
    assert all(bool(torch.isfinite(t).all()) for six in pop.stacks.values() for t in six)
    if P > 1:
        assert not torch.equal(pop.stacks[pop._NETS[0]][0][0], pop.stacks[pop._NETS[0]][0][1])


def _run(kind, P, B, D, batches, noises, values, force=True, seed_gen=3):
    pop = _population(kind, P, D, pc.generator(seed_gen), values, force=force)
    losses = [torch.stack(pc.train(kind, pop, b, n)) for b, n in zip(batches, noises)]
    return pop, torch.stack(losses)


@pytest.mark.parametrize("kind", KINDS)
def test_shared_values_equal_the_population_update_and_members_do_not_leak(kind):
    """(1) Every member given `one`'s values: the per-member entry point equals armenv_*_pop_update bit for bit.  (2) Distinct values,
    then members 0 and 2 swap their hyper-parameters and nothing else: member 1 is bit-identical to the first run and members 0 and 2
    are not."""
    P, B, D = 3, 257, 6
    gen = pc.generator(21)
    count = 3 if kind in ("td3", "daddpg") else 2
    batches = [pc.batch(gen, P, B, D) for _ in range(count)]
    noises = [_noise(kind, gen, P, B, True) for _ in range(count)]
    shared, ls = _run(kind, P, B, D, batches, noises, {}, force=False)
    forced, lf = _run(kind, P, B, D, batches, noises, {}, force=True)
    assert shared.entry_point.endswith("_pop_update") and forced.entry_point.endswith("_pop_update_hyper")
    assert torch.equal(ls, lf) and all(_equal(pc.state(shared, p), pc.state(forced, p)) for p in range(P))
    values = _member_values(kind, P, np.random.default_rng(22), edges=False)
    swapped = {n: [v[2], v[1], v[0]] for n, v in values.items()}
    a, la = _run(kind, P, B, D, batches, noises, values)
    c, lc = _run(kind, P, B, D, batches, noises, swapped)
    assert _equal(pc.state(a, 1), pc.state(c, 1)) and torch.equal(la[..., 1], lc[..., 1])
    n_nets = 6 * len(a._NETS)
    for p in (0, 2):
        assert not torch.equal(la[..., p], lc[..., p]), p
        assert not _equal(pc.state(a, p)[:n_nets], pc.state(c, p)[:n_nets]), p
    assert not _equal(pc.state(a, 1), pc.state(shared, 1))          # ... and the values did reach the kernels


def _prepared(kind, pop, B, b, noise, updates, ws=None, loss=None):
    """(call, loss, keep): `call()` enqueues the population's bound entry point (armenv_*_pop_update_hyper with the members' table as
    it is NOW) once per entry of `updates` -- TD3: with_actor values; the others: update_actor values -- with fixed step numbers, on
    the current stream"""
    from armenv import _lib as L
    stem = pc.classes(kind)[2]
    P, D = pop.members, pop.state_dim
    pop._bind(pop._static_args())
    pa, table, fn = pop._args, pop._table, pop._bound_fn
    assert table is not None and len(table) == P
    one = pa.one
    if ws is None:
        ws = torch.empty(getattr(L.load(), "armenv_%s_pop_workspace_bytes" % stem)(D, 256, B, P), dtype=torch.uint8, device=DEV)
    if loss is None:
        loss = torch.zeros(len(updates), P, device=DEV)
    one.batch, one.critic_step, one.actor_step = B, 5, 4
    one.states_dev, one.actions_dev, one.next_states_dev = (b[k].data_ptr() for k in ("states", "actions", "next_states"))
    one.rewards_dev, one.dones_dev = b["rewards"].data_ptr(), b["dones"].data_ptr()
    one.workspace_dev, one.workspace_bytes = ws.data_ptr(), ws.numel()

    def call():
        for i, k in enumerate(updates):
            one.loss_dev = loss[i].data_ptr()
            pc.set_update(one, kind, k, 7 + i, None if noise is None else noise[i])
            L.check(fn(C.byref(pa), table, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    return call, loss, (ws, pa, table)


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_is_written_outside_the_stacks_and_the_workspace(kind):
    """A canary of 64 floats on both sides of every stack, of every batch array, of the loss and of the workspace survives two updates
    on the per-member entry point (TD3: without and with the actor step; the others: both actors / critics stepped once)."""
    from armenv import _lib as L
    P, B, D = 3, 257, 9
    gen = pc.generator(31)
    pop = _population(kind, P, D, gen, _member_values(kind, P, np.random.default_rng(31)))
    bufs = []

    def padded(t):
        buf = torch.full((t.numel() + 2 * pc.PAD,), pc.CANARY if t.dtype == torch.float32 else 77, dtype=t.dtype, device=DEV)
        inner = buf[pc.PAD:pc.PAD + t.numel()].view(t.shape)
        inner.copy_(t)
        bufs.append(buf)
        return inner

    for name in list(pop.stacks):
        pop.stacks[name] = [padded(t) for t in pop.stacks[name]]
    ws_bytes = getattr(L.load(), "armenv_%s_pop_workspace_bytes" % pc.classes(kind)[2])(D, 256, B, P)
    ws = padded(torch.zeros(ws_bytes // 4, device=DEV)).view(torch.uint8)
    assert ws.numel() == ws_bytes and ws.data_ptr() % 16 == 0
    loss = padded(torch.zeros(2, P, device=DEV))
    held = {k: padded(t) for k, t in pc.batch(gen, P, B, D).items()}
    before = [t.clone() for t in pc.state(pop, 1)]
    call, _, _keep = _prepared(kind, pop, B, held, None, pc.updates(kind), ws=ws, loss=loss)
    call()
    torch.cuda.synchronize(DEV)
    for buf in bufs:
        edge = torch.cat([buf[:pc.PAD], buf[-pc.PAD:]])
        assert bool((edge == (pc.CANARY if buf.dtype == torch.float32 else 77)).all())
    assert bool(torch.isfinite(loss).all()) and bool((loss > 0).all())
    assert not any(torch.equal(x, y) for x, y in zip(before[:6], pc.state(pop, 1)[:6]))      # the update did run on the padded stacks


@pytest.mark.parametrize("kind", KINDS)
def test_a_member_with_zero_rates_stands_still_while_its_neighbours_move(kind):
    """Member 1 has actor_lr = critic_lr = tau = 0: every net and every target of it is bitwise unchanged after the trains (its Adam
    moments, which no rate scales, do move), while members 0 and 2, with the defaults, change."""
    P, B, D = 3, 64, 6
    gen = pc.generator(71)
    values = dict(actor_lr=[1e-3, 0.0, 1e-3], critic_lr=[1e-3, 0.0, 1e-3], tau=[0.005, 0.0, 0.005])
    pop = _population(kind, P, D, gen, values, force=False)
    assert pop.entry_point.endswith("_pop_update_hyper")
    n_nets = 6 * len(pop._NETS)
    before = [[t.clone() for t in pc.state(pop, p)] for p in range(P)]
    for _ in range(3 if kind in ("td3", "daddpg") else 2):         # TD3: total_it 5, 6, 7 -- the actor and the targets move at 6
        losses = pc.train(kind, pop, pc.batch(gen, P, B, D))
    assert all(bool(torch.isfinite(x).all()) for x in losses)
    assert _equal(before[1][:n_nets], pc.state(pop, 1)[:n_nets])
    assert not _equal(before[1][n_nets:], pc.state(pop, 1)[n_nets:])
    for p in (0, 2):
        moved = [not torch.equal(x, y) for x, y in zip(before[p][:n_nets], pc.state(pop, p)[:n_nets])]
        assert all(moved), (p, moved)


@pytest.mark.parametrize("kind", KINDS)
def test_the_update_is_deterministic_across_runs_and_streams(kind):
    """Three populations from the same state and the same members' values, three trains on the same batches with the in-kernel noise,
    two on the default stream and one on a side stream: all tensors and losses are bitwise equal."""
    P, B, D = 3, 257, 6
    gen = pc.generator(51)
    batches = [pc.batch(gen, P, B, D) for _ in range(3)]
    values = _member_values(kind, P, np.random.default_rng(51))
    pops = [_population(kind, P, D, pc.generator(52), values) for _ in range(3)]
    side = torch.cuda.Stream(device=DEV)
    losses = [[], [], []]
    for b in batches:
        for k in (0, 1):
            losses[k] += pc.train(kind, pops[k], b)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            losses[2] += pc.train(kind, pops[2], b)
        torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    for k in (1, 2):
        assert all(_equal(pc.state(pops[0], p), pc.state(pops[k], p)) for p in range(P)), k
        assert _equal(losses[0], losses[k]), k


@pytest.mark.parametrize("kind", KINDS)
def test_a_captured_update_keeps_the_values_of_capture_time(kind):
    """Two updates captured into a torch.cuda.graph on one stream (one serial chain) and replayed equal the direct calls bit for bit.
    After set_hyper the replay still runs with the values it was captured with -- they are kernel arguments -- while a fresh direct
    call runs with the new ones."""
    P, B, D = 3, 257, 6
    gen = pc.generator(61)
    b = pc.batch(gen, P, B, D)
    updates = pc.updates(kind)
    noise = None if kind == "daddpg" else [pc.noise_for(gen, P, B) for _ in updates]
    values = _member_values(kind, P, np.random.default_rng(61), edges=False)
    direct, graphed, fresh = (_population(kind, P, D, pc.generator(62), values) for _ in range(3))
    call_d, loss_d, _kd = _prepared(kind, direct, B, b, noise, updates)
    call_g, loss_g, _kg = _prepared(kind, graphed, B, b, noise, updates)
    torch.cuda.synchronize(DEV)
    before = [t.clone() for p in range(P) for t in pc.state(graphed, p)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call_g()
    torch.cuda.synchronize(DEV)
    assert _equal(before, [t for p in range(P) for t in pc.state(graphed, p)])          # capture runs nothing
    call_d()
    g.replay()
    torch.cuda.synchronize(DEV)
    assert torch.equal(loss_d, loss_g) and all(_equal(pc.state(direct, p), pc.state(graphed, p)) for p in range(P))
    assert not torch.equal(before[0], pc.state(graphed, 0)[0])
    # new values for member 1 of `graphed` (and of `fresh`, which is where `direct` was before its first call)
    new = dict(gamma=0.5, critic_lr=values["critic_lr"][1] * 4, tau=0.5)
    graphed.set_hyper(1, **new)
    assert graphed._args is None and graphed.hyper(1)["gamma"] == 0.5
    call_d()
    g.replay()
    torch.cuda.synchronize(DEV)
    assert torch.equal(loss_d, loss_g) and all(_equal(pc.state(direct, p), pc.state(graphed, p)) for p in range(P))
    fresh.set_hyper(1, **new)
    call_f, loss_f, _kf = _prepared(kind, fresh, B, b, noise, updates)
    first_d = _population(kind, P, D, pc.generator(62), values)          # the capture-time values, from the same state
    call_1, loss_first, _k1 = _prepared(kind, first_d, B, b, noise, updates)
    call_f()
    call_1()
    torch.cuda.synchronize(DEV)
    for p in (0, 2):
        assert _equal(pc.state(fresh, p), pc.state(first_d, p)) and torch.equal(loss_f[:, p], loss_first[:, p])
    assert not torch.equal(loss_f[:, 1], loss_first[:, 1]) and not _equal(pc.state(fresh, 1), pc.state(first_d, 1))


def test_a_sweep_trains_reach_and_a_member_with_zero_rates_keeps_its_initial_weights():
    """train_reach_population(members=3, sweep=...) at the size, iteration count and bar of
    test_population_training_loop_learns_reach_for_every_member: the first member, with that test's rates, reaches >= 90 % success over
    the last log window; the third, with actor_lr = critic_lr = tau = 0, ends on its initial weights bit for bit; every record names
    the three members' values."""
    from armenv.fused_td3_pop import FusedTD3Population
    from armenv.train_pop import train_reach_population
    sweep = {"actor_lr": [1e-3, 3e-4, 0.0], "critic_lr": [1e-3, 3e-4, 0.0], "tau": [0.005, 0.005, 0.0]}
    hist = []
    pop, _ = train_reach_population(members=3, num_envs=1024, iterations=140, updates=48, batch_size=2048, log_every=20,
                                    log=lambda s_: hist.append(json.loads(s_)), sweep=sweep)
    assert isinstance(pop, FusedTD3Population) and pop.total_it > 0 and len(hist) == 7
    assert pop.entry_point == "armenv_td3_pop_update_hyper" and pop.actor_lr == (1e-3, 3e-4, 0.0)
    print("success rates per log window:", [[round(r, 3) for r in h["success_rate"]] for h in hist])
    assert all(h["hyper"] == sweep for h in hist)
    assert hist[-1]["success_rate"][0] >= 0.9, [[round(r, 2) for r in h["success_rate"]] for h in hist]
    initial = FusedTD3Population(3, 6, 3, 0.7, device=DEV, seed=0)
    n_nets = 6 * len(pop._NETS)
    assert _equal(pc.state(pop, 2)[:n_nets], pc.state(initial, 2)[:n_nets])
    assert not any(torch.equal(x, y) for x, y in zip(pc.state(pop, 0)[:n_nets], pc.state(initial, 0)[:n_nets]))


@pytest.mark.parametrize("algo", KINDS)
def test_no_sweep_trains_the_bits_it_always_did(algo):
    """sweep=None and no `sweep` argument at all: the same stacks, bit for bit, the shared entry point, and records without `hyper`."""
    from armenv.train_pop import train_reach_population
    kw = dict(members=2, num_envs=64, iterations=8, rollout_steps=32, updates=3, batch_size=64, max_steps=20, log_every=4,
              log=lambda s_: None, algo=algo)
    a, ha = train_reach_population(**kw)
    c, hc = train_reach_population(sweep=None, **kw)
    assert a.total_it > 0 and a.total_it == c.total_it and a.entry_point.endswith("_pop_update")
    assert all(_equal(pc.state(a, p), pc.state(c, p)) for p in range(2))
    assert len(ha) == 2 and all("hyper" not in h for h in ha + hc)
    assert [h["success_rate"] for h in ha] == [h["success_rate"] for h in hc]
