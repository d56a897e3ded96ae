"""What the GPU tests of the population updates share (tests/test_gpu_td3_pop.py, test_gpu_daddpg_pop.py, test_gpu_datd3_pop.py,
test_gpu_pop_hyper.py, test_gpu_pbt.py): the populations of the four agents (kind "td3", "daddpg", "datd3" or "darc") on cuda:0 and
the checks that do not depend on the agent.  The oracle is the single-learner update: member p of a population update equals the
single entry point on member p's tensors BIT FOR BIT -- no tolerance anywhere."""
import ctypes as C

import torch

from learner_host import classes  # noqa: F401  ((population class, single class, the C entry points' stem) of a kind)

DEV = "cuda:0"
PAD, CANARY = 64, 12345.0


def generator(seed):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return gen


def batch(gen, P, B, D):
    r = lambda *shape: torch.rand(*shape, device=DEV, generator=gen)
    return dict(states=r(P, B, D), actions=r(P, B, 3) * 1.4 - 0.7, next_states=r(P, B, D), rewards=r(P, B) - 0.5,
                dones=(r(P, B) < 0.1).to(torch.uint8))


def member_batch(b, p):
    return {k: v[p] for k, v in b.items()}


def noise_for(gen, P, B):
    return torch.randn(P, B, 3, device=DEV, generator=gen)


def randomise(pop, gen):
    """different random nets, targets and (valid: v >= 0) moments for every member"""
    for name, six in pop.stacks.items():
        for t in six:
            x = torch.randn(t.shape, device=DEV, generator=gen) * 0.1
            t.copy_(x.abs() * 1e-3 if name.endswith("_v") else x * (0.01 if name.endswith("_m") else 1.0))


# TD3 (policy_freq 3) steps its actor at total_it 6 and 9: the second and the fifth train from here
MID_RUN = dict(td3=dict(total_it=4, critic_step=4, actor_step=1),
               daddpg=dict(total_it=5, critic_step=5, actor1_step=2, actor2_step=3),
               datd3=dict(total_it=6, actor1_step=3, critic1_step=3, actor2_step=3, critic2_step=3))
MID_RUN["darc"] = MID_RUN["datd3"]


def population(kind, P, D, gen, seed=11, **kw):
    """a population with random state and counters set mid-run: bias corrections that are not those of step 1"""
    pop = classes(kind)[0](P, D, 3, 0.7, device=DEV, seed=seed, **kw)
    if gen is not None:
        randomise(pop, gen)
    for name, value in MID_RUN[kind].items():
        setattr(pop, name, value)
    return pop


def state(pop, p):
    return pop._member_state(p)


def stack_names(pop, k):
    """(stacks an update writes, stacks it must leave alone); k: the actor / critic that the update steps, TD3: whether it takes the
    actor step"""
    if "q1" in pop.stacks:                # TD3: the actor, its moments and all three targets move with the actor step only
        with_actor = ["actor", "actor_m", "actor_v", "target_actor", "target_q1", "target_q2"]
        written = ["q1", "q2", "q1_m", "q1_v", "q2_m", "q2_v"] + (with_actor if k else [])
        return written, [] if k else with_actor
    other = 3 - k
    if "critic" in pop.stacks:            # DADDPG: one critic, its target moves only with actor 2
        written = ["actor%d" % k, "target_actor%d" % k, "actor%d_m" % k, "actor%d_v" % k, "critic", "critic_m", "critic_v"]
        written += ["target_critic"] if k == 2 else []
        untouched = ["actor%d" % other, "target_actor%d" % other, "actor%d_m" % other, "actor%d_v" % other]
        untouched += ["target_critic"] if k == 1 else []
        return written, untouched
    names = lambda j: [f % j for f in ("actor%d", "critic%d", "target_actor%d", "target_critic%d", "actor%d_m", "actor%d_v",
                                        "critic%d_m", "critic%d_v")]
    return names(k), names(other)


def train(kind, learner, b, noise=None):
    """one `train` of a population or a single learner; the losses as a list of tensors"""
    if kind == "daddpg":
        return [learner.train(b)]
    losses = learner.train(b, noise=noise)
    return [losses] if kind == "td3" else list(losses)


def run(kind, P, B, D, batches, noises, seed_gen=3, **kw):
    pop = population(kind, P, D, generator(seed_gen), **kw)
    losses = [torch.stack(train(kind, pop, b, n)) for b, n in zip(batches, noises)]
    return pop, torch.stack(losses)


def train_noises(kind, gen, P, B, count):
    """`count` train calls' given noise: None for DADDPG, one tensor per call for TD3, a pair per call for DATD3 / DARC"""
    def one():
        if kind == "daddpg":
            return None
        return noise_for(gen, P, B) if kind == "td3" else (noise_for(gen, P, B), noise_for(gen, P, B))
    return [one() for _ in range(count)]


def updates(kind):
    """what one C call is asked for, in turn: TD3 without and with the actor step, the others actor / critic 1 then 2"""
    return (0, 1) if kind == "td3" else (1, 2)


def set_update(one, kind, k, draw, noise=None):
    """the fields of `one` that name the update: which one, and (where the agent has noise) its draw and its given noise"""
    if kind == "td3":
        one.with_actor = k
    else:
        one.update_actor = k
    if kind != "daddpg":
        one.draw = draw
        one.noise_dev = noise.data_ptr() if noise is not None else None


def check_members_do_not_leak(kind):
    """Three train calls (TD3: the second with the actor step) twice, the second time with member 1's batch perturbed: members 0 and
    2 are bit-identical to the first run and member 1 is not."""
    P, B, D = 3, 257, 6
    gen = generator(21)
    batches = [batch(gen, P, B, D) for _ in range(3)]
    noises = train_noises(kind, gen, P, B, 3)
    a, la = run(kind, P, B, D, batches, noises)
    perturbed = [{k: v.clone() for k, v in b.items()} for b in batches]
    for b in perturbed:
        b["states"][1] += 0.125
        b["rewards"][1] -= 0.5
    c, lc = run(kind, P, B, D, perturbed, noises)
    for p in (0, 2):
        assert all(torch.equal(x, y) for x, y in zip(state(a, p), state(c, p))), p
        assert torch.equal(la[..., p], lc[..., p])
    assert not torch.equal(la[..., 1], lc[..., 1])
    n_nets = 6 * len(a._NETS)
    assert not all(torch.equal(x, y) for x, y in zip(state(a, 1)[:n_nets], state(c, 1)[:n_nets]))


def check_canaries(kind):
    """A canary of 64 floats on both sides of every stack, of the workspace, and of every batch array and the loss of each of three
    updates survives them (TD3: the second with the actor step; the others: actor / critic 1, 2, 1)."""
    from armenv import _lib as L
    P, B, D = 3, 257, 9
    gen = generator(31)
    pop = population(kind, P, D, gen)
    stem = classes(kind)[2]
    bufs = []

    def padded(t):
        """a copy of t inside a buffer with PAD canary floats (or bytes, for uint8) before and after it"""
        buf = torch.full((t.numel() + 2 * PAD,), CANARY if t.dtype == torch.float32 else 77, dtype=t.dtype, device=DEV)
        inner = buf[PAD:PAD + t.numel()].view(t.shape)
        inner.copy_(t)
        bufs.append(buf)
        return inner

    for name in list(pop.stacks):
        pop.stacks[name] = [padded(t) for t in pop.stacks[name]]
    lib = L.load()
    ws_bytes = getattr(lib, "armenv_%s_pop_workspace_bytes" % stem)(D, 256, B, P)
    ws = padded(torch.zeros(ws_bytes // 4, device=DEV)).view(torch.uint8)
    assert ws.numel() == ws_bytes and ws.data_ptr() % 16 == 0
    before = [t.clone() for t in state(pop, 1)]
    pa = pop._static_args()
    one = pa.one
    one.batch, one.critic_step, one.actor_step = B, 4, 4
    one.workspace_dev, one.workspace_bytes = ws.data_ptr(), ws.numel()
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    losses = []
    for i, k in enumerate(updates(kind) + updates(kind)[:1]):
        held = {name: padded(t) for name, t in batch(gen, P, B, D).items()}
        losses.append(padded(torch.zeros(P, device=DEV)))
        one.states_dev, one.actions_dev, one.next_states_dev = (held[n].data_ptr() for n in ("states", "actions", "next_states"))
        one.rewards_dev, one.dones_dev, one.loss_dev = held["rewards"].data_ptr(), held["dones"].data_ptr(), losses[-1].data_ptr()
        set_update(one, kind, k, 7 + i)
        L.check(getattr(lib, "armenv_%s_pop_update" % stem)(C.byref(pa), stream))
    torch.cuda.synchronize(DEV)
    assert len(bufs) == 6 * len(pop.stacks) + 1 + 3 * 6
    for buf in bufs:
        edge = torch.cat([buf[:PAD], buf[-PAD:]])
        assert bool((edge == (CANARY if buf.dtype == torch.float32 else 77)).all())
    assert all(bool(torch.isfinite(loss).all()) and bool((loss > 0).all()) for loss in losses)
    assert not any(torch.equal(x, y) for x, y in zip(before[:6], state(pop, 1)[:6]))      # the update did run on the padded stacks


def prepared_call(kind, P, B, D, b, noise, seed_gen, use_pop=True):
    """(population, call, loss): `call()` enqueues armenv_<algo>_pop_update (or, P = 1 and use_pop False, the single entry point on
    the very same argument struct `one`) once per entry of updates(kind) with fixed step numbers, on the current stream"""
    from armenv import _lib as L
    lib = L.load()
    stem = classes(kind)[2]
    pop = population(kind, P, D, generator(seed_gen))
    pa = pop._static_args()
    one = pa.one
    n = getattr(lib, "armenv_%s_pop_workspace_bytes" % stem)(D, 256, B, P)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    loss = torch.zeros(len(updates(kind)), P, device=DEV)
    one.batch, one.critic_step, one.actor_step = B, 5, 4
    one.states_dev, one.actions_dev, one.next_states_dev = (b[k].data_ptr() for k in ("states", "actions", "next_states"))
    one.rewards_dev, one.dones_dev = b["rewards"].data_ptr(), b["dones"].data_ptr()
    one.workspace_dev, one.workspace_bytes = ws.data_ptr(), ws.numel()
    fn = getattr(lib, "armenv_%s_pop_update" % stem) if use_pop else getattr(lib, "armenv_%s_update" % stem)

    def call():
        for i, k in enumerate(updates(kind)):
            one.loss_dev = loss[i].data_ptr()
            set_update(one, kind, k, 7 + i, None if noise is None else noise[i])
            L.check(fn(C.byref(pa) if use_pop else C.byref(one), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    return pop, call, loss, (ws, pa)


def check_one_member_equals_the_single_update_on_the_same_tensors(kind):
    """P = 1: the population entry point and the single entry point called on THE SAME tensors (a copy of the state, the very same
    argument struct as `one`) give the same bits, for both entries of updates(kind)."""
    gen = generator(41)
    B, D = 257, 6
    b = batch(gen, 1, B, D)
    (a, call_a, la, _ka), (c, call_c, lc, _kc) = (prepared_call(kind, 1, B, D, b, None, 42, use_pop=u) for u in (True, False))
    call_a()
    call_c()
    torch.cuda.synchronize(DEV)
    assert torch.equal(la, lc) and bool((la > 0).all())
    assert all(torch.equal(x, y) for x, y in zip(state(a, 0), state(c, 0)))


def check_determinism(kind):
    """Three populations from the same state, six train calls on the same batches with the in-kernel noise, two on the default
    stream and one on a side stream: all tensors and losses are bitwise equal."""
    P, B, D = 3, 257, 6
    gen = generator(51)
    batches = [batch(gen, P, B, D) for _ in range(6)]
    pops = [population(kind, P, D, generator(52)) for _ in range(3)]
    side = torch.cuda.Stream(device=DEV)
    losses = [[], [], []]
    for b in batches:
        for k in (0, 1):
            losses[k] += train(kind, pops[k], b)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            losses[2] += train(kind, pops[2], b)
        torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    for k in (1, 2):
        for p in range(P):
            assert all(torch.equal(x, y) for x, y in zip(state(pops[0], p), state(pops[k], p))), (k, p)
        assert all(torch.equal(x, y) for x, y in zip(losses[0], losses[k])), k


def check_graph_capture(kind):
    """One call per entry of updates(kind), with given noise, captured into a torch.cuda.graph on one stream and replayed three times
    equals three direct runs with the same arguments, bit for bit: the call only enqueues kernels, one serial chain."""
    P, B, D = 3, 257, 6
    gen = generator(61)
    b = batch(gen, P, B, D)
    noise = None if kind == "daddpg" else [noise_for(gen, P, B) for _ in updates(kind)]
    direct, call_d, loss_d, _kd = prepared_call(kind, P, B, D, b, noise, 62)
    for _ in range(3):
        call_d()
    graphed, call_g, loss_g, _kg = prepared_call(kind, P, B, D, b, noise, 62)
    torch.cuda.synchronize(DEV)
    before = [t.clone() for p in range(P) for t in state(graphed, p)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call_g()
    torch.cuda.synchronize(DEV)
    assert all(torch.equal(x, y) for x, y in zip(before, [t for p in range(P) for t in state(graphed, p)]))   # capture runs nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize(DEV)
    for p in range(P):
        assert all(torch.equal(x, y) for x, y in zip(state(direct, p), state(graphed, p))), p
    assert torch.equal(loss_d, loss_g)
    assert not torch.equal(before[0], state(graphed, 0)[0])                # the first actor's W1: every kind's updates step it


def check_zero_learning_rates(kind):
    """Three train calls (TD3: the second with the actor step) under zero rates and tau: the nets are bitwise what they were"""
    P, B, D = 3, 64, 6
    gen = generator(71)
    pop = population(kind, P, D, gen, actor_lr=0.0, critic_lr=0.0, tau=0.0)
    n_nets = 6 * len(pop._NETS)
    before = [[t.clone() for t in state(pop, p)[:n_nets]] for p in range(P)]          # the nets; the moments do move
    for _ in range(3):
        losses = train(kind, pop, batch(gen, P, B, D))
    assert all(bool(torch.isfinite(x).all()) for x in losses)
    assert all(getattr(pop, name) > value for name, value in MID_RUN[kind].items())   # every optimiser stepped ...
    assert kind != "td3" or pop.actor_step == 2                                        # ... TD3's actor once
    for p in range(P):
        assert all(torch.equal(x, y) for x, y in zip(before[p], state(pop, p)[:n_nets])), p


def check_round_trip(kind):
    Pop, Single, _ = classes(kind)
    gen = generator(81)
    pop = population(kind, 2, 6, gen)
    torch.manual_seed(4)
    single = Single(6, 3, 0.7, device=DEV) if kind == "daddpg" else Single(6, 3, 0.7, device=DEV, seed=3)
    for _ in range(4):
        train(kind, single, member_batch(batch(gen, 1, 64, 6), 0))
    names = Pop._COUNTERS
    want = tuple(getattr(single, n) for n in names)
    assert want[0] == (4 if kind in ("td3", "daddpg") else 8) and all(want)
    pop.load_member(1, single)
    assert tuple(getattr(pop, n) for n in names) == want
    assert kind != "td3" or (pop.total_it, pop.critic_step, pop.actor_step) == (4, 4, 1)
    assert all(torch.equal(x, y) for x, y in zip(state(pop, 1), Pop._single_state(single)))
    back = pop.export_member(1)
    assert type(back) is Single and tuple(getattr(back, n) for n in names) == want
    if kind != "daddpg":
        assert back.seed == 11 + 1
    assert all(torch.equal(x, y) for x, y in zip(Pop._single_state(back), Pop._single_state(single)))
    s = torch.rand(6).tolist()
    assert (pop.member(1).take_action(s) == single.take_action(s)).all()
