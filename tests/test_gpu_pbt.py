"""Population-based training on cuda:0: FusedPopulation.exploit (armenv_pop_exploit, ONE launch of pop_exploit_kernel) against the
member-by-member copy_member, bit for bit -- a copy has no tolerance -- for the four populations, whose stacks hold members of 1, 3,
256, 768, 1 536, 2 304 and 65 536 floats (unaligned members, tails, one block and many); the kernel alone over sizes around its
float4 and block boundaries and over misaligned bases; what a `train` makes of an exploited member; and train_reach_population(pbt=)."""
import ctypes as C
import random

import pytest
import torch

import pop_common as pc

pytestmark = pytest.mark.gpu
DEV = pc.DEV
KINDS = ("td3", "daddpg", "datd3", "darc")


def _population(kind, P, gen_seed, D=6, **values):
    """a population whose members all differ in every tensor (moments included), counters set mid-run"""
    return pc.population(kind, P, D, pc.generator(gen_seed), **values)


def _tensors(pop):
    return [t for six in pop.stacks.values() for t in six]


def _equal(xs, ys):
    return all(torch.equal(x, y) for x, y in zip(xs, ys))


@pytest.mark.parametrize("kind", KINDS)
def test_exploit_equals_the_member_by_member_copies_bit_for_bit(kind):
    P, src = 5, [0, 0, 2, 2, 4]
    pop, twin = _population(kind, P, 5), _population(kind, P, 5)
    assert all(_equal(pc.state(pop, p), pc.state(twin, p)) for p in range(P))
    assert not any(torch.equal(x, y) for x, y in zip(pc.state(pop, 0), pc.state(pop, 1)))
    sizes = {t[0].numel() for t in _tensors(pop)}
    assert sizes == {1, 3, 256, 768, 1536, 2304, 65536} and len(_tensors(pop)) == (72 if kind in ("td3", "daddpg") else 96)
    before = [t.clone() for t in _tensors(pop)]
    counters = {c: getattr(pop, c) for c in pop._COUNTERS}
    assert pop.exploit(src) == [1, 3]
    torch.cuda.synchronize(DEV)
    for t, t0 in zip(_tensors(pop), before):
        assert torch.equal(t[1], t0[0]) and torch.equal(t[3], t0[2])              # the replaced members: their sources' bits
        assert torch.equal(t[0], t0[0]) and torch.equal(t[2], t0[2]) and torch.equal(t[4], t0[4])     # the others: untouched
    twin.copy_member(0, 1)
    twin.copy_member(2, 3)
    assert _equal(_tensors(pop), _tensors(twin))
    assert {c: getattr(pop, c) for c in pop._COUNTERS} == counters                # the step numbers are the population's
    assert pop.member(1).actor.fc1.weight.data_ptr() == pop.stacks[pop._NETS[0]][0][1].data_ptr()     # still views into the stacks


@pytest.mark.parametrize("kind", ["td3", "darc"])
def test_exploit_writes_nothing_outside_the_replaced_members(kind):
    """Every stack inside a buffer with 64 canary floats on both sides, and a plan that replaces the first and the last member."""
    P = 4
    pop = _population(kind, P, 6)
    bufs = []
    for name in list(pop.stacks):
        for k, t in enumerate(pop.stacks[name]):
            buf = torch.full((t.numel() + 2 * pc.PAD,), pc.CANARY, device=DEV)
            inner = buf[pc.PAD:pc.PAD + t.numel()].view(t.shape)
            inner.copy_(t)
            bufs.append(buf)
            pop.stacks[name][k] = inner
    before = [t.clone() for t in _tensors(pop)]
    pop.exploit([1, 1, 2, 2])
    torch.cuda.synchronize(DEV)
    for buf in bufs:
        assert bool((torch.cat([buf[:pc.PAD], buf[-pc.PAD:]]) == pc.CANARY).all())
    for t, t0 in zip(_tensors(pop), before):
        assert torch.equal(t, t0[[1, 1, 2, 2]])


# floats per member around the kernel's boundaries: the float4 body and its tail of 1..3, one block of 4096 floats and the next
ELEMS = (1, 2, 3, 4, 5, 7, 255, 1023, 1025, 4095, 4096, 4097, 8191, 8193, 12290)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_the_kernel_copies_every_size_from_every_alignment(offset):
    """armenv_pop_exploit itself over stacks of ELEMS floats per member whose member 0 starts `offset` floats after a 16-byte boundary
    (so members are aligned or not, source and destination alike or not, whatever elems % 4 is): the whole buffer -- the stack, the
    floats in front of it and 64 behind it -- equals the same copies made by torch, bit for bit."""
    from armenv import _lib as L
    P, src = 6, [0, 0, 5, 5, 4, 5]
    gen = pc.generator(40 + offset)
    bufs, stacks = [], []
    for n in ELEMS:
        buf = torch.randn(offset + P * n + pc.PAD, device=DEV, generator=gen)
        bufs.append(buf)
        stacks.append(buf[offset:offset + P * n].view(P, n))
        assert buf.data_ptr() % 16 == 0
    want = [b.clone() for b in bufs]
    for w, n in zip(want, ELEMS):
        w[offset:offset + P * n].view(P, n).copy_(w[offset:offset + P * n].view(P, n)[src])
    a = L.ArmEnvPopExploitArgs()
    a.device, a.members, a.tensors = 0, P, len(ELEMS)
    src_c, base_c = (C.c_int32 * P)(*src), (C.c_void_p * len(ELEMS))(*[t.data_ptr() for t in stacks])
    elems_c = (C.c_int64 * len(ELEMS))(*ELEMS)
    a.src, a.base, a.elems = src_c, base_c, elems_c
    L.check(L.load().armenv_pop_exploit(C.byref(a), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize(DEV)
    bad = [n for n, b, w in zip(ELEMS, bufs, want) if not torch.equal(b, w)]
    assert not bad, bad


def test_a_refused_plan_raises_and_leaves_every_tensor_unchanged():
    pop = _population("daddpg", 3, 7, tau=[0.005, 0.01, 0.02])
    before = [t.clone() for t in _tensors(pop)]
    rows = [pop.hyper(p) for p in range(3)]
    for bad in ([1, 2, 2], [0, 3, 2], [0, 1]):
        with pytest.raises(ValueError):
            pop.exploit(bad)
    torch.cuda.synchronize(DEV)
    assert _equal(_tensors(pop), before) and [pop.hyper(p) for p in range(3)] == rows


@pytest.mark.parametrize("kind", ["daddpg", "td3"])
def test_an_exploited_member_trains_like_its_source(kind):
    """After exploit([0, 0, 2]) members 0 and 1 are given the same batch (TD3: and the same target-policy noise): every `train` leaves
    them bitwise equal, losses included, and member 2 equal to member 2 of a twin population that was never exploited.  TD3: the
    second train (total_it 6) steps the actor and the targets."""
    P, B = 3, 8
    pop, twin = _population(kind, P, 8), _population(kind, P, 8)
    pop.exploit([0, 0, 2])
    gen = pc.generator(9)
    for it in range(2):
        b = pc.batch(gen, P, B, 6)
        for t in b.values():
            t[1].copy_(t[0])
        noise = None
        if kind == "td3":
            noise = pc.noise_for(gen, P, B)
            noise[1].copy_(noise[0])
        losses = pc.train(kind, pop, b, noise)
        twin_losses = pc.train(kind, twin, b, noise)
        torch.cuda.synchronize(DEV)
        assert _equal(pc.state(pop, 0), pc.state(pop, 1)), it
        assert all(torch.equal(x[0], x[1]) for x in losses), it
        assert _equal(pc.state(pop, 2), pc.state(twin, 2)) and all(torch.equal(x[2], y[2]) for x, y in zip(losses, twin_losses)), it
        assert _equal(pc.state(pop, 0), pc.state(twin, 0)) and not _equal(pc.state(pop, 1), pc.state(twin, 1)), it


@pytest.mark.parametrize("kind", KINDS)
def test_exploit_copies_the_hyper_parameters_only_when_asked(kind):
    stem = pc.classes(kind)[2]
    values = dict(tau=[0.005, 0.01, 0.02], critic_lr=[1e-3, 2e-3, 3e-3])
    pop = _population(kind, 3, 10, **values)
    rows = [pop.hyper(p) for p in range(3)]
    assert not pop.uniform() and pop.entry_point == "armenv_%s_pop_update_hyper" % stem
    pop.exploit([0, 0, 2], hyper=False)
    assert [pop.hyper(p) for p in range(3)] == rows and pop.tau == (0.005, 0.01, 0.02)
    assert _equal(pc.state(pop, 1), pc.state(pop, 0))
    pop.exploit([2, 1, 2], hyper=True)
    assert [pop.hyper(p) for p in range(3)] == [rows[2], rows[1], rows[2]] and pop.critic_lr == (3e-3, 2e-3, 3e-3)
    assert pop._args is None and pop.entry_point == "armenv_%s_pop_update_hyper" % stem
    pop.exploit([2, 2, 2])                                  # all members level: the shared-scalar entry point, as uniform() says
    assert pop.uniform() and pop.entry_point == "armenv_%s_pop_update" % stem and pop.tau == 0.02 and pop.critic_lr == 3e-3
    torch.cuda.synchronize(DEV)
    assert _equal(pc.state(pop, 0), pc.state(pop, 2)) and _equal(pc.state(pop, 1), pc.state(pop, 2))


def _stripped(history):
    return [{k: v for k, v in rec.items() if k != "wall_s"} for rec in history]


def test_a_pbt_run_is_reproducible_and_no_pbt_is_what_it_was():
    from armenv.train_pop import train_reach_population
    kw = dict(members=4, num_envs=64, iterations=6, updates=2, batch_size=64, seed=0, log=lambda s_: None)
    a, ha = train_reach_population(pbt=dict(every=2), **kw)
    b, hb = train_reach_population(pbt=dict(every=2), **kw)
    assert _equal(_tensors(a), _tensors(b)) and _stripped(ha) == _stripped(hb)
    steps = [rec for rec in ha if rec.get("kind") == "pbt"]
    assert [rec["iteration"] for rec in steps] == [2, 4, 6]
    for rec in steps:
        assert len(rec["fitness"]) == 4 and len(rec["src"]) == 4 and all(rec["src"][s] == s for s in rec["src"])
        assert [n["member"] for n in rec["new"]] == [p for p, s in enumerate(rec["src"]) if s != p]
        assert set(rec["hyper"]) == {"actor_lr", "critic_lr", "tau", "policy_noise", "noise_clip", "expl_sigma"}
    c, hc = train_reach_population(**kw)
    d, hd = train_reach_population(store="members", **kw)
    assert c.total_it == d.total_it and _equal(_tensors(c), _tensors(d)) and _stripped(hc) == _stripped(hd)
    assert all("kind" not in rec and "hyper" not in rec for rec in hc)


def test_the_training_loop_exploits_explores_and_records():
    """A schedule whose plan is fixed -- member 0 becomes member 1, member 3 becomes member 2 -- so that the loop's exploit branch runs
    whatever the success rates: after the step that ends the run, the replaced members hold their sources' bits, their values are
    their sources' times the documented draws, and the record says so.  Episodes of 20 steps, so that the updates do run."""
    from armenv.pbt import PBTSchedule
    from armenv.train_pop import sweepable_names, train_reach_population

    class Fixed(PBTSchedule):
        def plan(self, fitness):
            return [1, 1, 2, 2]

    logged = []
    sweep = dict(actor_lr=[1e-3, 5e-4, 2e-4, 1e-4], expl_sigma=[0.6, 0.5, 0.4, 0.3])
    pop, hist = train_reach_population(members=4, num_envs=64, iterations=8, updates=2, batch_size=64, max_steps=20, seed=3, log_every=4,
                                       log=logged.append, sweep=sweep, pbt=Fixed(every=4, seed=5))
    torch.cuda.synchronize(DEV)
    assert pop.total_it > 0 and len(logged) == len(hist) == 4
    assert [(rec.get("kind"), rec["iteration"]) for rec in hist] == [(None, 4), ("pbt", 4), (None, 8), ("pbt", 8)]
    assert _equal(pc.state(pop, 0), pc.state(pop, 1)) and _equal(pc.state(pop, 3), pc.state(pop, 2))
    assert not _equal(pc.state(pop, 1), pc.state(pop, 2))
    # the values: two steps, each drawing for member 0 then member 3, one draw per name in order
    names = tuple(n for n in sweepable_names("td3") if n != "gamma")
    rng = random.Random(5)
    defaults = type(pop)(1, 6, 3, 0.7, device="cpu").hyper(0)
    rows = [dict(defaults, expl_sigma=s, actor_lr=lr) for s, lr in zip(sweep["expl_sigma"], sweep["actor_lr"])]
    assert hist[0]["hyper"] == {n: [r[n] for r in rows] for n in sweepable_names("td3") if n != "gamma"}       # before the first step
    for step in (1, 3):
        for p, s in ((0, 1), (3, 2)):
            rows[p] = dict(rows[s])
            for n in names:
                rows[p][n] = rows[s][n] * (0.8 if rng.random() < 0.5 else 1.2)
        rec = hist[step]
        assert rec["src"] == [1, 1, 2, 2] and [(n["member"], n["source"]) for n in rec["new"]] == [(0, 1), (3, 2)]
        assert [n["hyper"] for n in rec["new"]] == [rows[0], rows[3]]
        assert rec["hyper"] == {n: [r[n] for r in rows] for n in names}
    assert [dict(pop.hyper(p), expl_sigma=rows[p]["expl_sigma"]) for p in range(4)] == rows
    assert hist[2]["hyper"] == hist[1]["hyper"] and not pop.uniform() and pop.entry_point.endswith("_hyper")
