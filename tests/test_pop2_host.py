"""CPU tests of the host side of the DADDPG and DATD3 / DARC population updates (armenv_daddpg_pop_update, armenv_datd3_pop_update,
include/armenv.h): the ctypes structs agree with the header, the workspace queries are P single workspaces, every argument is
validated before any HIP call, the population classes' stacks hold what P seeded single learners hold, and the four population head
kernels are in the built code object."""
import ctypes as C

import pytest
import torch

from learner_host import (AGENTS, POP_REFUSALS, POP_REFUSALS_DATD3, classes, ctypes_layout, fake_pop_args, header_layout,  # noqa: F401
                          learner_kernels, refused)

POP_KERNELS = ("daddpg_actor_head_pop_kernel", "daddpg_critic_head_pop_kernel", "datd3_actor_head_pop_kernel",
               "datd3_critic_head_pop_kernel")
ALGOS = ("daddpg", "datd3")


@pytest.mark.parametrize("algo", ALGOS)
def test_struct_layout_matches_the_header(algo):
    Pop, One, nets = (AGENTS[algo][k] for k in ("pop_args", "args", "nets"))
    members = ctypes_layout(Pop)
    assert ("members", Pop.members.offset) in members and any(m.startswith("one.%s." % nets[-1]) for m, _ in members)
    sizes, offsets = header_layout(Pop, extra=("sizeof(%s)" % One.__name__,))
    assert sizes == [C.sizeof(Pop), C.sizeof(One)]
    assert offsets == [o for _, o in members], members
    assert Pop.members.offset == C.sizeof(One)


def test_the_abi_version_did_not_move():
    from armenv import _lib as L
    assert L.load().armenv_abi_version() == 9 and L.ABI_VERSION == 9


@pytest.mark.parametrize("algo", ALGOS)
def test_population_workspace_is_p_single_workspaces(algo):
    from armenv import _lib as L
    lib = L.load()
    single, pop = getattr(lib, "armenv_%s_workspace_bytes" % algo), getattr(lib, "armenv_%s_pop_workspace_bytes" % algo)
    for D in (6, 9):
        for B in (1, 256, 4097):
            one = single(D, 256, B)
            assert one > 0 and one % 256 == 0
            for P in (1, 2, 16, 64):
                assert pop(D, 256, B, P) == P * one, (D, B, P)


@pytest.mark.parametrize("algo", ALGOS)
def test_population_workspace_refuses_unsupported_sizes(algo):
    from armenv import _lib as L
    pop = getattr(L.load(), "armenv_%s_pop_workspace_bytes" % algo)
    assert pop(6, 256, 64, 0) == -1 and pop(6, 256, 64, 65) == -1
    assert pop(6, 128, 64, 2) == -1
    assert pop(13, 256, 64, 2) == -1 and pop(0, 256, 64, 2) == -1
    assert pop(6, 256, 0, 2) == -1 and pop(6, 256, (1 << 20) + 1, 2) == -1


def _refused(algo, pa):
    return refused("armenv_%s_pop_update" % algo, C.byref(pa) if pa is not None else None, None)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("field,mutate", POP_REFUSALS["daddpg"])          # one table under both keys
def test_bad_arguments_are_refused_before_any_device_call(algo, field, mutate):
    pa = fake_pop_args(algo)
    mutate(pa)
    assert field in _refused(algo, pa)


@pytest.mark.parametrize("field,darc,mutate", POP_REFUSALS_DATD3)
def test_bad_datd3_arguments_are_refused_before_any_device_call(field, darc, mutate):
    pa = fake_pop_args("datd3", darc=darc)
    mutate(pa)
    assert field in _refused("datd3", pa)


@pytest.mark.parametrize("algo", ALGOS)
def test_a_single_workspace_is_too_small_for_a_population(algo):
    from armenv import _lib as L
    pa = fake_pop_args(algo, P=2)
    pa.one.workspace_bytes = getattr(L.load(), "armenv_%s_workspace_bytes" % algo)(6, 256, 64)
    msg = _refused(algo, pa)
    assert "workspace_bytes" in msg and "armenv_%s_pop_workspace_bytes" % algo in msg, msg


@pytest.mark.parametrize("algo", ALGOS)
def test_null_args_are_refused(algo):
    assert "args" in _refused(algo, None)


KINDS = ("daddpg", "datd3", "darc")


@pytest.mark.parametrize("kind", KINDS)
def test_population_members_start_as_seeded_single_learners(kind):
    Pop, Single, _ = classes(kind)
    nets = AGENTS[kind]["nets"]
    torch.manual_seed(99)
    before = torch.get_rng_state()
    pop = Pop(3, 6, 3, 0.7, device="cpu", seed=5)
    assert torch.equal(before, torch.get_rng_state())          # the global CPU generator is where it was
    n_nets = len(nets) // 2
    for p in range(3):
        torch.manual_seed(5 + p)
        single = Single(6, 3, 0.7, device="cpu")
        m = pop.member(p)
        mine = [q for n in m._nets() for q in n.parameters()]
        theirs = [q for n in single._nets() for q in n.parameters()]
        assert len(mine) == len(theirs) == 6 * n_nets
        assert all(torch.equal(x, y) for x, y in zip(mine, theirs)), p
        mine_sd, theirs_sd = m.policy_state_dicts(), single.policy_state_dicts()
        assert len(mine_sd) == len(theirs_sd) == (3 if kind == "daddpg" else 4)
        for a, b in zip(mine_sd, theirs_sd):
            assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert m.actor is m.actor1
        s = torch.rand(6).tolist()
        assert (m.take_action(s) == single.take_action(s)).all()
    assert not torch.equal(pop.member(0).actor1.fc1.weight, pop.member(1).actor1.fc1.weight)
    assert all(t.shape[0] == 3 and t.is_contiguous() for six in pop.stacks.values() for t in six)
    assert sorted(pop.stacks) == sorted(nets) and all(len(six) == 6 for six in pop.stacks.values())
    assert all(float(t.abs().max()) == 0.0 for name in nets if name.endswith(("_m", "_v")) for t in pop.stacks[name])
    assert len(pop._member_state(1)) == len(pop._single_state(single)) == 6 * len(nets)
    assert all(x.shape == y.shape for x, y in zip(pop._member_state(1), pop._single_state(single)))
    assert pop.total_it == 0 and all(getattr(pop, c) == 0 for c in pop._COUNTERS) and len(pop._COUNTERS) == (4 if kind == "daddpg" else 5)
    if kind == "darc":
        assert (pop.q_weight, pop.regularization_weight) == (single.q_weight, single.regularization_weight) == (0.2, 0.005)


@pytest.mark.parametrize("kind", KINDS)
def test_member_parameters_are_views_into_the_stacks(kind):
    Pop, _, _ = classes(kind)
    pop = Pop(3, 6, 3, 0.7, device="cpu", seed=5)
    critic = "critic" if kind == "daddpg" else "critic2"
    W1 = pop.stacks["actor2"][0]
    others = W1[[0, 2]].clone()
    with torch.no_grad():
        pop.member(1).actor2.fc1.weight.fill_(0.25)
        getattr(pop.member(2), critic).fc3.bias.fill_(-3.0)
    assert bool((W1[1] == 0.25).all()) and torch.equal(W1[[0, 2]], others)
    assert float(pop.stacks[critic][5][2]) == -3.0
    assert pop.member(1).actor2.fc1.weight.data_ptr() == W1[1].data_ptr()
    with torch.no_grad():
        pop.stacks["target_" + critic][4][0].fill_(7.0)         # ... and the other way round: W3 of member 0's target critic
    assert bool((getattr(pop.member(0), "target_" + critic).fc3.weight == 7.0).all())


@pytest.mark.parametrize("kind", KINDS)
def test_member_buffers_are_what_the_sampler_accepts(kind):
    """TrajectoryStore.sample(out=...) wants, per key, a contiguous tensor of the batch's shape and dtype on the store's device."""
    Pop, _, _ = classes(kind)
    pop = Pop(3, 9, 3, 0.4, device="cpu")
    with pytest.raises(RuntimeError):
        pop.member_buffers(0)
    B, D = 257, 9
    stacked = pop.batch_buffers(B)
    want = dict(states=((B, D), torch.float32), actions=((B, 3), torch.float32), next_states=((B, D), torch.float32),
                rewards=((B,), torch.float32), dones=((B,), torch.uint8))
    for p in range(3):
        out = pop.member_buffers(p)
        assert set(out) == set(want)
        for k, (shape, dt) in want.items():
            t = out[k]
            assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous() and t.device == stacked[k].device, (p, k)
            assert t.data_ptr() == stacked[k][p].data_ptr() and tuple(stacked[k].shape) == (3,) + shape


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kw", [dict(state_dim=13), dict(state_dim=0), dict(action_dim=2), dict(hidden_dim=128), dict(members=0),
                                dict(members=65)])
def test_unsupported_shapes_raise(kind, kw):
    Pop, _, _ = classes(kind)
    a = dict(members=2, state_dim=6, action_dim=3, hidden_dim=256)
    a.update(kw)
    with pytest.raises(ValueError):
        Pop(a["members"], a["state_dim"], a["action_dim"], 0.7, hidden_dim=a["hidden_dim"], device="cpu")


@pytest.mark.parametrize("algo", ("td3", "daddpg", "datd3", "darc"))
def test_a_refused_call_leaves_every_counter_at_zero(algo):
    """A batch of 0 rows, which the workspace query refuses, and a `noise` of the wrong shape raise from `train` (DATD3 / DARC: from
    `update` too) before total_it or a step number moves -- in the single learner as in a population.  No device is touched."""
    from armenv.fused_td3 import FusedTD3
    Pop, Single, _ = classes(algo)
    two_updates = algo in ("datd3", "darc")
    for learner, lead in ((Single(6, 3, 0.7, device="cpu"), ()), (Pop(2, 6, 3, 0.7, device="cpu"), (2,))):
        def batch(B):
            return dict(states=torch.zeros(*lead, B, 6), actions=torch.zeros(*lead, B, 3), next_states=torch.zeros(*lead, B, 6),
                        rewards=torch.zeros(*lead, B), dones=torch.zeros(*lead, B, dtype=torch.uint8))

        def counters():
            return {k: v for k, v in vars(learner).items() if k == "total_it" or k.endswith("_step")}
        assert set(counters()) == set(learner._COUNTERS) and len(counters()) == dict(td3=3, daddpg=4, datd3=5, darc=5)[algo]
        assert tuple(batch(0)["states"].shape) == lead + (0, 6)
        calls = [lambda: learner.train(batch(0))]
        if two_updates:
            calls += [lambda: learner.update(batch(0)), lambda: learner.update(batch(0), update_a1=False)]
        for call in calls:
            with pytest.raises(ValueError):
                call()
            assert all(v == 0 for v in counters().values()), counters()
        if algo == "daddpg":
            continue                                            # takes no noise
        # TD3's single learner keeps the AssertionError it always raised for this
        error = AssertionError if isinstance(learner, FusedTD3) else ValueError
        good, bad = torch.zeros(*lead, 4, 3), torch.zeros(*lead, 5, 3)
        calls = [lambda: learner.train(batch(4), noise=(good, bad) if two_updates else bad)]
        if two_updates:
            calls += [lambda: learner.train(batch(4), noise=(bad, good)), lambda: learner.update(batch(4), noise=bad)]
        for call in calls:
            with pytest.raises(error):
                call()
            assert all(v == 0 for v in counters().values()), counters()


def test_train_pop_refuses_an_unknown_agent():
    from armenv.train_pop import ALGOS as algos, train_reach_population
    assert algos == ("td3", "daddpg", "datd3", "darc")
    with pytest.raises(ValueError):
        train_reach_population(members=1, iterations=0, algo="ddpg")


def test_population_head_kernels_are_in_the_code_object(learner_kernels):
    """test_td3_fused_host.py holds all of learner_host.learner_kernels, these included, to no scratch, no atomics and exact f32; here:
    they exist, beside their single forms, and take the member from the grid's second dimension."""
    assert set(POP_KERNELS) <= set(learner_kernels), sorted(learner_kernels)
    assert {k.replace("_pop_kernel", "_kernel") for k in POP_KERNELS} <= set(learner_kernels)
    for k in POP_KERNELS:
        md, ins = learner_kernels[k]
        assert md["scratch"] == 0 and md["lds"] == 0 and len(ins) > 0, (k, md)
