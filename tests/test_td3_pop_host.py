"""CPU tests of the population TD3 update's host side (armenv_td3_pop_update, include/armenv.h): the ctypes struct agrees with the
header, the workspace query is P single workspaces, every argument is validated before any HIP call, FusedTD3Population's stacks
hold what P seeded FusedTD3 learners hold, and the population kernels are in the built code object."""
import ctypes as C

import pytest
import torch

from learner_host import POP_REFUSALS, TD3_NETS as NETS, ctypes_layout, fake_pop_args, header_layout, learner_kernels, refused  # noqa: F401

POP_KERNELS = ("gemm_pop_kernel", "actor_head_pop_kernel", "critic_head_pop_kernel", "actor_back_pop_kernel", "adam_pop_kernel")


def test_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = ctypes_layout(L.ArmEnvTd3PopArgs)
    assert ("members", L.ArmEnvTd3PopArgs.members.offset) in members and any(m.startswith("one.q2_v.") for m, _ in members)
    sizes, offsets = header_layout(L.ArmEnvTd3PopArgs, extra=("sizeof(ArmEnvTd3Args)",))
    assert sizes == [C.sizeof(L.ArmEnvTd3PopArgs), C.sizeof(L.ArmEnvTd3Args)]
    assert offsets == [o for _, o in members], members


def test_the_abi_version_did_not_move():
    from armenv import _lib as L
    assert L.load().armenv_abi_version() == 9


@pytest.mark.parametrize("D", [1, 6, 9, 12])
def test_population_workspace_is_p_single_workspaces(D):
    from armenv import _lib as L
    lib = L.load()
    for B in (1, 64, 257, 2048):
        one = lib.armenv_td3_workspace_bytes(D, 256, B)
        assert one > 0 and one % 256 == 0
        for P in (1, 2, 16, 64):
            assert lib.armenv_td3_pop_workspace_bytes(D, 256, B, P) == P * one, (D, B, P)


def test_population_workspace_refuses_unsupported_sizes():
    from armenv import _lib as L
    lib = L.load()
    assert lib.armenv_td3_pop_workspace_bytes(6, 256, 64, 0) == -1 and lib.armenv_td3_pop_workspace_bytes(6, 256, 64, 65) == -1
    assert lib.armenv_td3_pop_workspace_bytes(6, 128, 64, 2) == -1
    assert lib.armenv_td3_pop_workspace_bytes(13, 256, 64, 2) == -1
    assert lib.armenv_td3_pop_workspace_bytes(6, 256, 0, 2) == -1


@pytest.mark.parametrize("field,mutate", POP_REFUSALS["td3"])
def test_bad_arguments_are_refused_before_any_device_call(field, mutate):
    pa = fake_pop_args("td3")
    mutate(pa)
    assert field in refused("armenv_td3_pop_update", C.byref(pa), None)


def test_a_single_workspace_is_too_small_for_a_population():
    from armenv import _lib as L
    lib = L.load()
    pa = fake_pop_args("td3", P=2)
    pa.one.workspace_bytes = lib.armenv_td3_workspace_bytes(6, 256, 64)
    rc, msg = lib.armenv_td3_pop_update(C.byref(pa), None), lib.armenv_last_error().decode()
    assert rc == -1 and "workspace_bytes" in msg and "armenv_td3_pop_workspace_bytes" in msg, msg


def test_null_args_are_refused():
    from armenv import _lib as L
    lib = L.load()
    rc, msg = lib.armenv_td3_pop_update(None, None), lib.armenv_last_error().decode()
    assert rc == -1 and "args" in msg and "armenv_td3_pop_update" in msg, msg


def _single_nets(agent):
    return [p for n in agent._nets() for p in n.parameters()]


def test_population_members_start_as_seeded_single_learners():
    from armenv.fused_td3 import FusedTD3
    from armenv.fused_td3_pop import FusedTD3Population
    torch.manual_seed(99)
    before = torch.get_rng_state()
    pop = FusedTD3Population(3, 6, 3, 0.7, device="cpu", seed=5)
    assert torch.equal(before, torch.get_rng_state())          # the global CPU generator is where it was
    for p in range(3):
        torch.manual_seed(5 + p)
        single = FusedTD3(6, 3, 0.7, device="cpu")
        m = pop.member(p)
        mine = [q for n in (m.actor, m.critic, m.target_actor, m.target_critic) for q in n.parameters()]
        theirs = _single_nets(single)
        assert len(mine) == len(theirs) == 36
        assert all(torch.equal(x, y) for x, y in zip(mine, theirs)), p
        assert set(m.actor_state_dict()) == set(single.actor_state_dict())
    assert not torch.equal(pop.member(0).actor.fc1.weight, pop.member(1).actor.fc1.weight)
    assert all(t.shape[0] == 3 and t.is_contiguous() for six in pop.stacks.values() for t in six)
    assert sorted(pop.stacks) == sorted(NETS)
    assert all(float(t.abs().max()) == 0.0 for name in NETS if name.endswith(("_m", "_v")) for t in pop.stacks[name])


def test_member_parameters_are_views_into_the_stacks():
    from armenv.fused_td3_pop import FusedTD3Population
    pop = FusedTD3Population(3, 6, 3, 0.7, device="cpu", seed=5)
    W1 = pop.stacks["actor"][0]
    others = W1[[0, 2]].clone()
    with torch.no_grad():
        pop.member(1).actor.fc1.weight.fill_(0.25)
        pop.member(2).critic.fc6.bias.fill_(-3.0)
    assert bool((W1[1] == 0.25).all()) and torch.equal(W1[[0, 2]], others)
    assert float(pop.stacks["q2"][5][2]) == -3.0
    assert pop.member(1).actor.fc1.weight.data_ptr() == W1[1].data_ptr()
    with torch.no_grad():
        pop.stacks["target_actor"][4][0].fill_(7.0)             # ... and the other way round: W3 of member 0's target actor
    assert bool((pop.member(0).target_actor.fc3.weight == 7.0).all())


def test_member_buffers_are_what_the_sampler_accepts():
    """TrajectoryStore.sample(out=...) wants, per key, a contiguous tensor of the batch's shape and dtype on the store's device."""
    from armenv.fused_td3_pop import FusedTD3Population
    pop = FusedTD3Population(3, 9, 3, 0.4, device="cpu")
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


@pytest.mark.parametrize("kw", [dict(state_dim=13), dict(state_dim=0), dict(action_dim=2), dict(hidden_dim=128), dict(members=0),
                                dict(members=65)])
def test_unsupported_shapes_raise(kw):
    from armenv.fused_td3_pop import FusedTD3Population
    a = dict(members=2, state_dim=6, action_dim=3, hidden_dim=256)
    a.update(kw)
    with pytest.raises(ValueError):
        FusedTD3Population(a["members"], a["state_dim"], a["action_dim"], 0.7, hidden_dim=a["hidden_dim"], device="cpu")


def test_population_kernels_are_in_the_code_object(learner_kernels):
    """test_td3_fused_host.py holds all of learner_host.learner_kernels, these included, to no scratch, no atomics and exact f32."""
    assert set(POP_KERNELS) <= set(learner_kernels), sorted(learner_kernels)
    md, ins = learner_kernels["gemm_pop_kernel"]
    assert "v_mfma_f32_32x32x2_f32" in [i.mnem for i in ins]
