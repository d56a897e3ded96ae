"""CPU tests of the population TD3 update's host side (armenv_td3_pop_update, include/armenv.h): the ctypes struct agrees with the
header, the workspace query is P single workspaces, every argument is validated before any HIP call, FusedTD3Population's stacks
hold what P seeded FusedTD3 learners hold, and the population kernels are in the built code object."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import isa  # noqa: E402

HEADER_DIR = os.path.join(ROOT, "include")
POP_KERNELS = ("gemm_pop_kernel", "actor_head_pop_kernel", "critic_head_pop_kernel", "actor_back_pop_kernel", "adam_pop_kernel")
NETS = ("actor", "q1", "q2", "target_actor", "target_q1", "target_q2", "actor_m", "actor_v", "q1_m", "q1_v", "q2_m", "q2_v")


def _ctypes_layout(struct, prefix=""):
    """[(C member path, offset)] of every scalar member of a ctypes struct, nested structs flattened"""
    out = []
    for name, typ in struct._fields_:
        off = getattr(struct, name).offset
        if isinstance(typ, type) and issubclass(typ, C.Structure):
            out += [(f"{prefix}{name}.{k}", off + o) for k, o in _ctypes_layout(typ, "")]
        else:
            out.append((prefix + name, off))
    return out


def test_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = _ctypes_layout(L.ArmEnvTd3PopArgs)
    assert ("members", L.ArmEnvTd3PopArgs.members.offset) in members and any(m.startswith("one.q2_v.") for m, _ in members)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "armenv.h"', "int main(void) {",
             '  printf("%zu %zu\\n", sizeof(ArmEnvTd3PopArgs), sizeof(ArmEnvTd3Args));']
    lines += ['  printf("%%zu\\n", offsetof(ArmEnvTd3PopArgs, %s));' % m for m, _ in members]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-I", HEADER_DIR, "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert int(out[0]) == C.sizeof(L.ArmEnvTd3PopArgs) and int(out[1]) == C.sizeof(L.ArmEnvTd3Args)
    assert [int(x) for x in out[2:]] == [o for _, o in members], members


def test_the_abi_version_did_not_move():
    from armenv import _lib as L
    assert L.load().armenv_abi_version() == 8


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


def _args(P=3, B=64, D=6):
    """Arguments that pass every check but the one a test breaks: fake (never dereferenced) 16-byte aligned device pointers.
    NOT to be passed unmodified -- a valid set would be enqueued."""
    from armenv import _lib as L
    pa = L.ArmEnvTd3PopArgs()
    pa.members = P
    a = pa.one
    a.device, a.state_dim, a.action_dim, a.hidden_dim, a.batch = 0, D, 3, 256, B
    a.action_bound, a.gamma, a.tau, a.policy_noise, a.noise_clip = 0.7, 0.98, 0.005, 0.2, 0.5
    a.actor_lr, a.critic_lr, a.beta1, a.beta2, a.eps = 1e-3, 1e-3, 0.9, 0.999, 1e-8
    a.critic_step, a.actor_step, a.with_actor = 1, 1, 1
    addr = [0x10000000]

    def ptr():
        addr[0] += 0x1000000
        return addr[0]
    for net in NETS:
        m = getattr(a, net)
        for k in ("W1", "b1", "W2", "b2", "W3", "b3"):
            setattr(m, k, ptr())
    for k in ("states_dev", "actions_dev", "next_states_dev", "rewards_dev", "dones_dev", "workspace_dev"):
        setattr(a, k, ptr())
    a.workspace_bytes = L.load().armenv_td3_pop_workspace_bytes(D, 256, B, P)
    assert a.workspace_bytes > 0
    return pa


def _one(field, value):
    return lambda pa: setattr(pa.one, field, value)


@pytest.mark.parametrize("field,mutate", [
    ("members", lambda pa: setattr(pa, "members", 0)),
    ("members", lambda pa: setattr(pa, "members", 65)),
    ("target_q2", lambda pa: setattr(pa.one.target_q2, "W2", None)),
    ("states_dev", _one("states_dev", None)),
    ("workspace_bytes", lambda pa: setattr(pa.one, "workspace_bytes", pa.one.workspace_bytes - 1)),
    ("gamma", _one("gamma", float("nan"))),
    ("batch", _one("batch", 0)),
    ("hidden_dim", _one("hidden_dim", 128)),
])
def test_bad_arguments_are_refused_before_any_device_call(field, mutate):
    from armenv import _lib as L
    lib = L.load()
    pa = _args()
    mutate(pa)
    rc, msg = lib.armenv_td3_pop_update(C.byref(pa), None), lib.armenv_last_error().decode()
    assert rc == -1, (rc, msg)                       # ARMENV_EINVAL, not ENODEV: nothing touched the device
    assert field in msg and msg.startswith("armenv_td3_pop_update"), msg


def test_a_single_workspace_is_too_small_for_a_population():
    from armenv import _lib as L
    lib = L.load()
    pa = _args(P=2)
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


@pytest.fixture(scope="module")
def learner_kernels():
    if not os.path.exists(isa.LIB):
        pytest.skip("libarmenv.so is not built")
    if not os.path.exists(os.path.join(isa.LLVM, "llvm-objdump")):
        pytest.skip("the ROCm LLVM tools (llvm-objdump, llvm-readelf) are not installed")
    rows = [r for r in isa.all_kernels() if "armenv::learner::" in r[1]]
    return {dm.split("armenv::learner::")[1].split("(")[0]: (md, ins) for _, dm, md, ins in rows}


def test_population_kernels_are_in_the_code_object(learner_kernels):
    """test_td3_fused_host.py holds every armenv::learner:: kernel, these included, to no scratch, no atomics and exact f32."""
    assert set(POP_KERNELS) <= set(learner_kernels), sorted(learner_kernels)
    md, ins = learner_kernels["gemm_pop_kernel"]
    assert "v_mfma_f32_32x32x2_f32" in [i.mnem for i in ins]
