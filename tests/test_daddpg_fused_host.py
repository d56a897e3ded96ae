"""CPU tests of the fused DADDPG learner's host side (armenv_daddpg_update, include/armenv.h ABI 8): the ctypes struct agrees with the
header, every argument is validated before any HIP call, the workspace query covers the activations and the actor-sized partial
slices, the new kernels are in the built code object, and the training loop's learner choices."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import isa  # noqa: E402

HEADER_DIR = os.path.join(ROOT, "include")
DADDPG_KERNELS = ("gemm_kernel", "daddpg_actor_head_kernel", "daddpg_critic_head_kernel", "actor_back_kernel", "adam_kernel")
NETS = ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic",
        "actor1_m", "actor1_v", "actor2_m", "actor2_v", "critic_m", "critic_v")


def _ctypes_layout(struct, prefix=""):
    """[(C member path, offset)] of every scalar member of a ctypes struct, nested structs flattened"""
    out = []
    for name, typ in struct._fields_:
        off = getattr(struct, name).offset
        if isinstance(typ, type) and issubclass(typ, C.Structure):
            out += [(f"{prefix}{name}.{k}", off + o) for k, o in _ctypes_layout(typ)]
        else:
            out.append((prefix + name, off))
    return out


def test_daddpg_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = _ctypes_layout(L.ArmEnvDaddpgArgs)
    assert {m.split(".")[0] for m, _ in members} >= set(NETS) | {"update_actor", "critic_step", "actor_step", "loss_dev"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "armenv.h"', "int main(void) {",
             '  printf("%zu %d\\n", sizeof(ArmEnvDaddpgArgs), ARMENV_ABI_VERSION);']
    lines += ['  printf("%%zu\\n", offsetof(ArmEnvDaddpgArgs, %s));' % m for m, _ in members]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-I", HEADER_DIR, "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert int(out[0]) == C.sizeof(L.ArmEnvDaddpgArgs) and int(out[1]) == L.ABI_VERSION == 8
    assert [int(x) for x in out[2:]] == [o for _, o in members], members


def _args(B=64, D=6):
    """Arguments that pass every check but the one a test breaks: fake (never dereferenced) 16-byte aligned device pointers.
    NOT to be passed unmodified -- a valid set would be enqueued."""
    from armenv import _lib as L
    a = L.ArmEnvDaddpgArgs()
    a.device, a.state_dim, a.action_dim, a.hidden_dim, a.batch = 0, D, 3, 256, B
    a.action_bound, a.gamma, a.tau = 0.7, 0.98, 0.005
    a.actor_lr, a.critic_lr, a.beta1, a.beta2, a.eps = 1e-3, 1e-3, 0.9, 0.999, 1e-8
    a.critic_step, a.actor_step, a.update_actor = 1, 1, 2
    addr = [0x10000]

    def ptr():
        addr[0] += 0x1000
        return addr[0]
    for net in NETS:
        m = getattr(a, net)
        for k in ("W1", "b1", "W2", "b2", "W3", "b3"):
            setattr(m, k, ptr())
    for k in ("states_dev", "actions_dev", "next_states_dev", "rewards_dev", "dones_dev", "workspace_dev"):
        setattr(a, k, ptr())
    a.workspace_bytes = L.load().armenv_daddpg_workspace_bytes(D, 256, B)
    assert a.workspace_bytes > 0
    return a


def _breaks(mutate):
    from armenv import _lib as L
    lib = L.load()
    a = _args()
    mutate(a)
    rc = lib.armenv_daddpg_update(C.byref(a), None)
    return rc, lib.armenv_last_error().decode()


@pytest.mark.parametrize("field,mutate", [
    ("batch", lambda a: setattr(a, "batch", 0)),
    ("batch", lambda a: setattr(a, "batch", (1 << 20) + 1)),
    ("hidden_dim", lambda a: setattr(a, "hidden_dim", 128)),
    ("state_dim", lambda a: setattr(a, "state_dim", 0)),
    ("state_dim", lambda a: setattr(a, "state_dim", 13)),
    ("action_dim", lambda a: setattr(a, "action_dim", 2)),
    ("update_actor", lambda a: setattr(a, "update_actor", 0)),
    ("update_actor", lambda a: setattr(a, "update_actor", 3)),
    ("critic_step", lambda a: setattr(a, "critic_step", 0)),
    ("actor_step", lambda a: setattr(a, "actor_step", 0)),
    ("gamma", lambda a: setattr(a, "gamma", float("nan"))),
    ("tau", lambda a: setattr(a, "tau", 1.5)),
    ("beta1", lambda a: setattr(a, "beta1", 1.0)),
    ("eps", lambda a: setattr(a, "eps", 0.0)),
    ("actor1", lambda a: setattr(a.actor1, "W1", None)),
    ("actor2", lambda a: setattr(a.actor2, "b3", None)),
    ("critic", lambda a: setattr(a.critic, "W2", None)),
    ("target_actor2", lambda a: setattr(a.target_actor2, "W3", None)),
    ("target_critic", lambda a: setattr(a.target_critic, "b1", a.target_critic.b1 + 4)),      # misaligned
    ("actor1_m", lambda a: setattr(a.actor1_m, "b2", None)),
    ("actor2_v", lambda a: setattr(a.actor2_v, "W1", a.actor2_v.W1 + 8)),                    # misaligned
    ("critic_v", lambda a: setattr(a.critic_v, "b3", None)),
    ("states_dev", lambda a: setattr(a, "states_dev", None)),
    ("dones_dev", lambda a: setattr(a, "dones_dev", None)),
    ("workspace_dev", lambda a: setattr(a, "workspace_dev", None)),
    ("workspace_dev", lambda a: setattr(a, "workspace_dev", a.workspace_dev + 4)),
    ("workspace_bytes", lambda a: setattr(a, "workspace_bytes", a.workspace_bytes - 1)),
])
def test_daddpg_bad_arguments_are_refused_before_any_device_call(field, mutate):
    rc, msg = _breaks(mutate)
    assert rc == -1, (rc, msg)                       # ARMENV_EINVAL, not ENODEV: nothing touched the device
    assert field in msg and "armenv_daddpg_update" in msg, msg


def test_daddpg_null_args_are_refused():
    from armenv import _lib as L
    lib = L.load()
    assert lib.armenv_daddpg_update(None, None) == -1
    assert "armenv_daddpg_update" in lib.armenv_last_error().decode()


def test_daddpg_workspace_size_queries():
    from armenv import _lib as L
    lib = L.load()
    q = lib.armenv_daddpg_workspace_bytes
    assert q(6, 128, 64) == -1 and q(0, 256, 64) == -1 and q(13, 256, 64) == -1
    assert q(6, 256, 0) == -1 and q(6, 256, (1 << 20) + 1) == -1
    assert q(1, 256, 1) > 0 and q(12, 256, 1 << 20) > 0
    sizes = [q(6, 256, B) for B in (1, 64, 256, 257, 1000, 2048, 4097, 1 << 20)]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    H = 256
    for B in (1, 1000, 2048, 4097):
        S = -(-B // 256)
        # the fourteen [B][256] activations and deltas, and S partial slices of at least the ACTOR's size: W3 | b3 [3][257],
        # W2 | b2 [256][257], W1 | b1 [256][16] -- larger than the one critic's [1][257] + [256][257] + [256][16]
        actor_slice = 3 * (H + 1) + H * (H + 1) + 16 * H
        assert q(6, 256, B) >= 4 * (14 * B * H + S * actor_slice), B
        assert q(9, 256, B) == q(6, 256, B)


@pytest.fixture(scope="module")
def learner_kernels():
    if not os.path.exists(isa.LIB):
        pytest.skip("libarmenv.so is not built")
    if not os.path.exists(os.path.join(isa.LLVM, "llvm-objdump")):
        pytest.skip("the ROCm LLVM tools (llvm-objdump, llvm-readelf) are not installed")
    rows = [r for r in isa.all_kernels() if "armenv::learner::" in r[1]]
    return {dm.split("armenv::learner::")[1].split("(")[0]: (md, ins) for _, dm, md, ins in rows}


def test_daddpg_kernels_are_in_the_code_object(learner_kernels):
    assert set(DADDPG_KERNELS) <= set(learner_kernels), sorted(learner_kernels)
    for name in ("daddpg_actor_head_kernel", "daddpg_critic_head_kernel"):
        md, ins = learner_kernels[name]
        assert md["scratch"] == 0 and md["spill_vgpr"] == 0 and ins, (name, md)
        assert not [i.mnem for i in ins if "atomic" in i.mnem], name


def test_learner_choices_of_the_training_loop():
    """learner="fused" is each agent's own fused update; "hip" stays the fused TD3 update (td3 only); others are refused."""
    from armenv import train
    from armenv.fused_daddpg import FusedDADDPG
    from armenv.fused_td3 import FusedTD3
    for algo in ("td3", "daddpg"):
        train._check_learner(algo, "fused")
        train._check_learner(algo, "torch")
    train._check_learner("td3", "hip")
    with pytest.raises(ValueError):
        train._check_learner("daddpg", "hip")
    with pytest.raises(ValueError):
        train._check_learner("daddpg", "triton")
    assert FusedDADDPG.__name__ == "FusedDADDPG" and FusedTD3.__name__ == "FusedTD3"


def test_fused_daddpg_refuses_unsupported_shapes():
    from armenv.fused_daddpg import FusedDADDPG
    for kw in (dict(state_dim=13, action_dim=3), dict(state_dim=6, action_dim=2), dict(state_dim=6, action_dim=3, hidden_dim=128)):
        with pytest.raises(ValueError):
            FusedDADDPG(action_bound=0.7, device="cpu", **kw)
