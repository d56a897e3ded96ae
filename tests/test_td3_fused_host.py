"""CPU tests of the fused TD3 learner's host side (armenv_td3_update, include/armenv.h ABI 7): the ctypes structs agree with the
header, every argument is validated before any HIP call, and the learner kernels' code objects hold what DESIGN.md section 4 claims
(no scratch, exact-f32 MFMA, no atomics)."""
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
LEARNER_KERNELS = ("gemm_kernel", "actor_head_kernel", "critic_head_kernel", "actor_back_kernel", "adam_kernel")


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


def test_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = _ctypes_layout(L.ArmEnvTd3Args)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "armenv.h"', "int main(void) {",
             '  printf("%zu %zu\\n", sizeof(ArmEnvTd3Args), sizeof(ArmEnvMlpRW));']
    lines += ['  printf("%%zu\\n", offsetof(ArmEnvTd3Args, %s));' % m for m, _ in members]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-I", HEADER_DIR, "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert int(out[0]) == C.sizeof(L.ArmEnvTd3Args) and int(out[1]) == C.sizeof(L.ArmEnvMlpRW)
    assert [int(x) for x in out[2:]] == [o for _, o in members], members


def _args(B=64, D=6):
    """Arguments that pass every check but the one a test breaks: fake (never dereferenced) 16-byte aligned device pointers.
    NOT to be passed unmodified -- a valid set would be enqueued."""
    from armenv import _lib as L
    a = L.ArmEnvTd3Args()
    a.device, a.state_dim, a.action_dim, a.hidden_dim, a.batch = 0, D, 3, 256, B
    a.action_bound, a.gamma, a.tau, a.policy_noise, a.noise_clip = 0.7, 0.98, 0.005, 0.2, 0.5
    a.actor_lr, a.critic_lr, a.beta1, a.beta2, a.eps = 1e-3, 1e-3, 0.9, 0.999, 1e-8
    a.critic_step, a.actor_step, a.with_actor = 1, 1, 1
    addr = [0x10000]

    def ptr():
        addr[0] += 0x1000
        return addr[0]
    for net in ("actor", "q1", "q2", "target_actor", "target_q1", "target_q2", "actor_m", "actor_v", "q1_m", "q1_v", "q2_m", "q2_v"):
        m = getattr(a, net)
        for k in ("W1", "b1", "W2", "b2", "W3", "b3"):
            setattr(m, k, ptr())
    for k in ("states_dev", "actions_dev", "next_states_dev", "rewards_dev", "dones_dev", "workspace_dev"):
        setattr(a, k, ptr())
    a.workspace_bytes = L.load().armenv_td3_workspace_bytes(D, 256, B)
    assert a.workspace_bytes > 0
    return a


def _breaks(mutate):
    from armenv import _lib as L
    lib = L.load()
    a = _args()
    mutate(a)
    rc = lib.armenv_td3_update(C.byref(a), None)
    return rc, lib.armenv_last_error().decode()


@pytest.mark.parametrize("field,mutate", [
    ("batch", lambda a: setattr(a, "batch", 0)),
    ("hidden_dim", lambda a: setattr(a, "hidden_dim", 128)),
    ("state_dim", lambda a: setattr(a, "state_dim", 0)),
    ("state_dim", lambda a: setattr(a, "state_dim", 13)),
    ("q2", lambda a: setattr(a.q2, "W2", None)),
    ("actor_v", lambda a: setattr(a.actor_v, "b3", None)),
    ("states_dev", lambda a: setattr(a, "states_dev", None)),
    ("dones_dev", lambda a: setattr(a, "dones_dev", None)),
    ("workspace_dev", lambda a: setattr(a, "workspace_dev", None)),
    ("workspace_bytes", lambda a: setattr(a, "workspace_bytes", a.workspace_bytes - 1)),
    ("action_dim", lambda a: setattr(a, "action_dim", 2)),
    ("gamma", lambda a: setattr(a, "gamma", float("nan"))),
])
def test_bad_arguments_are_refused_before_any_device_call(field, mutate):
    from armenv import _lib as L
    rc, msg = _breaks(mutate)
    assert rc == -1, (rc, msg)                       # ARMENV_EINVAL, not ENODEV: nothing touched the device
    assert field in msg and "armenv_td3_update" in msg, msg


def test_workspace_size_queries():
    from armenv import _lib as L
    lib = L.load()
    assert lib.armenv_td3_workspace_bytes(6, 128, 64) == -1
    assert lib.armenv_td3_workspace_bytes(0, 256, 64) == -1 and lib.armenv_td3_workspace_bytes(13, 256, 64) == -1
    assert lib.armenv_td3_workspace_bytes(6, 256, 0) == -1
    small, big = lib.armenv_td3_workspace_bytes(6, 256, 1000), lib.armenv_td3_workspace_bytes(6, 256, 2048)
    assert 0 < small < big and small % 256 == 0
    assert big >= 16 * 2048 * 256 * 4             # at least the sixteen [B][256] activations and deltas


@pytest.fixture(scope="module")
def learner_kernels():
    if not os.path.exists(isa.LIB):
        pytest.skip("libarmenv.so is not built")
    if not os.path.exists(os.path.join(isa.LLVM, "llvm-objdump")):
        pytest.skip("the ROCm LLVM tools (llvm-objdump, llvm-readelf) are not installed")
    rows = [r for r in isa.all_kernels() if "armenv::learner::" in r[1]]
    return {dm.split("armenv::learner::")[1].split("(")[0]: (md, ins) for _, dm, md, ins in rows}


def test_learner_kernels_are_present_without_scratch(learner_kernels):
    assert set(LEARNER_KERNELS) <= set(learner_kernels), sorted(learner_kernels)
    for name, (md, ins) in learner_kernels.items():
        assert md["scratch"] == 0 and md["spill_vgpr"] == 0, (name, md)
        assert ins, name


def test_learner_contractions_are_exact_f32_mfma(learner_kernels):
    md, ins = learner_kernels["gemm_kernel"]
    mnems = [i.mnem for i in ins]
    assert "v_mfma_f32_32x32x2_f32" in mnems, sorted(set(m for m in mnems if "mfma" in m))
    for name, (md, ins) in learner_kernels.items():
        low = [m for m in (i.mnem for i in ins) if m.startswith("v_mfma") and ("f16" in m or "bf16" in m or "xf32" in m)]
        assert not low, (name, low)


def test_learner_kernels_have_no_atomics(learner_kernels):
    for name, (md, ins) in learner_kernels.items():
        atomics = [i.mnem for i in ins if i.mnem.startswith(("global_atomic", "buffer_atomic", "flat_atomic", "ds_add"))]
        assert not atomics, (name, atomics)
