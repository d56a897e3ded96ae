"""CPU tests of the fused TD3 learner's host side (armenv_td3_update, include/armenv.h ABI 7): the ctypes structs agree with the
header, every argument is validated before any HIP call, the batch-size limits, and the learner kernels' code objects hold what DESIGN.md section 4 claims
(no scratch, exact-f32 MFMA, no atomics)."""
import ctypes as C

import pytest

from learner_host import REFUSALS, ctypes_layout, fake_args, header_layout, learner_kernels  # noqa: F401

LEARNER_KERNELS = ("gemm_kernel", "actor_head_kernel", "critic_head_kernel", "actor_back_kernel", "adam_kernel")


def test_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = ctypes_layout(L.ArmEnvTd3Args)
    sizes, offsets = header_layout(L.ArmEnvTd3Args, extra=("sizeof(ArmEnvMlpRW)",))
    assert sizes == [C.sizeof(L.ArmEnvTd3Args), C.sizeof(L.ArmEnvMlpRW)]
    assert offsets == [o for _, o in members], members


@pytest.mark.parametrize("field,mutate", REFUSALS["td3"])
def test_bad_arguments_are_refused_before_any_device_call(field, mutate):
    from armenv import _lib as L
    lib = L.load()
    a = fake_args("td3")
    mutate(a)
    rc, msg = lib.armenv_td3_update(C.byref(a), None), lib.armenv_last_error().decode()
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


def test_workspace_query_at_the_batch_limit():
    from armenv import _lib as L
    lib = L.load()
    for D in (1, 6, 12):
        assert lib.armenv_td3_workspace_bytes(D, 256, 2 ** 20) > 0
        assert lib.armenv_td3_workspace_bytes(D, 256, 2 ** 20 + 1) == -1


def test_update_refuses_a_batch_above_the_limit():
    from armenv import _lib as L
    lib, a = L.load(), fake_args("td3")
    a.batch = 2 ** 20 + 1
    rc, msg = lib.armenv_td3_update(C.byref(a), None), lib.armenv_last_error().decode()
    assert rc == -1 and "batch" in msg and "armenv_td3_update" in msg, (rc, msg)


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
