"""CPU tests of the fused DADDPG learner's host side (armenv_daddpg_update, include/armenv.h ABI 8): the ctypes struct agrees with the
header, every argument is validated before any HIP call, the workspace query covers the activations and the actor-sized partial
slices, the new kernels are in the built code object, and the training loop's learner choices."""
import ctypes as C

import pytest

from learner_host import DADDPG_NETS as NETS, REFUSALS, ctypes_layout, fake_args, header_layout, learner_kernels  # noqa: F401

DADDPG_KERNELS = ("gemm_kernel", "daddpg_actor_head_kernel", "daddpg_critic_head_kernel", "actor_back_kernel", "adam_kernel")


def test_daddpg_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = ctypes_layout(L.ArmEnvDaddpgArgs)
    assert {m.split(".")[0] for m, _ in members} >= set(NETS) | {"update_actor", "critic_step", "actor_step", "loss_dev"}
    sizes, offsets = header_layout(L.ArmEnvDaddpgArgs, extra=("ARMENV_ABI_VERSION",))
    assert sizes[0] == C.sizeof(L.ArmEnvDaddpgArgs) and sizes[1] == L.ABI_VERSION == 9
    assert offsets == [o for _, o in members], members


@pytest.mark.parametrize("field,mutate", REFUSALS["daddpg"])
def test_daddpg_bad_arguments_are_refused_before_any_device_call(field, mutate):
    from armenv import _lib as L
    lib = L.load()
    a = fake_args("daddpg")
    mutate(a)
    rc, msg = lib.armenv_daddpg_update(C.byref(a), None), lib.armenv_last_error().decode()
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
