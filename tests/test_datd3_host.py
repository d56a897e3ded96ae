"""CPU tests of the DATD3 / DARC learners: the torch learners (armenv.datd3) against the reference's recorded runs G17 / G18, which
tensors an update may touch, DARC's target arithmetic; and the fused update's host side (armenv_datd3_update, include/armenv.h): the
ctypes struct agrees with the header, every argument is validated before any HIP call, the workspace query, the new kernels in the
built code object, and the training loop's learner choices."""
import ctypes as C

import numpy as np
import pytest

from datd3_golden import NETS, batch, expected_losses, load_train_fixture
from learner_host import DATD3_NETS as ALL_NETS, REFUSALS, ctypes_layout, fake_args, header_layout, learner_kernels  # noqa: F401


@pytest.mark.parametrize("algo", ["datd3", "darc"])
def test_torch_learner_reproduces_the_reference_updates(algo):
    """G17 / G18: four train() calls = eight updates of DATD3_MLP / DARC_MLP reproduced by armenv.datd3 on the CPU from
    torch.manual_seed(0) (creation order actor1, actor2, critic1, critic2) with the recorded noise: every loss to 2e-6 relative, every
    tensor of the eight nets with >= 99.9 % of its elements within 2e-6 and none beyond 2e-3 (test_host_logic.py's DADDPG bounds)."""
    import torch
    from armenv.datd3 import DARC, DATD3
    darc = algo == "darc"
    g = load_train_fixture(algo + "_train_seed0")
    assert g["noise"].shape == (8, 64, 3) and g["mse"].shape == ((8, 2) if darc else (8,))
    torch.manual_seed(0)
    agent = (DARC if darc else DATD3)(6, 3, 0.7, device="cpu")
    got = []
    for i in range(4):
        noise = tuple(torch.from_numpy(g["noise"][2 * i + j]) for j in (0, 1))
        losses = agent.train(batch(g, i), noise=noise)
        assert all(x.dim() == 0 for x in losses)
        got += [float(x) for x in losses]
    assert agent.total_it == 8
    for i, (have, want) in enumerate(zip(got, expected_losses(g, darc))):
        print(algo, "update", i, "loss", have, "recorded", want)
        assert abs(have - want) < 2e-6 * max(1.0, abs(want)), (i, have, want)
    for name in NETS:
        for k, v in getattr(agent, name).state_dict().items():
            d = np.abs(v.numpy() - g[f"{name}__{k.replace('.', '_')}"])
            print(algo, name, k, "within 2e-6:", (d < 2e-6).mean(), "max", d.max())
            assert (d < 2e-6).mean() >= 0.999 and d.max() <= 2e-3, (name, k, (d < 2e-6).mean(), d.max())
    a1, a2, c1, c2 = agent.policy_state_dicts()
    assert tuple(a2["fc1.weight"].shape) == (256, 6) and tuple(c2["fc1.weight"].shape) == (256, 9)
    assert agent.take_action(g["b0_states"][0]).shape == (3,)


def _torch_state(agent):
    out = {}
    for name in NETS:
        for k, v in getattr(agent, name).state_dict().items():
            out[f"{name}.{k}"] = v.clone()
    for name in NETS[:4]:
        opt = getattr(agent, name + "_opt")
        for i, p in enumerate(getattr(agent, name).parameters()):
            for k, v in opt.state.get(p, {}).items():
                out[f"{name}_opt.{i}.{k}"] = v.clone() if hasattr(v, "clone") else v
    return out


@pytest.mark.parametrize("algo", ["datd3", "darc"])
def test_an_update_touches_its_own_actor_and_critic_only(algo):
    """After update(k) the other actor, the other critic, their optimiser state and their targets are torch.equal to before -- for
    DARC too, whose other critic sees gradient -- and what update k owns has moved."""
    import torch
    from armenv.datd3 import DARC, DATD3
    g = load_train_fixture("datd3_train_seed0")
    torch.manual_seed(5)
    agent = (DARC if algo == "darc" else DATD3)(6, 3, 0.7, device="cpu")
    agent.train(batch(g, 0))                     # optimiser state exists for all four
    for n, k in enumerate((1, 2, 2, 1)):
        before = _torch_state(agent)
        agent.update(batch(g, 1 + n % 3), k == 1)
        after = _torch_state(agent)
        o = 3 - k
        still = tuple(s % o for s in ("actor%d.", "critic%d.", "actor%d_opt.", "critic%d_opt.", "target_actor%d.", "target_critic%d."))
        moved = tuple(s % k for s in ("actor%d.", "critic%d.", "target_actor%d.", "target_critic%d."))
        assert set(before) == set(after)
        for key in before:
            if key.startswith(still):
                assert torch.equal(torch.as_tensor(before[key]), torch.as_tensor(after[key])), (k, key)
            if key.startswith(moved):
                assert not torch.equal(before[key], after[key]), (k, key)
    assert agent.total_it == 6


def test_darc_target_is_the_rounded_mix_not_T():
    """DARC with regularization_weight = 0 differs from DATD3 only through the rounding of q_weight T + (1 - q_weight) T: its target
    value is that expression bit for bit, differs from T in at least one row of the batch, and one update's parameters differ from
    DATD3's by no more than that rounding can carry through one Adam step (lr-sized at most)."""
    import torch
    from armenv.datd3 import DARC, DATD3
    g = load_train_fixture("darc_train_seed0")
    torch.manual_seed(0)
    a = DATD3(6, 3, 0.7, device="cpu")
    torch.manual_seed(0)
    b = DARC(6, 3, 0.7, device="cpu", regularization_weight=0.0)
    bt = batch(g, 0)
    noise = torch.from_numpy(g["noise"][0])
    with torch.no_grad():
        s2 = bt["next_states"]
        nz = (noise * 0.2).clamp(-0.5, 0.5)
        t = torch.min(b.target_critic1(s2, (b.target_actor1(s2) + nz).clamp(-0.7, 0.7)),
                      b.target_critic2(s2, (b.target_actor2(s2) + nz).clamp(-0.7, 0.7)))
        mix = b._target_value(t)
    assert torch.equal(mix, 0.2 * t + (1.0 - 0.2) * t) and torch.equal(a._target_value(t), t)
    assert int((mix != t).sum()) >= 1, "the batch must hold a row where the rounded mix differs from T"
    assert float((mix - t).abs().max()) <= 2 ** -22 * float(t.abs().max())
    la, lb = a.update(bt, True, noise), b.update(bt, True, noise)
    assert abs(float(la) - float(lb)) < 1e-6 * abs(float(la))
    for p, q in zip(a.critic1.parameters(), b.critic1.parameters()):
        assert float((p - q).detach().abs().max()) <= 2.1e-3          # one Adam step moves an element by at most lr, either way


def test_datd3_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = ctypes_layout(L.ArmEnvDatd3Args)
    assert ALL_NETS[:8] == NETS and {m.split(".")[0] for m, _ in members} >= set(ALL_NETS) | {
        "update_actor", "darc", "q_weight", "regularization_weight", "policy_noise", "noise_clip", "seed", "draw", "noise_dev",
        "critic_step", "actor_step", "loss_dev"}
    sizes, offsets = header_layout(L.ArmEnvDatd3Args, extra=("ARMENV_ABI_VERSION",))
    assert sizes[0] == C.sizeof(L.ArmEnvDatd3Args) and sizes[1] == L.ABI_VERSION == 9
    assert offsets == [o for _, o in members], members


@pytest.mark.parametrize("field,mutate", REFUSALS["datd3"])
def test_datd3_bad_arguments_are_refused_before_any_device_call(field, mutate):
    from armenv import _lib as L
    lib = L.load()
    a = fake_args("darc")
    mutate(a)
    rc, msg = lib.armenv_datd3_update(C.byref(a), None), lib.armenv_last_error().decode()
    assert rc == -1, (rc, msg)                       # ARMENV_EINVAL, not ENODEV: nothing touched the device
    assert field in msg and "armenv_datd3_update" in msg, msg


def test_datd3_null_args_are_refused():
    from armenv import _lib as L
    lib = L.load()
    assert lib.armenv_datd3_update(None, None) == -1
    assert "armenv_datd3_update" in lib.armenv_last_error().decode()


def test_datd3_workspace_size_queries():
    from armenv import _lib as L
    lib = L.load()
    q = lib.armenv_datd3_workspace_bytes
    assert q(6, 128, 64) == -1 and q(0, 256, 64) == -1 and q(13, 256, 64) == -1
    assert q(6, 256, 0) == -1 and q(6, 256, (1 << 20) + 1) == -1
    assert q(1, 256, 1) > 0 and q(12, 256, 1 << 20) > 0
    sizes = [q(6, 256, B) for B in (1, 64, 256, 257, 1000, 2048, 4097, 1 << 20)]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    H = 256
    for B in (1, 1000, 2048, 4097):
        S = -(-B // 256)
        # DADDPG's fourteen [B][256] activations and deltas plus the other critic's two hidden layers (DARC), S partial slices of
        # the ACTOR's size (W3 | b3 [3][257], W2 | b2 [256][257], W1 | b1 [256][16]) and DARC's two loss columns
        actor_slice = 3 * (H + 1) + H * (H + 1) + 16 * H
        assert q(6, 256, B) >= 4 * (16 * B * H + S * actor_slice + 2 * B), B
        assert q(6, 256, B) >= lib.armenv_daddpg_workspace_bytes(6, 256, B) + 4 * (2 * B * H + 2 * B), B
        assert q(9, 256, B) == q(6, 256, B)


def test_datd3_kernels_are_in_the_code_object(learner_kernels):
    new = ("datd3_actor_head_kernel", "datd3_critic_head_kernel")
    assert set(new + ("gemm_kernel", "actor_back_kernel", "adam_kernel")) <= set(learner_kernels), sorted(learner_kernels)
    for name in new:
        md, ins = learner_kernels[name]
        assert md["scratch"] == 0 and md["spill_vgpr"] == 0 and ins, (name, md)
        assert not [i.mnem for i in ins if "atomic" in i.mnem], name
        assert not [i.mnem for i in ins if "mfma" in i.mnem], name      # per-row heads: every contraction stays in gemm_kernel


def test_learner_choices_for_datd3_and_darc():
    """learner="fused" is FusedDATD3 / FusedDARC, "torch" the torch learners; "hip" stays the TD3 update and refuses them."""
    from armenv import train
    for algo in ("datd3", "darc"):
        train._check_learner(algo, "fused")
        train._check_learner(algo, "torch")
        with pytest.raises(ValueError):
            train._check_learner(algo, "hip")
        with pytest.raises(ValueError):
            train._check_learner(algo, "triton")
    with pytest.raises(ValueError):
        train._check_learner("ddpg", "torch")
    agent, static, graphs = train._make_agent("darc", "torch", 9, 0.4, "cpu", 64, False, 0)
    assert type(agent).__name__ == "DARC" and static is None and not graphs and agent.actor1.fc1.in_features == 9


def test_fused_datd3_refuses_unsupported_shapes():
    from armenv.fused_datd3 import FusedDARC, FusedDATD3
    for cls in (FusedDATD3, FusedDARC):
        for kw in (dict(state_dim=13, action_dim=3), dict(state_dim=6, action_dim=2), dict(state_dim=6, action_dim=3, hidden_dim=128)):
            with pytest.raises(ValueError):
                cls(action_bound=0.7, device="cpu", **kw)
    f = FusedDARC(6, 3, 0.7, device="cpu", seed=3)
    assert f._darc == 1 and f.q_weight == 0.2 and f.regularization_weight == 0.005 and len(f._nets()) == 8 and f.total_it == 0
