"""CPU tests of the DATD3 / DARC learners: the torch learners (armenv.datd3) against the reference's recorded runs G17 / G18, which
tensors an update may touch, DARC's target arithmetic; and the fused update's host side (armenv_datd3_update, include/armenv.h): the
ctypes struct agrees with the header, every argument is validated before any HIP call, the workspace query, the new kernels in the
built code object, and the training loop's learner choices."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from datd3_golden import NETS, batch, expected_losses, load_train_fixture

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import isa  # noqa: E402

HEADER_DIR = os.path.join(ROOT, "include")
MOMENTS = tuple(n + mv for n in NETS[:4] for mv in ("_m", "_v"))
ALL_NETS = NETS + MOMENTS


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


def test_datd3_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = _ctypes_layout(L.ArmEnvDatd3Args)
    assert {m.split(".")[0] for m, _ in members} >= set(ALL_NETS) | {
        "update_actor", "darc", "q_weight", "regularization_weight", "policy_noise", "noise_clip", "seed", "draw", "noise_dev",
        "critic_step", "actor_step", "loss_dev"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "armenv.h"', "int main(void) {",
             '  printf("%zu %d\\n", sizeof(ArmEnvDatd3Args), ARMENV_ABI_VERSION);']
    lines += ['  printf("%%zu\\n", offsetof(ArmEnvDatd3Args, %s));' % m for m, _ in members]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-I", HEADER_DIR, "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert int(out[0]) == C.sizeof(L.ArmEnvDatd3Args) and int(out[1]) == L.ABI_VERSION == 8
    assert [int(x) for x in out[2:]] == [o for _, o in members], members


def _args(B=64, D=6, darc=1):
    """Arguments that pass every check but the one a test breaks: fake (never dereferenced) 16-byte aligned device pointers.
    NOT to be passed unmodified -- a valid set would be enqueued."""
    from armenv import _lib as L
    a = L.ArmEnvDatd3Args()
    a.device, a.state_dim, a.action_dim, a.hidden_dim, a.batch = 0, D, 3, 256, B
    a.action_bound, a.gamma, a.tau, a.policy_noise, a.noise_clip = 0.7, 0.98, 0.005, 0.2, 0.5
    a.actor_lr, a.critic_lr, a.beta1, a.beta2, a.eps = 1e-3, 1e-3, 0.9, 0.999, 1e-8
    a.q_weight, a.regularization_weight, a.darc = 0.2, 0.005, darc
    a.critic_step, a.actor_step, a.update_actor = 1, 1, 2
    addr = [0x10000]

    def ptr():
        addr[0] += 0x1000
        return addr[0]
    for net in ALL_NETS:
        m = getattr(a, net)
        for k in ("W1", "b1", "W2", "b2", "W3", "b3"):
            setattr(m, k, ptr())
    for k in ("states_dev", "actions_dev", "next_states_dev", "rewards_dev", "dones_dev", "workspace_dev"):
        setattr(a, k, ptr())
    a.workspace_bytes = L.load().armenv_datd3_workspace_bytes(D, 256, B)
    assert a.workspace_bytes > 0
    return a


def _breaks(mutate):
    from armenv import _lib as L
    lib = L.load()
    a = _args()
    mutate(a)
    rc = lib.armenv_datd3_update(C.byref(a), None)
    return rc, lib.armenv_last_error().decode()


def _null(net, key):
    return lambda a: setattr(getattr(a, net), key, None)


@pytest.mark.parametrize("field,mutate", [
    ("batch", lambda a: setattr(a, "batch", 0)),
    ("batch", lambda a: setattr(a, "batch", (1 << 20) + 1)),
    ("hidden_dim", lambda a: setattr(a, "hidden_dim", 128)),
    ("state_dim", lambda a: setattr(a, "state_dim", 0)),
    ("state_dim", lambda a: setattr(a, "state_dim", 13)),
    ("action_dim", lambda a: setattr(a, "action_dim", 2)),
    ("update_actor", lambda a: setattr(a, "update_actor", 0)),
    ("update_actor", lambda a: setattr(a, "update_actor", 3)),
    ("darc", lambda a: setattr(a, "darc", 2)),
    ("darc", lambda a: setattr(a, "darc", -1)),
    ("critic_step", lambda a: setattr(a, "critic_step", 0)),
    ("actor_step", lambda a: setattr(a, "actor_step", 0)),
    ("action_bound", lambda a: setattr(a, "action_bound", 0.0)),
    ("gamma", lambda a: setattr(a, "gamma", float("nan"))),
    ("tau", lambda a: setattr(a, "tau", 1.5)),
    ("policy_noise", lambda a: setattr(a, "policy_noise", -0.1)),
    ("noise_clip", lambda a: setattr(a, "noise_clip", float("inf"))),
    ("actor_lr", lambda a: setattr(a, "actor_lr", -1e-3)),
    ("critic_lr", lambda a: setattr(a, "critic_lr", float("nan"))),
    ("beta1", lambda a: setattr(a, "beta1", 1.0)),
    ("beta2", lambda a: setattr(a, "beta2", -0.1)),
    ("eps", lambda a: setattr(a, "eps", 0.0)),
    ("q_weight", lambda a: setattr(a, "q_weight", 1.5)),
    ("q_weight", lambda a: setattr(a, "q_weight", -0.1)),
    ("regularization_weight", lambda a: setattr(a, "regularization_weight", -0.005)),
    ("regularization_weight", lambda a: setattr(a, "regularization_weight", float("nan"))),
] + [(net, _null(net, key)) for net, key in zip(ALL_NETS, ("W1", "b1", "W2", "b2", "W3", "b3") * 3)] + [
    ("target_critic2", lambda a: setattr(a.target_critic2, "b1", a.target_critic2.b1 + 4)),      # misaligned
    ("critic1_v", lambda a: setattr(a.critic1_v, "W1", a.critic1_v.W1 + 8)),                    # misaligned
    ("states_dev", lambda a: setattr(a, "states_dev", None)),
    ("actions_dev", lambda a: setattr(a, "actions_dev", None)),
    ("next_states_dev", lambda a: setattr(a, "next_states_dev", None)),
    ("rewards_dev", lambda a: setattr(a, "rewards_dev", None)),
    ("dones_dev", lambda a: setattr(a, "dones_dev", None)),
    ("workspace_dev", lambda a: setattr(a, "workspace_dev", None)),
    ("workspace_dev", lambda a: setattr(a, "workspace_dev", a.workspace_dev + 4)),
    ("workspace_bytes", lambda a: setattr(a, "workspace_bytes", a.workspace_bytes - 1)),
])
def test_datd3_bad_arguments_are_refused_before_any_device_call(field, mutate):
    rc, msg = _breaks(mutate)
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


@pytest.fixture(scope="module")
def learner_kernels():
    if not os.path.exists(isa.LIB):
        pytest.skip("libarmenv.so is not built")
    if not os.path.exists(os.path.join(isa.LLVM, "llvm-objdump")):
        pytest.skip("the ROCm LLVM tools (llvm-objdump, llvm-readelf) are not installed")
    rows = [r for r in isa.all_kernels() if "armenv::learner::" in r[1]]
    return {dm.split("armenv::learner::")[1].split("(")[0]: (md, ins) for _, dm, md, ins in rows}


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
