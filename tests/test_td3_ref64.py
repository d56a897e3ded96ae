"""CPU tests of tests/td3_ref64.py, the float64 restatement of one TD3 update that the fused HIP update is tested against: it
reproduces the reference's own golden updates, equals torch autograd in float64, and every defect switch breaks that equality.
Also: the host restatement of the kernel's target-policy noise, and the batch-size limits of the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_npz
import td3_ref64 as R

HP = dict(action_bound=0.7, gamma=0.98, tau=0.005, policy_noise=0.2, noise_clip=0.5, actor_lr=1e-3, critic_lr=1e-3, beta1=0.9,
          beta2=0.999, eps=1e-8)
KEYS = ("states", "actions", "next_states", "rewards", "dones")


def test_reference_reproduces_the_golden_updates():
    """The six TD3_MLP.train updates of tests/golden/td3_train_seed0.npz (B = 64, two with the actor step), from
    torch.manual_seed(0)'s initial weights and with the golden run's noise (torch.manual_seed(123), one randn(64, 3) per update):
    the tolerances of test_td3_learner_matches_reference_golden."""
    from armenv.td3 import TD3
    g = golden_npz("td3_train_seed0.npz")
    torch.manual_seed(0)
    t = TD3(6, 3, 0.7, device="cpu")
    st = R.state_from(t.actor, t.critic, t.target_actor, t.target_critic, [torch.zeros_like(p) for p in t.actor.parameters()],
                      [torch.zeros_like(p) for p in t.actor.parameters()], [torch.zeros_like(p) for p in t.critic.parameters()],
                      [torch.zeros_like(p) for p in t.critic.parameters()], 0, 0)
    torch.manual_seed(123)
    for i, want in enumerate(g["losses"]):
        b = {k: torch.from_numpy(g[f"b{i}_{k}"]).to(torch.float64) for k in KEYS}
        noise = torch.randn(64, 3).to(torch.float64)
        with_actor = (i + 1) % 3 == 0
        out = R.td3_update(st, b, noise, HP, with_actor)
        assert abs(out["loss"] - want) < 1e-5 * max(1.0, abs(want)), (i, out["loss"], want)
        st = R.advance(st, out, with_actor)
    assert st["critic_step"] == 6 and st["actor_step"] == 2
    for name, net in (("actor", t.actor), ("critic", t.critic), ("target_actor", t.target_actor), ("target_critic", t.target_critic)):
        for (k, _), v in zip(net.state_dict().items(), st[name]):
            ref = g[f"{name}__{k.replace('.', '_')}"]
            assert np.abs(v.numpy() - ref).max() < 1e-5, (name, k, np.abs(v.numpy() - ref).max())


def _torch_state(t):
    (am, av, a_step), (cm, cv, c_step) = R.adam_state(t.actor, t.actor_opt), R.adam_state(t.critic, t.critic_opt)
    return R.state_from(t.actor, t.critic, t.target_actor, t.target_critic, am, av, cm, cv, a_step, c_step)


def _autograd_case(B, D, with_actor, seed, monkeypatch, hp, target_actor_gain=1.0):
    """armenv.td3.TD3's networks and Adam in float64 (torch autograd), two priming updates, then one more with or without the actor
    step.  Returns (state before it, batch, noise, the torch learner after it, its critic loss).  target_actor_gain scales the
    target actor's last layer (pre-tanh outputs of order one, so that target actions reach the clamp)."""
    from armenv.td3 import TD3
    torch.manual_seed(seed)
    t = TD3(D, 3, hp["action_bound"], device="cpu", actor_lr=hp["actor_lr"], critic_lr=hp["critic_lr"], tau=hp["tau"],
            gamma=hp["gamma"], policy_noise=hp["policy_noise"], noise_clip=hp["noise_clip"], policy_freq=1)
    for n in t._nets():
        n.double()
    with torch.no_grad():
        t.target_actor.fc3.weight.mul_(target_actor_gain)
    gen = torch.Generator().manual_seed(seed + 1)

    def update(batch, noise, flag):
        monkeypatch.setattr(torch, "randn_like", lambda x: noise.clone())
        try:
            return t._update(batch["states"], batch["actions"], batch["rewards"].view(-1, 1), batch["next_states"],
                             batch["dones"].view(-1, 1), flag)
        finally:
            monkeypatch.undo()
    for _ in range(2):
        update(R.random_batch(gen, B, D), torch.randn(B, 3, generator=gen, dtype=torch.float64), True)
    st = _torch_state(t)
    batch, noise = R.random_batch(gen, B, D), torch.randn(B, 3, generator=gen, dtype=torch.float64)
    loss = float(update(batch, noise, with_actor))
    return st, batch, noise, t, loss


def _autograd_failures(out, t, loss, with_actor, tol=2.0 ** -18):
    """names of the quantities of `out` that differ from the float64 autograd learner `t` by more than tol 2^-24 (= 2^-42, a few
    hundred float64 roundings) times their magnitude, plus the allowance"""
    bad = []
    if abs(out["loss"] - loss) > tol * R.U * out["loss_mag"]:
        bad.append("loss")
    sides = [("critic", t.critic, t.target_critic)] + ([("actor", t.actor, t.target_actor)] if with_actor else [])
    for name, net, tnet in sides:
        for k, p in enumerate(net.parameters()):
            if R.bad_elements(p.grad.detach(), out[name + "_grad"][k], out[name + "_grad_mag"][k], out[name + "_grad_allow"][k], tol)[0]:
                bad.append(f"{name}_grad{k}")
            if R.bad_elements(p.detach(), out[name][k], out[name + "_mag"][k], 0 * p, tol)[0]:
                bad.append(f"{name}{k}")
        if with_actor:
            for k, p in enumerate(tnet.parameters()):
                if R.bad_elements(p.detach(), out["target_" + name][k], out["target_" + name + "_mag"][k], 0 * p, tol)[0]:
                    bad.append(f"target_{name}{k}")
    return bad


@pytest.mark.parametrize("with_actor", [False, True])
@pytest.mark.parametrize("B,D,seed", [(65, 6, 0), (300, 9, 1), (7, 1, 2), (257, 12, 3)])
def test_reference_equals_autograd_in_float64(B, D, seed, with_actor, monkeypatch):
    """Gradients, loss, Adam-stepped parameters and soft-updated targets equal those of armenv.td3.TD3's update run in float64 with
    torch autograd and torch.optim.Adam, from primed (non-zero) Adam moments, to 2^-42 of their magnitudes."""
    st, batch, noise, t, loss = _autograd_case(B, D, with_actor, seed, monkeypatch, HP)
    out = R.td3_update(st, batch, noise, HP, with_actor, chunk=64)           # several chunks
    assert _autograd_failures(out, t, loss, with_actor) == []
    assert out["ambiguous"] < 1e-3 * out["units"] and out["units"] == B * 256 * (10 + (4 if with_actor else 0))


# hyper-parameters under which every defect has something to change: the noise clip binds on many elements, and with target
# actions of order one (target_actor_gain) the action clamp binds on many others, with and without the clip
HP_DEFECT = dict(HP, action_bound=0.25, policy_noise=0.4, noise_clip=0.1)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_switch_breaks_the_autograd_comparison(defect, monkeypatch):
    st, batch, noise, t, loss = _autograd_case(300, 6, True, 4, monkeypatch, HP_DEFECT, target_actor_gain=30.0)
    assert _autograd_failures(R.td3_update(st, batch, noise, HP_DEFECT, True), t, loss, True) == []
    bad = _autograd_failures(R.td3_update(st, batch, noise, HP_DEFECT, True, defect=defect), t, loss, True)
    assert bad, defect


# ---- the host restatement of the kernel's noise ----

def test_vectorised_philox_matches_the_oracle(O):
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, (64, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (64, 2), dtype=np.uint64)
    ctr[:3] = [[0, 0, 0, 0], [0xffffffff] * 4, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]]
    key[:3] = [[0, 0], [0xffffffff] * 2, [0xa4093822, 0x299f31d0]]
    got = R.philox4x32_10(ctr, key)
    assert got[:3].tolist() == [[0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd],
                                [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]]          # Random123 kat_vectors
    for c, k, w in zip(ctr, key, got):
        assert O.philox([int(x) for x in c], [int(x) for x in k]) == [int(x) for x in w]


def test_kernel_noise_is_the_box_muller_of_the_philox_words(O):
    """z of a few rows against a scalar restatement on the oracle's Philox, seeds and draws above 2^32 included"""
    import math
    for seed, draw in ((0, 1), (2 ** 32 + 5, 2 ** 32 + 1), (0xDEADBEEFCAFE, 7)):
        rows = [0, 1, 255, 2 ** 20 - 1, 2 ** 32 + 3]
        z = R.kernel_noise(seed, draw, rows)
        for b, zr in zip(rows, z):
            w = O.philox([b & 0xffffffff, b >> 32, draw & 0xffffffff, draw >> 32], [seed & 0xffffffff, seed >> 32])
            want = []
            for w0, w1 in ((w[0], w[1]), (w[2], w[3])):
                u1, u2 = ((w0 >> 8) + 1) / 2.0 ** 24, (w1 >> 8) / 2.0 ** 24
                r = math.sqrt(-2 * math.log(u1))
                want += [r * math.cos(2 * math.pi * u2), r * math.sin(2 * math.pi * u2)]
            assert np.array_equal(zr, np.array(want[:3])), (seed, draw, b)


def test_kernel_noise_is_standard_normal():
    """3.6e5 draws (120 000 rows x 3): mean, variance and the Kolmogorov-Smirnov statistic fit N(0, 1) (KS critical value at
    p = 0.001: 1.95 / sqrt(n))"""
    z = R.kernel_noise(12345, 17, np.arange(120000)).reshape(-1)
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / n), z.var()
    zs = torch.from_numpy(np.sort(z))
    cdf = (0.5 * (1 + torch.erf(zs / np.sqrt(2)))).numpy()
    i = np.arange(1, n + 1)
    ks = max((i / n - cdf).max(), (cdf - (i - 1) / n).max())
    assert ks < 1.95 / np.sqrt(n), ks
    # the three columns are each N(0, 1) too (z2 comes from the other pair of words)
    for j in range(3):
        c = z.reshape(-1, 3)[:, j]
        assert abs(c.mean()) < 5 / np.sqrt(c.size) and abs(c.var() - 1) < 5 * np.sqrt(2 / c.size), (j, c.mean(), c.var())


def test_kernel_noise_streams_differ():
    """Rows, draws and seeds, their words above 2^32 included, each select another stream."""
    base = R.kernel_noise(5, 3, [7, 2 ** 32 + 7])
    assert not np.array_equal(base[0], base[1])                       # row's high word
    for seed, draw in ((5 + 2 ** 32, 3), (5, 3 + 2 ** 32), (6, 3), (5, 4)):
        other = R.kernel_noise(seed, draw, [7, 2 ** 32 + 7])
        assert not np.any(other == base), (seed, draw)
    z = R.kernel_noise(0, 1, np.arange(1000))
    assert len(np.unique(z)) == z.size


# ---- batch-size limits of the C ABI ----

def test_workspace_query_at_the_batch_limit():
    from armenv import _lib as L
    lib = L.load()
    for D in (1, 6, 12):
        assert lib.armenv_td3_workspace_bytes(D, 256, 2 ** 20) > 0
        assert lib.armenv_td3_workspace_bytes(D, 256, 2 ** 20 + 1) == -1


def test_update_refuses_a_batch_above_the_limit():
    from armenv import _lib as L
    from learner_host import fake_args
    lib, a = L.load(), fake_args("td3")
    a.batch = 2 ** 20 + 1
    rc, msg = lib.armenv_td3_update(C.byref(a), None), lib.armenv_last_error().decode()
    assert rc == -1 and "batch" in msg and "armenv_td3_update" in msg, (rc, msg)
