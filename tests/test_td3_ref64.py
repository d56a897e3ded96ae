"""CPU tests of tests/learner_ref64.py for TD3, the float64 restatement of one update that the fused HIP update is tested against:
it reproduces the reference's own golden updates, equals torch autograd in float64, every defect switch breaks that equality, and
every TD3 case of tests/test_gpu_td3_ref64.py (tests/learner_cases.py) keeps its share of ambiguous relu units under the cap (the
bodies shared with tests/test_da_ref64.py are tests/learner_ref64_checks.py's).  Also: the host restatement of the kernel's
target-policy noise."""
import numpy as np
import pytest
import torch

from conftest import golden_npz
import learner_cases as K
import learner_ref64 as R
pytest.register_assert_rewrite("learner_ref64_checks")          # the shared bodies assert there
import learner_ref64_checks as X  # noqa: E402

KEYS = ("states", "actions", "next_states", "rewards", "dones")


def test_reference_reproduces_the_golden_updates():
    """The six TD3_MLP.train updates of tests/golden/td3_train_seed0.npz (B = 64, two with the actor step), from
    torch.manual_seed(0)'s initial weights and with the golden run's noise (torch.manual_seed(123), one randn(64, 3) per update):
    the tolerances of test_td3_learner_matches_reference_golden."""
    from armenv.td3 import TD3
    g = golden_npz("td3_train_seed0.npz")
    torch.manual_seed(0)
    st = X.zeros("td3", TD3(6, 3, 0.7, device="cpu"))
    torch.manual_seed(123)
    for i, want in enumerate(g["losses"]):
        b = {k: torch.from_numpy(g[f"b{i}_{k}"]).to(torch.float64) for k in KEYS}
        noise = torch.randn(64, 3).to(torch.float64)
        out = R.update("td3", st, b, noise, X.HP_GOLDEN, with_actor=(i + 1) % 3 == 0)
        assert abs(out["loss"] - want) < 1e-5 * max(1.0, abs(want)), (i, out["loss"], want)
        st = R.advance(st, out)
    assert st["critic_step"] == 6 and st["actor_step"] == 2
    X.assert_golden_nets("td3", st, g)


@pytest.mark.parametrize("with_actor", [False, True])
@pytest.mark.parametrize("B,D,seed", [(65, 6, 0), (300, 9, 1), (7, 1, 2), (257, 12, 3)])
def test_reference_equals_autograd_in_float64(B, D, seed, with_actor):
    """armenv.td3.TD3's update in float64, with and without the actor step; the reference evaluates B * 256 * (10 + 4) relu units"""
    X.check_reference_equals_autograd("td3", B, D, None, seed, with_actor)


@pytest.mark.parametrize("defect", R.DEFECTS["td3"])
def test_every_defect_switch_breaks_the_autograd_comparison(defect):
    X.check_defect_switch("td3", defect)


@pytest.mark.parametrize("c", [c for c in K.ALL_CASES if c["agent"] == "td3"], ids=K.case_id)
def test_gpu_case_inputs_keep_ambiguity_rare(c):
    X.check_case_inputs(c)


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
