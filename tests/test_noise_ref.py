"""CPU checks of the exploration-noise reference (tests/noise_ref.py) and its case table (tests/noise_cases.py): the committed
fixture is valid, the float64 reference has true zeros where the function has them, the f32 emulation of the kernel sits inside the
derived bound on every case, every planted defect leaves the bound on a named case, and the reference stream -- which is the
distribution the kernel must have -- is N(0, 1), independent across components, steps, envs and episodes."""
import math

import numpy as np
import pytest

import noise_cases as NC
import noise_ref as NR


def _edge():
    k = NC.edge_keys()
    w = NC.edge_words(k)
    return k, w


def _all_cases():
    """[(name, seed, ids, episode index, step)]: the planted tuples as one case, each random block as one"""
    k = NC.edge_keys()
    out = [("edge-keys", k["seed"], np.uint64(k["offset"]) + k["env"].astype(np.uint64), k["episode"], k["step"])]
    for b in NC.BLOCKS:
        ids, ep, sp = NC.block_keys(b)
        out.append((b["id"], b["seed"], ids.reshape(-1), ep.reshape(-1), sp.reshape(-1)))
    return out


def test_fixture_is_valid_and_every_class_is_present():
    k, w = _edge()
    assert (k["seed"], k["offset"]) == (NC.EDGE_SEED, NC.EDGE_OFFSET) and k["names"] == NC.CLASSES
    assert k["seed"] >= 2 ** 32 and k["offset"] < 2 ** 32 <= k["offset"] + NC.EDGE_ENVS - 1
    assert np.all((0 <= k["env"]) & (k["env"] < NC.EDGE_ENVS)) and np.all((0 <= k["step"]) & (k["step"] < NC.EDGE_STEPS))
    assert np.all((0 <= k["episode"]) & (k["episode"] < 2 ** 31 - 1))        # planted as the i32 counter index + 1
    member = NC.classify(w)
    assert member[np.arange(len(w)), k["cls"]].all()                          # recomputed: a stale fixture cannot pass
    per_class = np.bincount(k["cls"], minlength=len(NC.CLASSES))
    assert np.all(per_class >= NC.MIN_PER_CLASS), dict(zip(NC.CLASSES, per_class))
    launches = NC.edge_launches(k)
    rows = np.concatenate([r[r >= 0] for _, _, r in launches])
    assert len(set(rows)) == len(rows) and len(launches) <= 16


def test_edge_uniforms_are_what_the_classes_say():
    k, w = _edge()
    u = NR.uniforms(w)
    for j, c in enumerate(k["cls"]):
        pair, kind = NC.CLASSES[c].split(":")
        ur, ua = (u[j, 0], u[j, 1]) if pair == "a" else (u[j, 2], u[j, 3])
        if kind == "rad-one":
            assert ur == 1.0
        elif kind == "rad-below-one":
            assert ur == np.float32(1.0 - 2.0 ** -24)
        elif kind == "rad-tail":
            assert ur <= 2.0 ** -24
        elif kind == "ang-one":
            assert ua == 1.0
        elif kind == "ang-zero":
            assert ua < 2.0 ** -24
        else:
            q = int(kind.rsplit("-", 1)[1]) / (4.0 if "sign" in kind else 8.0)
            assert abs(float(ua) - q) <= 2.0 ** -24


def test_reference_has_true_zeros():
    """u0 = 1: z0 = z1 = 0; u = k / 4: the sine (k even) or the cosine (k odd) is 0; and the bound there is 0, i.e. demands them"""
    top, mid = 0xFFFFFFFF, 0x12345678
    w = np.array([[top, mid, top, mid]] + [[mid, q << 30, mid, q << 30] for q in range(4)] + [[mid, top, mid, top]], dtype=np.uint64)
    z, b = NR.reference(w), NR.bound(w)
    assert np.all(z[0] == 0) and np.all(b[0] == 0)
    assert np.all(z[[1, 3, 5], 1] == 0) and np.all(b[[1, 3, 5], 1] == 0)         # sin at u = 0, 1/2 and 1
    assert np.all(z[[2, 4]][:, [0, 2]] == 0) and np.all(b[[2, 4]][:, [0, 2]] == 0)   # cos at u = 1/4, 3/4
    u = NR.uniforms(w)[1, 0]
    r = math.sqrt(-2.0 * math.log(float(u)))
    assert abs(z[1, 0] - r) < 1e-15 * r and abs(z[3, 0] + r) < 1e-15 * r and abs(z[2, 1] - r) < 1e-15 * r and abs(z[4, 1] + r) < 1e-15 * r
    assert abs(z[5, 0] - r) < 1e-15 * r                                            # u = 1.0 is the angle 0 again
    # next to u0 = 1: -2 ln(1 - 2^-24) = 2^-23 (1 + 2^-25 + ...)
    z1 = NR.reference(np.array([[0xFFFFFF00, 0, 0xFFFFFF00, 0]], dtype=np.uint64))
    assert abs(z1[0, 0] - math.sqrt(2.0 ** -23 * (1 + 2.0 ** -25))) < 1e-18


def test_bound_is_of_the_stated_size():
    """between 6.5 and 8.2 times 2^-24 relative on every draw (the module docstring's figures): a bound that grew or shrank by
    mistake shows here"""
    ids, ep, sp = NC.block_keys(NC.block("seed21-offset5"))
    w = NR.words(21, ids, ep, sp)
    z, b = NR.reference(w), NR.bound(w)
    rel = b / np.abs(z) * 2.0 ** 24
    assert 6.5 <= rel.min() < 6.6 and 8.1 < rel.max() <= 8.2, (rel.min(), rel.max())


@pytest.mark.parametrize("name", ["edge-keys"] + [b["id"] for b in NC.BLOCKS])
def test_emulation_is_within_the_bound(name):
    _, seed, ids, ep, sp = next(c for c in _all_cases() if c[0] == name)
    w = NR.words(seed, ids, ep, sp)
    got, ref, bnd = NR.emulate(w), NR.reference(w), NR.bound(w)
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    r = NR.ratio(got, ref, bnd)
    print("%s: emulation err / bound %.3f" % (name, r))
    assert r <= 1.0, r
    if name == "edge-keys":
        k = NC.edge_keys()
        for j, c in enumerate(k["cls"]):
            if NC.CLASSES[c] == "a:rad-one":
                assert got[j, 0] == 0 and got[j, 1] == 0
            if NC.CLASSES[c] == "b:rad-one":
                assert got[j, 2] == 0


@pytest.mark.parametrize("defect", NR.DEFECTS)
def test_every_planted_defect_leaves_the_bound(defect):
    """the case table is sensitive: each defect of noise_ref.DEFECTS puts the emulation outside the bound on at least one case;
    the arithmetic ones on the planted class that exists for them"""
    caught = {}
    for name, seed, ids, ep, sp in _all_cases():
        w = NR.words(seed, ids, ep, sp)
        got = NR.emulate_keys(seed, ids, ep, sp, defect)
        ref, bnd = NR.reference(w), NR.bound(w)
        with np.errstate(invalid="ignore", divide="ignore"):
            bad = ~(np.abs(got.astype(np.float64) - ref) <= bnd)             # NaN counts as outside
        if bad.any():
            caught[name] = int(bad.any(1).sum())
            if name == "edge-keys":
                k = NC.edge_keys()
                caught["edge-classes"] = sorted({NC.CLASSES[c] for c in k["cls"][bad.any(1)]})
    print("%s: caught on %s" % (defect, caught))
    assert caught, defect
    where = dict([("radius-plus-one-dropped", "rad-tail"), ("k4-sign", "ang-one"), ("sine-coefficient", "ang-tie")])
    if defect in where:
        assert any(where[defect] in c for c in caught.get("edge-classes", [])), (defect, caught)
    expect = {"id-high-dropped": "ids-across-2^32", "seed-high-dropped": "seed-high-word", "episode-not-minus-one": "counter-wraps",
              "step-bit-dropped": "seed21-offset5"}
    if defect in expect:
        assert expect[defect] in caught, (defect, caught)
    if defect == "id-high-dropped":
        assert "seed21-offset5" not in caught              # ids below 2^32 cannot see it: the boundary block is what does


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean()))


def test_reference_stream_is_standard_normal_and_independent():
    """4096 envs x 128 steps at one keying past every key boundary.  Every statistic within 5 standard errors of its N(0, 1) value:
    a condition on deterministic inputs (the largest here is 3.3), not a measurement.  The standard errors are those of N independent
    N(0, 1) draws: mean 1 / sqrt N, variance sqrt(2 / N), fourth moment sqrt(96 / N) (E z^8 - 9 = 96), P(|z| > 3) = p:
    sqrt(p (1 - p) / N), a correlation 1 / sqrt N."""
    S = NC.STREAM
    n, T = S["envs"], S["steps"]
    ids = np.uint64(S["offset"]) + np.arange(n, dtype=np.uint64)
    def stream(ep):
        return NR.reference(NR.words(S["seed"], np.repeat(ids, T), ep, np.tile(np.arange(T), n))).reshape(n, T, 3)
    z = stream(S["episode"])
    z_next = stream((S["episode"] + 1) & 0xFFFFFFFF)                # the episode after the wrap: index 0
    N = n * T
    p3 = math.erfc(3.0 / math.sqrt(2.0))
    stats = {}
    for c in range(3):
        v = z[..., c].reshape(-1)
        stats["mean z%d" % c] = v.mean() * math.sqrt(N)
        stats["var z%d" % c] = ((v * v).mean() - 1.0) / math.sqrt(2.0 / N)
        stats["m4 z%d" % c] = ((v ** 4).mean() - 3.0) / math.sqrt(96.0 / N)
        stats["tail z%d" % c] = ((np.abs(v) > 3.0).mean() - p3) / math.sqrt(p3 * (1 - p3) / N)
    f = z.reshape(-1, 3)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        stats["corr z%d z%d" % (a, b)] = _corr(f[:, a], f[:, b]) * math.sqrt(N)
    stats["corr z0^2 z1^2"] = _corr(f[:, 0] ** 2, f[:, 1] ** 2) * math.sqrt(N)           # they share a radius
    stats["lag-1 steps"] = _corr(z[:, :-1].reshape(-1), z[:, 1:].reshape(-1)) * math.sqrt(3 * n * (T - 1))
    stats["lag-1 envs"] = _corr(z[:-1].reshape(-1), z[1:].reshape(-1)) * math.sqrt(3 * (n - 1) * T)
    stats["lag-1 episodes"] = _corr(z.reshape(-1), z_next.reshape(-1)) * math.sqrt(3 * N)
    worst = max(stats, key=lambda k: abs(stats[k]))
    print("largest: %s at %.2f standard errors of %d statistics" % (worst, stats[worst], len(stats)))
    assert abs(stats[worst]) <= 5.0, {k: round(v, 2) for k, v in stats.items()}
    assert np.abs(z).max() < 6.67                                   # sqrt(-2 ln 2^-32) = 6.66
