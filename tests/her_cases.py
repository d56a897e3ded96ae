"""The case table of the trajectory store's tests: rings for the episode index (index_episodes_kernel) and rings with picks for the
HER-"future" sampler (her_sample_kernel, her_sample_one), built on the CPU from one seed, with the conditions each block is named
after asserted when the table is built (build()) and again on a loaded one (check()).

A STORE is a dict: name, block, the geometry (cap, base, T, N, D, at_reset), the PHYSICAL arrays as the ring holds them (obs0 [N][D];
obs_after, next_obs [cap][N][D]; action [cap][N][3]; reward [cap][N]; done u8 [cap][N]: logical step t lives in row (base + t) % cap),
picks i32 [B][4] = (episode, step_state, use_her, step_goal), family (one name per pick), thr (dis_threshold, a Python float).
Expected values are oracle.her on the LINEAR window (linear(), expected()): the restatement of the reference's sampler, which
tests/golden/her_edges_*.npz (G17 of gen_fixtures.py) holds against the reference itself on the threshold block and the linear
addressing stores.

Blocks
  index       T = 5 with all 32 done patterns as env columns (column n: pattern n % 32, bit t = done of step t), N in {32, 257},
              cap in {5, 8}, every base, both starts_at_reset; T = 1 with cap = 1.  Rows outside the window hold done = 1.
  addressing  cap 7, N 3, T in {7, 5}, every base, both at_reset, D in {6, 9}.  Column 0: done on every step (episodes of length 1);
              column 1: episodes of 1, 3 and 2 steps, then an unfinished one (T = 5 cuts the 2-step one short: unfinished); column 2:
              done on the window's last step only (one full-length episode from obs0 with at_reset, none without: a zero count
              between non-zero ones).  Every element names its origin: ((array * 8 + physical row) * 4 + env) * 16 + component + 1,
              times 2^-10 (the other blocks' rings hold such values too, with 512 for 4 where N > 4).  Rows outside the window hold such values too.  Column 1's rewards are -0.0, a denormal, +-inf and a NaN.
              Picks: ALL of them -- (ep, st) without HER, (ep, st, sg) for st + 1 <= sg <= L with.  Goals and next states are next_obs
              rows of one column: their distance is 64 sqrt(3) 2^-10 = 0.108 per physical row apart, so dis_threshold = 0.15 puts
              neighbours (and sg = st + 1: the goal IS the next state, dis = 0) near and everything else far.
  threshold   cap 4, base 3, T 3; column n: a 2-step episode whose next_obs[:3] of step 0 and of step 1 (the goal of the pick
              (st 0, sg 2)) are planted, then a 1-step episode.  One store per (D, threshold in 0.1, 0.25, 0.7); families below.
  draw        rings of E in {1, 3, 37} complete episodes; (B, seed, draw, her_ratio, use_her) combinations with the picks the
              kernel must draw computed here (philox_uniforms, picks_from_uniforms), kept in the store's `draws` list.

Threshold families (>= 8 planted cases each, over the three thresholds): D = 6, on the reference's f32 dis: eq (== float32(thr)), pred,
succ, each with axis-aligned and three-component differences; D = 9, on the f64 dis: between (strictly between thr and
(double)(float)thr; thr 0.1 and 0.7), exact (dis == 0.25) and above (one component one f32 step further); both: order (summing
d0^2 + (d1^2 + d2^2) lands on the other side), fma (fma(d2, d2, d0^2 + d1^2) lands on the other side); D = 9: f32 (f32 arithmetic
lands on the other side).  How the D = 9 cases reach single ulps of the f64 distance although the stored values are f32: the goal's
third component is tiny, so next - goal there carries far more than 24 bits.
"""
from fractions import Fraction

import numpy as np

from oracle import her

SEED = 20261021
RINGS = ("obs_after", "next_obs", "action", "reward", "done")
BATCH = ("states", "actions", "next_states", "rewards", "dones")
THRESHOLDS = (0.1, 0.25, 0.7)
ADDR_THR = 0.15
PER_FAMILY = 4                      # planted cases per (family, threshold, outcome or shape)
ARRAY_ID = dict(obs0=0, obs_after=1, next_obs=2, action=3, reward=4)
SPECIAL_REWARDS = np.array([0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC00000], np.uint32).view(np.float32)
FAMILIES6 = ("eq", "pred", "succ", "order", "fma")
FAMILIES9 = ("between", "exact", "above", "order", "fma", "f32")
DEFECTS = ("thr_f32", "ge", "f32_at_9", "sum_order", "fused", "obs_after_for_next", "obs0_ignored", "no_ring", "row_off_by_one",
           "sg_upper", "keep_6_9", "goal_state_only")
KEY_XOR = 0x5DEECE66D1CE4E5B
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------- the distance, in every form

def _round(x, dt):
    """the Fraction x rounded once, to nearest even, to dt"""
    f = dt(float(x))                                     # float(Fraction) rounds correctly to f64
    if dt is np.float64:
        return f
    around = [np.nextafter(f, dt(-np.inf)), f, np.nextafter(f, dt(np.inf))]
    return min(around, key=lambda c: (abs(Fraction(float(c)) - x), int(c.view(np.uint32)) & 1))


def distance(nv, g, D, form="ref", f32_at_9=False):
    """dis of her_sample_one from next_state[:3] and goal (f32 values): f32 arithmetic for D = 6, f64 for D = 9.  form: ref =
    (d0^2 + d1^2) + d2^2, order = d0^2 + (d1^2 + d2^2), fused = fma(d2, d2, d0^2 + d1^2).  A Python float."""
    dt = np.float32 if (D == 6 or f32_at_9) else np.float64
    d0, d1, d2 = (dt(nv[k]) - dt(g[k]) for k in range(3))
    if form == "ref":
        s = (d0 * d0 + d1 * d1) + d2 * d2
    elif form == "order":
        s = d0 * d0 + (d1 * d1 + d2 * d2)
    else:
        s = _round(Fraction(float(d2)) ** 2 + Fraction(float(d0 * d0 + d1 * d1)), dt)
    return float(np.sqrt(dt(s)))


def _distance_many(p, g, D, form="ref", f32_at_9=False):
    """distance() over arrays [M][3], forms ref and order"""
    dt = np.float32 if (D == 6 or f32_at_9) else np.float64
    d = p.astype(dt) - g.astype(dt)
    q = d * d
    s = (q[:, 0] + q[:, 1]) + q[:, 2] if form == "ref" else q[:, 0] + (q[:, 1] + q[:, 2])
    return np.sqrt(s).astype(np.float64)


# ---------------------------------------------------------------------------------------------- stores

def linear(S):
    """the window of a store in logical time, as oracle.her reads a chunk"""
    rows = (S["base"] + np.arange(S["T"])) % S["cap"]
    ch = {k: S[k][rows] for k in RINGS}
    ch["obs0"] = S["obs0"]
    return ch


def episodes_of(S):
    return her.index_episodes(linear(S)["done"], starts_at_reset=bool(S["at_reset"]))


def expected(S, picks=None):
    """oracle.her on the linear window: the batch the sampler owes for the store's picks"""
    return her.sample_with_picks(linear(S), episodes_of(S), S["picks"] if picks is None else picks, S["thr"])


def bits(a):
    """an array as integers: floats by their bit patterns"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _named(array, cap, N, comps):
    r, n, c = np.meshgrid(np.arange(cap), np.arange(N), np.arange(comps), indexing="ij")
    return ((((ARRAY_ID[array] * 8 + r) * (4 if N <= 4 else 512) + n) * 16 + c + 1) * 2.0 ** -10).astype(np.float32)


def _named_ring(cap, N, D):
    """the six arrays of a ring of cap rows, every element naming (array, physical row, env, component); done = 1 everywhere"""
    S = dict(obs0=_named("obs0", 1, N, D)[0], obs_after=_named("obs_after", cap, N, D), next_obs=_named("next_obs", cap, N, D),
             action=_named("action", cap, N, 3), reward=_named("reward", cap, N, 1)[..., 0], done=np.ones((cap, N), np.uint8))
    flat = np.concatenate([S[k].ravel() for k in ("obs0", "obs_after", "next_obs", "action", "reward")])
    assert len(np.unique(flat)) == flat.size
    return S


def _set_done(S, logical_done):
    """writes the window's done [T][N] into its physical rows"""
    rows = (S["base"] + np.arange(S["T"])) % S["cap"]
    S["done"][rows] = logical_done


def all_picks(episodes):
    """every pick a list of episodes admits"""
    out = []
    for ep, (_, _, L) in enumerate(episodes):
        for st in range(L):
            out.append((ep, st, 0, st + 1))
            out.extend((ep, st, 1, sg) for sg in range(st + 1, L + 1))
    return np.array(out, np.int32).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------- index block

def index_cases():
    """(cap, T, N, base, at_reset) of the index block"""
    for cap in (5, 8):
        for N in (32, 257):
            for base in range(cap):
                for at_reset in (0, 1):
                    yield cap, 5, N, base, at_reset
    for at_reset in (0, 1):
        yield 1, 1, 2, 0, at_reset


def index_done(cap, T, N, base):
    """(physical done u8 [cap][N], the linear window [T][N]): column n holds pattern n % 32, bit t = done of logical step t"""
    n = np.arange(N)
    window = ((n[None, :] % 32) >> np.arange(T)[:, None] & 1).astype(np.uint8)
    phys = np.ones((cap, N), np.uint8)
    phys[(base + np.arange(T)) % cap] = window
    return phys, window


# ---------------------------------------------------------------------------------------------- addressing block

def _addressing_store(D, T, base, at_reset):
    cap, N = 7, 3
    S = dict(name=f"addr.D{D}.T{T}.b{base}.r{at_reset}", block="addressing", cap=cap, base=base, T=T, N=N, D=D, at_reset=at_reset,
             thr=ADDR_THR, **_named_ring(cap, N, D))
    done = np.zeros((T, N), np.uint8)
    done[:, 0] = 1
    done[[0, 3] + ([5] if T == 7 else []), 1] = 1
    done[T - 1, 2] = 1
    _set_done(S, done)
    rows = (base + np.arange(5)) % cap
    S["reward"][rows, 1] = SPECIAL_REWARDS
    S["picks"] = all_picks(episodes_of(S))
    S["family"] = np.array(["all"] * len(S["picks"]))
    return S


def addressing_block():
    return [_addressing_store(D, T, base, r) for D in (6, 9) for T in (7, 5) for base in range(7) for r in (0, 1)]


def rolled(S, shift):
    """an addressing store with its env columns rotated by `shift` (column n becomes column n - shift): the same geometry and the same
    episodes under other env numbers, hence another index, other picks and other values -- what the members of a population hold"""
    R = dict(S, name=f"{S['name']}.c{shift}", obs0=np.roll(S["obs0"], -shift, axis=0), **{k: np.roll(S[k], -shift, axis=1) for k in RINGS})
    R["picks"] = all_picks(episodes_of(R))
    R["family"] = np.array(["all"] * len(R["picks"]))
    assert len(R["picks"]) == len(S["picks"])
    return R


def is_linear_addressing(S):
    return S["block"] == "addressing" and S["base"] == 0 and S["T"] == S["cap"] and S["at_reset"] == 1


# ---------------------------------------------------------------------------------------------- threshold block

def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _candidates(rng, M, thr, D, axis_aligned):
    """M (next[:3], goal) pairs of f32 values whose distance is within a few ulps of thr"""
    g = rng.uniform(0.2, 0.6, (M, 3))
    if axis_aligned:
        k = rng.integers(0, 3, M)
        sign = rng.choice([-1.0, 1.0], M)
        t32 = np.float64(np.float32(thr))
        step = rng.integers(-3, 4, M) * np.spacing(np.float32(thr)).astype(np.float64)
        g, p = _f32(g), _f32(g)
        p[np.arange(M), k] = _f32(p[np.arange(M), k].astype(np.float64) + sign * (t32 + step))
        return p, g
    v = rng.normal(size=(M, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = np.where(np.abs(v) < 0.2, np.sign(v) * 0.2 + (v == 0) * 0.2, v)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if D == 6:
        g = _f32(g)
        return _f32(g.astype(np.float64) + thr * v * (1.0 + rng.uniform(-3e-7, 3e-7, (M, 1)))), g
    # D = 9: two ordinary components; the third closes the f64 distance onto a target within a few f64 ulps of thr (or inside the
    # band between thr and its f32 rounding): next = f32(d2), goal = f32(next - d2) is tiny and non-zero, so next - goal has ~50 bits
    g = _f32(g)
    p = _f32(g.astype(np.float64) + thr * v)
    band = np.float64(np.float32(thr)) - thr
    target = thr + np.where(rng.random(M) < 0.5, rng.integers(-2, 3, M) * np.spacing(thr), band * rng.uniform(0.05, 0.95, M))
    d = p.astype(np.float64) - g.astype(np.float64)
    d2 = np.sqrt(target * target - d[:, 0] ** 2 - d[:, 1] ** 2) * rng.choice([-1.0, 1.0], M)
    p[:, 2] = _f32(d2)
    g[:, 2] = _f32(p[:, 2].astype(np.float64) - d2)
    return p, g


def _take(sel, count):
    return np.flatnonzero(sel)[:count].tolist()


def _planted(D, thr, rng):
    """[(family, next[:3], goal)] for one (D, threshold)"""
    out, n = [], PER_FAMILY
    far = lambda dis: dis > thr
    t32 = np.float32(thr)
    lo32, hi32 = np.nextafter(t32, np.float32(-1)), np.nextafter(t32, np.float32(2))
    pa, ga = _candidates(rng, 20000, thr, D, True)
    pc, gc = _candidates(rng, 400000, thr, D, False)
    pc, gc = pc[(gc != 0).all(axis=1)], gc[(gc != 0).all(axis=1)]
    da, dc = _distance_many(pa, ga, D), _distance_many(pc, gc, D)
    add = lambda fam, p, g, idx: out.extend((fam, p[i], g[i]) for i in idx)
    if D == 6:
        for fam, v in (("eq", t32), ("pred", lo32), ("succ", hi32)):
            add(fam, pa, ga, _take(da == np.float64(v), n))
            add(fam, pc, gc, _take(dc == np.float64(v), n))
    else:
        f32thr = np.float64(t32)
        if f32thr != thr:
            add("between", pc, gc, _take((dc > min(thr, f32thr)) & (dc < max(thr, f32thr)), 2 * n))
        else:
            m = 4 * n                                                   # goal = k 2^-24 in [0.25, 0.5): goal + 0.25 is an f32
            k = rng.integers(1 << 22, 1 << 23, m)
            g = _f32(rng.uniform(0.2, 0.6, (m, 3)))
            ax = np.arange(m) % 3
            g[np.arange(m), ax] = k * 2.0 ** -24
            p = g.copy()
            p[np.arange(m), ax] = g[np.arange(m), ax] + np.float32(thr)
            add("exact", p, g, range(2 * n))
            add("exact", pc, gc, _take(dc == thr, n))
            p2 = p.copy()
            p2[np.arange(m), ax] = np.nextafter(p2[np.arange(m), ax], np.float32(2))
            add("above", p2, g, range(2 * n, m))
        d32 = _distance_many(pc, gc, D, f32_at_9=True)
        for outcome in (False, True):
            add("f32", pc, gc, _take((far(dc) == outcome) & (far(d32) != outcome), n))
    do = _distance_many(pc, gc, D, "order")
    for outcome in (False, True):
        add("order", pc, gc, _take((far(dc) == outcome) & (far(do) != outcome), n))
    # the fused form is evaluated exactly, case by case, on the candidates within two ulps of the threshold
    ulp = np.spacing(np.float32(thr)).astype(np.float64) if D == 6 else np.spacing(thr)
    want = {False: n, True: n}
    for i in np.flatnonzero(np.abs(dc - thr) <= 2.5 * ulp)[:12000]:
        outcome = bool(far(dc[i]))
        if want[outcome] and far(distance(pc[i], gc[i], D, "fused")) != outcome:
            out.append(("fma", pc[i], gc[i]))
            want[outcome] -= 1
        if not (want[False] or want[True]):
            break
    return out


def _threshold_store(D, thr, rng):
    planted = _planted(D, thr, rng)
    N, cap, base, T = len(planted), 4, 3, 3
    assert 1 <= N <= 257
    S = dict(name=f"thr.D{D}.{thr}", block="threshold", cap=cap, base=base, T=T, N=N, D=D, at_reset=1, thr=thr, **_named_ring(cap, N, D))
    done = np.zeros((T, N), np.uint8)
    done[1:] = 1
    _set_done(S, done)
    r0, r1 = base % cap, (base + 1) % cap
    picks, family = [], []
    for n, (fam, p, g) in enumerate(planted):
        S["next_obs"][r0, n, :3], S["next_obs"][r1, n, :3] = p, g
        for pick in all_picks([(n, 0, 2), (n, 2, 1)]):
            picks.append((2 * n + pick[0],) + tuple(pick[1:]))
            family.append(fam if tuple(pick) == (0, 0, 1, 2) else "aux")
    S["picks"], S["family"] = np.array(picks, np.int32), np.array(family)
    return S


def threshold_block():
    rng = np.random.default_rng([SEED, 1])
    return [_threshold_store(D, thr, rng) for D in (6, 9) for thr in THRESHOLDS]


# ---------------------------------------------------------------------------------------------- draw block

def philox_uniforms(seed, draw, B):
    """u0..u3 f64 [4][B] of her_sample_one for rows 0..B-1: Philox4x32-10 (learner_ref64.philox4x32_10) with key seed ^ KEY_XOR and
    counters (b lo, b hi, the low 32 bits of draw, block 0 | 1); u53 of the word pairs (0, 1) and (2, 3) of each block"""
    from learner_ref64 import philox4x32_10
    k = (int(seed) ^ KEY_XOR) & M64
    b = np.arange(B, dtype=np.uint64)
    key = np.broadcast_to(np.array([k & M32, k >> 32], np.uint64), (B, 2))
    u = []
    for block in (0, 1):
        ctr = np.stack([b & np.uint64(M32), b >> np.uint64(32), np.full_like(b, int(draw) & M32), np.full_like(b, block)], -1)
        w = philox4x32_10(ctr, key)
        for hi, lo in ((0, 1), (2, 3)):
            v = ((w[:, hi] << np.uint64(32)) | w[:, lo]) >> np.uint64(11)
            u.append(v.astype(np.float64) * 2.0 ** -53)
    return np.stack(u)


def picks_from_uniforms(u, episodes, her_ratio, use_her, defect=None):
    E, lengths = len(episodes), episodes[:, 2].astype(np.int64)
    ep = (u[0] * np.float64(E)).astype(np.int32)
    L = lengths[ep]
    st = (u[1] * L.astype(np.float64)).astype(np.int32)
    h = (bool(use_her) & (u[2] <= her_ratio)).astype(np.int32)
    span = L - st - (1 if defect == "sg_upper" else 0)
    sg = st + 1 + (u[3] * span.astype(np.float64)).astype(np.int32)
    return np.stack([ep, st, h, sg], -1).astype(np.int32)


def _draw_store(name, cap, base, lengths_by_column, D):
    """a ring whose column n holds the complete episodes lengths_by_column[n] back to back, then an unfinished rest"""
    N = len(lengths_by_column)
    S = dict(name=name, block="draw", cap=cap, base=base, T=cap, N=N, D=D, at_reset=1, thr=ADDR_THR, **_named_ring(cap, N, D))
    done = np.zeros((cap, N), np.uint8)
    for n, ls in enumerate(lengths_by_column):
        done[np.cumsum(ls) - 1, n] = 1
    _set_done(S, done)
    S["picks"], S["family"] = np.zeros((0, 4), np.int32), np.array([], dtype="U1")
    return S


DRAW_SEEDS = (0, 5, 2 ** 32 + 5, 2 ** 64 - 1)
DRAW_DRAWS = (0, 1, 2 ** 32 - 1, 2 ** 32 + 1)


def draw_block():
    stores = [_draw_store("draw.E1", 1, 0, [[1]], 6),
              _draw_store("draw.E3", 4, 2, [[1, 3], [4]], 9),
              _draw_store("draw.E37", 8, 5, [[1] * 8, [1] * 8, [2] * 4, [2] * 4, [3, 5], [1, 2, 3], [1] * 8], 6)]
    for S, E in zip(stores, (1, 3, 37)):
        eps = episodes_of(S)
        assert len(eps) == E and (eps[:, 2] == 1).any()
        combos = [(257, s, d, 0.8, 1) for s in DRAW_SEEDS for d in DRAW_DRAWS]
        combos += [(B, 5, 1, 0.8, 1) for B in (1, 256)] + [(257, 5, 1, r, 1) for r in (0.0, 1.0)]
        combos += [(B, 2 ** 32 + 5, 2 ** 32 + 1, r, 0) for B, r in ((257, 0.8), (256, 1.0), (1, 0.0))]
        S["draws"] = [dict(B=B, seed=s, draw=d, her_ratio=r, use_her=h, members=1,
                           picks=picks_from_uniforms(philox_uniforms(s, d, B), eps, r, h)[None]) for B, s, d, r, h in combos]
        if E == 37:                                               # the population: member p draws with seed + p, wrapping
            s = 2 ** 64 - 1
            S["draws"].append(dict(B=257, seed=s, draw=1, her_ratio=0.8, use_her=1, members=3, picks=np.stack(
                [picks_from_uniforms(philox_uniforms((s + p) & M64, 1, 257), eps, 0.8, 1) for p in range(3)])))
    return stores


# ---------------------------------------------------------------------------------------------- the table

def build():
    T = dict(stores=addressing_block() + threshold_block() + draw_block())
    check(T, whole=True)
    return T


FIXTURE_KEYS = ("obs0",) + RINGS + ("picks", "family")
GEOMETRY = ("cap", "base", "T", "N", "D", "at_reset")


def fixture_stores(T, D):
    """the stores G17 runs the reference on: the threshold block and the linear addressing stores of one observation width"""
    return [S for S in T["stores"] if S["D"] == D and (S["block"] == "threshold" or is_linear_addressing(S))]


def fixture_arrays(S):
    """a store as flat npz entries under its name"""
    out = {f"{S['name']}/{k}": S[k] for k in FIXTURE_KEYS}
    out[f"{S['name']}/geometry"] = np.array([S[k] for k in GEOMETRY], np.int64)
    out[f"{S['name']}/thr"] = np.float64(S["thr"])
    return out


def load_fixture(npz):
    """the stores of a her_edges_*.npz, each with `ref`: the reference's outputs for its picks"""
    stores = []
    for name in [str(s) for s in npz["names"]]:
        S = dict(name=name, block="threshold" if name.startswith("thr.") else "addressing", thr=float(npz[f"{name}/thr"]))
        S.update({k: npz[f"{name}/{k}"] for k in FIXTURE_KEYS})
        S.update(zip(GEOMETRY, (int(v) for v in npz[f"{name}/geometry"])))
        S["ref"] = {k: npz[f"{name}/ref.{k}"] for k in BATCH}
        stores.append(S)
    return dict(stores=stores)


def check(T, whole=False):
    """The blocks' conditions, on a built table (whole = True: every block must be there) or on a loaded fixture."""
    stores = T["stores"]
    by_block = {b: [S for S in stores if S["block"] == b] for b in ("addressing", "threshold", "draw")}
    if whole:
        assert len(by_block["addressing"]) == 56 and len(by_block["threshold"]) == 6 and len(by_block["draw"]) == 3
        for cap, T_, N, base, at_reset in index_cases():
            phys, window = index_done(cap, T_, N, base)
            outside = np.setdiff1d(np.arange(cap), (base + np.arange(T_)) % cap)
            assert (phys[outside] == 1).all() and N >= min(32, 2 ** T_)
            assert np.array_equal(window[:, :2 ** T_ if N >= 32 else N].T @ (1 << np.arange(T_)), np.arange(min(N, 2 ** T_)))
    for S in stores:
        assert S["obs_after"].shape == (S["cap"], S["N"], S["D"]) and S["done"].shape == (S["cap"], S["N"]), S["name"]
        assert S["cap"] * S["N"] <= 8 * 257 and S["T"] <= S["cap"] and 0 <= S["base"] < S["cap"]
        eps = episodes_of(S)
        pk = S["picks"]
        if len(pk):
            L = eps[pk[:, 0], 2]
            assert (pk[:, 0] < len(eps)).all() and (0 <= pk[:, 1]).all() and (pk[:, 1] < L).all(), S["name"]
            assert (pk[:, 3] > pk[:, 1]).all() and (pk[:, 3] <= L).all(), S["name"]
    for S in by_block["addressing"]:
        eps, pk, name = episodes_of(S), S["picks"], S["name"]
        assert np.array_equal(pk, all_picks(eps))
        counts = np.bincount(eps[:, 0], minlength=3)
        assert counts[0] == S["T"] - (0 if S["at_reset"] else 1) and (eps[eps[:, 0] == 0, 2] == 1).all(), name
        want1 = [1, 3, 2] if S["T"] == 7 else [1, 3]
        assert eps[eps[:, 0] == 1, 2].tolist() == (want1 if S["at_reset"] else want1[1:]), name
        assert counts[2] == S["at_reset"] and (not S["at_reset"] or tuple(eps[-1]) == (2, 0, S["T"])), name
        rows = (S["base"] + np.arange(S["T"])) % S["cap"]
        assert set(bits(SPECIAL_REWARDS).tolist()) <= set(bits(S["reward"][rows, 1]).tolist()), name
        flat = np.concatenate([bits(S[k]).ravel() for k in ("obs0", "obs_after", "next_obs", "action", "reward")])
        assert len(np.unique(flat)) == flat.size, name                                       # distinct, in and outside the window
        her_pk = pk[pk[:, 2] == 1]
        assert (her_pk[:, 3] == her_pk[:, 1] + 1).any() and (her_pk[:, 3] == eps[her_pk[:, 0], 2]).any(), name
        out = expected(S, her_pk)
        assert set(out["dones"].tolist()) == {0, 1}, name                                    # both outcomes among the relabelled picks
    fams = {6: {}, 9: {}}
    for S in by_block["threshold"]:
        D, thr, eps = S["D"], S["thr"], episodes_of(S)
        assert thr in THRESHOLDS and np.array_equal(eps[:, 2], np.tile([2, 1], S["N"])), S["name"]
        lin = linear(S)
        f32thr = float(np.float32(thr))
        for pick, fam in zip(S["picks"], S["family"]):
            if fam == "aux":
                continue
            n = eps[pick[0], 0]
            assert tuple(pick[1:]) == (0, 1, 2)
            nv, g = lin["next_obs"][0, n, :3], lin["next_obs"][1, n, :3]
            assert (g != 0).all(), (S["name"], n)
            dis = distance(nv, g, D)
            far = dis > thr
            other = lambda **kw: distance(nv, g, D, **kw) > thr
            if fam in ("eq", "pred", "succ"):
                t32 = np.float32(thr)
                want = dict(eq=t32, pred=np.nextafter(t32, np.float32(-1)), succ=np.nextafter(t32, np.float32(2)))[fam]
                assert D == 6 and dis == float(want), (S["name"], n, fam)
            elif fam == "between":
                assert D == 9 and min(thr, f32thr) < dis < max(thr, f32thr), (S["name"], n)
            elif fam == "exact":
                assert D == 9 and dis == thr == 0.25, (S["name"], n)
            elif fam == "above":
                step = nv.copy()
                k = int(np.argmax(np.abs(nv - g)))
                step[k] = np.nextafter(step[k], np.float32(-1))
                assert D == 9 and thr == 0.25 and far and distance(step, g, D) == thr, (S["name"], n)
            elif fam == "order":
                assert other(form="order") != far, (S["name"], n)
            elif fam == "fma":
                assert other(form="fused") != far, (S["name"], n)
            elif fam == "f32":
                assert D == 9 and other(f32_at_9=True) != far, (S["name"], n)
            else:
                raise AssertionError(fam)
            shape = "axis" if (nv != g).sum() == 1 else "three" if (nv != g).all() else "two"
            fams[D].setdefault(fam, []).append((thr, bool(far), shape))
    if by_block["threshold"]:
        for D, names in ((6, FAMILIES6), (9, FAMILIES9)):
            if not any(S["D"] == D for S in by_block["threshold"]):
                continue
            for fam in names:
                cases = fams[D].get(fam, [])
                assert len(cases) >= 8, (D, fam, len(cases))
                outcomes = {c[1] for c in cases}
                # pred is near and succ far at every threshold, exact is near and above far by their definitions
                allows_both = fam not in ("pred", "succ", "exact", "above")
                assert outcomes == ({False, True} if allows_both else outcomes) and len(outcomes) >= 1, (D, fam, outcomes)
                if fam in ("eq", "pred", "succ"):
                    assert {c[2] for c in cases} == {"axis", "three"} and {c[0] for c in cases} == set(THRESHOLDS), (D, fam)
                if fam in ("order", "fma"):
                    assert {c[0] for c in cases} == set(THRESHOLDS), (D, fam)
    for S in by_block["draw"]:
        eps = episodes_of(S)
        seen = set()
        for d in S["draws"]:
            pk = d["picks"]
            assert pk.shape == (d["members"], d["B"], 4)
            L = eps[pk[..., 0], 2]
            assert (pk[..., 0] >= 0).all() and (pk[..., 0] < len(eps)).all() and (pk[..., 1] < L).all() and (pk[..., 3] <= L).all()
            assert (pk[..., 3] > pk[..., 1]).all()
            if not d["use_her"] or d["her_ratio"] == 0.0:
                assert (pk[..., 2] == 0).all()
            if d["use_her"] and d["her_ratio"] == 1.0:
                assert (pk[..., 2] == 1).all()
            seen.add((d["B"], d["seed"], d["draw"], d["her_ratio"], d["use_her"]))
        assert {s[0] for s in seen} == {1, 256, 257} and {s[1] for s in seen} >= set(DRAW_SEEDS) and {s[2] for s in seen} >= set(DRAW_DRAWS)
        assert {s[3] for s in seen} == {0.0, 0.8, 1.0} and {s[4] for s in seen} == {0, 1}
        # the low 32 bits of draw enter the counter: draws 1 and 2^32 + 1 give the same picks, 0 and 1 do not (E > 1)
        same = {(d["seed"], d["draw"]): d["picks"] for d in S["draws"] if d["B"] == 257 and d["her_ratio"] == 0.8 and d["use_her"] and d["members"] == 1}
        assert np.array_equal(same[(5, 1)], same[(5, 2 ** 32 + 1)])
        assert len(eps) == 1 or not np.array_equal(same[(5, 0)], same[(5, 1)])
    if whole:
        pop = [d for S in by_block["draw"] for d in S["draws"] if d["members"] == 3]
        assert len(pop) == 1 and pop[0]["seed"] == 2 ** 64 - 1
        single = {d["seed"]: d["picks"][0] for d in by_block["draw"][2]["draws"] if d["members"] == 1 and d["draw"] == 1 and d["B"] == 257 and d["her_ratio"] == 0.8 and d["use_her"]}
        assert np.array_equal(pop[0]["picks"][1], single[0])          # member 1 of seed 2^64 - 1 draws with seed 0


# ---------------------------------------------------------------------------------------------- her_sample_one, restated

def emu_sample(S, picks=None, defect=None):
    """her_sample_one on the PHYSICAL arrays of a store for given picks, in numpy; `defect`: one of DEFECTS planted into it"""
    D, N, cap, base, thr = S["D"], S["N"], S["cap"], S["base"], S["thr"]
    picks = S["picks"] if picks is None else picks
    eps = episodes_of(S)                      # the index has its own block; the sampler reads it as given
    if defect == "thr_f32":
        thr = float(np.float32(thr))
    row = (lambda lt: lt) if defect == "no_ring" else (lambda lt: (base + lt) % cap)
    B = len(picks)
    out = dict(states=np.zeros((B, D), np.float32), actions=np.zeros((B, 3), np.float32), next_states=np.zeros((B, D), np.float32),
               rewards=np.zeros(B, np.float32), dones=np.zeros(B, np.uint8))

    def state(n, t0, j):
        tt = t0 + j
        if j == 0:
            return S["obs0"][n] if (tt == 0 and defect != "obs0_ignored") else S["obs_after"][row(tt - 1), n]
        return (S["obs_after"] if defect == "obs_after_for_next" else S["next_obs"])[row(tt - 1), n]

    for b, (ep, st, h, sg) in enumerate(picks):
        n, t0, _ = eps[ep]
        t = row(t0 + st + (1 if defect == "row_off_by_one" else 0))
        sv, nv = state(n, t0, st).copy(), state(n, t0, st + 1).copy()
        r, dn = S["reward"][t, n], S["done"][t, n]
        if h:
            g = state(n, t0, sg)[:3].copy()
            form = "order" if defect == "sum_order" else "fused" if defect == "fused" else "ref"
            dis = distance(nv, g, D, form, f32_at_9=defect == "f32_at_9")
            far = dis >= thr if defect == "ge" else dis > thr
            r, dn = np.float32(-0.1 if far else 1.0), 0 if far else 1
            if D == 9 and defect != "keep_6_9":
                nv[6:9] = sv[6:9]
            sv[3:6] = g
            if defect != "goal_state_only":
                nv[3:6] = g
        out["states"][b], out["next_states"][b], out["actions"][b] = sv, nv, S["action"][t, n]
        out["rewards"][b], out["dones"][b] = r, dn
    return out


def first_difference(got, want):
    """(key, row) of the first element of a batch that differs bit for bit, or None"""
    for k in BATCH:
        a, b = bits(got[k]), bits(want[k])
        assert a.shape == b.shape, k
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        if len(bad):
            return k, int(bad[0])
    return None
