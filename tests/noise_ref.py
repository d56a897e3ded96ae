"""The rollouts' exploration noise in float64, with a derived error bound (test infrastructure; CPU only).

The engine's `policy_noise` (csrc/armenv_env.h) draws one Philox4x32-10 block per (env, episode, step) -- counter
{id, id >> 32, episode index, 0x80000000 | step}, key {seed, seed >> 32} -- forms four f32 uniforms, and returns three Box-Muller
normals: z0 = r0 cos(2 pi u1), z1 = r0 sin(2 pi u1), z2 = r1 cos(2 pi u3), r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2).

words()      the four Philox words of the block, through learner_ref64.philox4x32_10 (pinned against the oracle's known answers).
uniforms()   the f32 uniforms EXACTLY as the kernel forms them ((float)w rounds to nearest even, the +1 is an f32 add, the multiply by
             2^-32 is exact): they are the inputs of the function under test, not part of its error.
reference()  the three values in float64.  The angle goes through the exactly reduced argument d = u - k / 4 (k = rint(4 u); exact in
             f64, u has 24 bits), so sin and cos are TRUE zeros at u = k / 4 and relative errors stay meaningful next to them; ln u is
             taken as log1p(u - 1) above 1/2 (u - 1 is exact), so the radius keeps its relative accuracy next to u = 1 and is a true
             zero there.  float64's own error is below 1e-15 against a bound of order 1e-7.
bound()      |kernel - reference| <= bound, per output, term by term (below).  No constant tolerance.
emulate()    the kernel's arithmetic in numpy f32 (one rounding per fmaf), with named planted defects; used only to show that the case
             table of tests/noise_cases.py is sensitive (tests/test_noise_ref.py).

The bound.  eps = 2^-24 is the unit roundoff of f32 (one correctly rounded operation: relative error <= eps), ulp = 2^-23 the
relative size of "1 ulp".  The accuracies of the two hardware builtins (v_log_f32, v_sqrt_f32: 1 ulp each, as the CDNA ISA guide states
for both) and of the Cephes sinf / cosf kernels on |x| <= pi / 4 (< 1 ulp) are TAKEN FROM THE KERNEL'S OWN COMMENTS: this bound
holds the kernel to what it claims.

  radius   L^ = log2(u) (1 + d1)                  |d1| <= ulp                builtin log
           p^ = -c L^ (1 + d2)                    |d2| <= eps                f32 product; c = f32(2 ln 2) = 2 ln 2 (1 + dc), dc exact below
           r^ = sqrt(p^) (1 + d3)                 |d3| <= ulp                builtin sqrt; the square root halves what p^ carries
           => |r^ - r| <= r er,  er = (ulp + dc + eps) / 2 + ulp
           u = 1: log2(1) = 0 has no ulp to be wrong by, -c * 0 = -0, sqrt(-0) = -0: the draw is +-0 exactly (er * 0 = 0).
  angle    k = (int)fmaf(u, 4, 0.5) and u - k / 4 are exact (the comment's claim, and a theorem: both are sums of two f32 numbers whose
           result has at most 24 bits)
           x^ = P d (1 + d4)                      |d4| <= eps                P = f32(2 pi) = 2 pi (1 + dp), dp exact below
           => x^ = x (1 + ex), |ex| <= ea = dp + eps; |x| <= pi / 4 (1 + 2^-23) whichever way a tie of k goes
           sin x^ - sin x = x ex cos(xi),  cos x^ - cos x = -x ex sin(xi)  for a xi between x and x^:
           |.| <= |x| ea  and  |x| ea (|sin x| + |x| ea)                     propagation through sin and cos on |x| <= pi / 4
           s^ = sin(x^) (1 + d5), c^ = cos(x^) (1 + d6)      |d5|, |d6| <= ulp    the polynomial kernels, evaluation included
           => |t^ - t| <= at = ulp |t| + (1 + ulp) * (the propagation term)   for t = whichever of sin x, cos x the quadrant selects
           (swaps and sign flips are exact).  At u = k / 4: x = 0, the sine is an exact 0 and the cosine an exact 1.
  product  z^ = r^ t^ (1 + d7)                    |d7| <= eps
           => |z^ - z| <= r |t| er + r at + eps r |t|, times (1 + 2^-20) for every product of two of the terms above.

For scale: between 6.5 (a cosine at x ~ 0) and 8.2 (a sine at |x| = pi / 4, where the propagation term is x / sin x = 1.11 times ea)
times 2^-24 relative.  An f32 emulation of the kernel with correctly rounded log2 and sqrt (emulate() here) reaches 4.5 * 2^-24,
0.56 of the bound, over 4e6 draws and is exact at the edge words, so a correct kernel has room and the reference alone sits well
inside.
"""
import math

import numpy as np

import learner_ref64 as LR

F = np.float32
EPS = 2.0 ** -24
ULP = 2.0 ** -23
C_LN = F(1.3862943611198906)          # the kernel's f32(2 ln 2)
C_2PI = F(6.283185307179586)          # the kernel's f32(2 pi)
D_LN = abs(float(C_LN) - 2.0 * math.log(2.0)) / (2.0 * math.log(2.0))
D_2PI = abs(float(C_2PI) - 2.0 * math.pi) / (2.0 * math.pi)
SECOND_ORDER = 1.0 + 2.0 ** -20
STEP_BIT = 0x80000000
_M32 = np.uint64(0xFFFFFFFF)

KEY_DEFECTS = ("step-bit-dropped", "episode-not-minus-one", "id-high-dropped", "seed-high-dropped")
ARITH_DEFECTS = ("radius-plus-one-dropped", "sin-cos-exchanged", "k4-sign", "nz2-first-angle", "log2-without-ln2", "two-pi-6.28",
                 "sine-coefficient")
DEFECTS = ARITH_DEFECTS + KEY_DEFECTS


def words(seed, env_ids, episode_index, step, defect=None):
    """uint64 [n, 4]: the Philox words of the noise block of global env ids `env_ids` at the running episode's index (number of resets
    so far minus one, mod 2^32) and step counter `step` (arrays broadcast).  defect: one of KEY_DEFECTS, for emulate_keys()."""
    ids, ep, sp = np.broadcast_arrays(np.asarray(env_ids, dtype=np.uint64), np.asarray(episode_index, dtype=np.uint64) & _M32,
                                      np.asarray(step, dtype=np.uint64) & _M32)
    ids, ep, sp = ids.reshape(-1), ep.reshape(-1), sp.reshape(-1)
    seed = int(seed) & (2 ** 64 - 1)
    hi = ids >> np.uint64(32)
    if defect == "id-high-dropped":
        hi = np.zeros_like(hi)
    if defect == "episode-not-minus-one":
        ep = (ep + np.uint64(1)) & _M32
    if defect != "step-bit-dropped":
        sp = sp | np.uint64(STEP_BIT)
    k1 = 0 if defect == "seed-high-dropped" else seed >> 32
    ctr = np.stack([ids & _M32, hi, ep, sp], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, k1], dtype=np.uint64), (ids.size, 2))
    return LR.philox4x32_10(ctr, key)


def uniforms(w, plus_one=True):
    """f32 [n, 4]: u0 and u2 = ((float)w + 1) * 2^-32 in (0, 1], u1 and u3 = (float)w * 2^-32 in [0, 1]"""
    f = np.asarray(w, dtype=np.uint64).astype(F)                     # uint64 -> f32 rounds to nearest even, once
    one = F(1.0) if plus_one else F(0.0)
    k = F(2.0 ** -32)
    return np.stack([(f[:, 0] + one) * k, f[:, 1] * k, (f[:, 2] + one) * k, f[:, 3] * k], -1)


def _radius64(u):
    u = u.astype(np.float64)
    with np.errstate(divide="ignore"):
        ln = np.where(u > 0.5, np.log1p(u - 1.0), np.log(u))
    return np.sqrt(-2.0 * ln)


def _angle64(u):
    """(sin 2 pi u, cos 2 pi u) in float64 through d = u - k / 4"""
    u = u.astype(np.float64)
    k = np.rint(4.0 * u)
    x = 2.0 * math.pi * (u - 0.25 * k)
    s, c = np.sin(x), np.cos(x)
    q = k.astype(np.int64) & 3
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def reference(w):
    """float64 [n, 3] of the words w"""
    u = uniforms(w)
    r0, r1 = _radius64(u[:, 0]), _radius64(u[:, 2])
    s0, c0 = _angle64(u[:, 1])
    _, c1 = _angle64(u[:, 3])
    return np.stack([r0 * c0, r0 * s0, r1 * c1], -1)


def _kernel_k(u):
    """the kernel's quadrant (int)fmaf(u, 4, 0.5): 4 u + 0.5 is exact in f64, one rounding to f32, truncation"""
    return (u.astype(np.float64) * 4.0 + 0.5).astype(F).astype(np.int64)


def bound(w):
    """float64 [n, 3]: the module docstring's bound for each output"""
    u = uniforms(w)
    er = 0.5 * (ULP + D_LN + EPS) + ULP
    ea = D_2PI + EPS
    out = []
    for ri, ai, want_sin in ((0, 1, False), (0, 1, True), (2, 3, False)):
        r = _radius64(u[:, ri])
        s, c = _angle64(u[:, ai])
        k = _kernel_k(u[:, ai])
        x = np.abs(2.0 * math.pi * (u[:, ai].astype(np.float64) - 0.25 * k))          # the kernel's own reduced argument
        takes_sin = ((k & 1) == 1) != want_sin               # the output is +-sin x (else +-cos x) of the reduced argument
        t = np.abs(s if want_sin else c)
        prop = np.where(takes_sin, x * ea, x * ea * (np.abs(np.sin(x)) + x * ea))
        at = ULP * t + (1.0 + ULP) * prop
        out.append((r * t * er + r * at + EPS * r * t) * SECOND_ORDER)
    return np.stack(out, -1)


# ---- the kernel's arithmetic in f32 ----

def _fma32(a, b, c):
    """fmaf on f32 arrays with ONE rounding: a * b is exact in f64; the f64 sum is rounded to odd (Boldo-Melquiond), after which the
    rounding to f32 is the rounding of the exact value (53 >= 24 + 2)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                      # TwoSum: p + c = s + err exactly
    bits = s.copy().view(np.int64)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
    up = (err > 0) == (s > 0)                                # towards larger magnitude
    bits = np.where(fix, bits + np.where(up, 1, -1), bits)
    with np.errstate(over="ignore"):
        return bits.view(np.float64).astype(F)


SIN_C = (F(-1.9515295891e-4), F(8.3321608736e-3), F(-1.6666654611e-1))
COS_C = (F(2.443315711809948e-5), F(-1.388731625493765e-3), F(4.166664568298827e-2))


def _sincos32(u, defect):
    k = _fma32(u, F(4.0), F(0.5)).astype(np.int64)
    kf = k.astype(F)
    two_pi = F(6.28) if defect == "two-pi-6.28" else C_2PI
    x = two_pi * _fma32(F(-0.25), kf, u)
    z = x * x
    s3 = F(float(SIN_C[2]) * (1.0 + 1e-5)) if defect == "sine-coefficient" else SIN_C[2]
    sx = _fma32(_fma32(_fma32(SIN_C[0], z, SIN_C[1]), z, s3) * z, x, x)
    cx = _fma32(_fma32(_fma32(COS_C[0], z, COS_C[1]), z, COS_C[2]) * z, z, _fma32(F(-0.5), z, F(1.0)))
    odd = (k & 1) == 1
    ss, cc = np.where(odd, cx, sx), np.where(odd, sx, cx)
    s = np.where((k & 2) != 0, -ss, ss)
    c = np.where(((k + 1) & 2) != 0, -cc, cc)
    if defect == "k4-sign":
        c = np.where(k == 4, -c, c)                          # the quadrant put back as if k = 4 were k = 2
    if defect == "sin-cos-exchanged":
        s, c = c, s
    return s.astype(F), c.astype(F)


def emulate(w, defect=None):
    """f32 [n, 3]: policy_noise's statements on the words w, log2 and sqrt correctly rounded.  defect: None or one of ARITH_DEFECTS."""
    assert defect is None or defect in ARITH_DEFECTS, defect
    u = uniforms(w, plus_one=defect != "radius-plus-one-dropped")
    with np.errstate(divide="ignore", invalid="ignore"):
        def radius(x):
            lg = np.log2(x.astype(np.float64)).astype(F)
            p = (F(-1.0) if defect == "log2-without-ln2" else -C_LN) * lg
            return np.sqrt(p.astype(np.float64)).astype(F)
        r0, r1 = radius(u[:, 0]), radius(u[:, 2])
        s0, c0 = _sincos32(u[:, 1], defect)
        s1, c1 = _sincos32(u[:, 3], defect)
        if defect == "nz2-first-angle":
            c1 = c0
        return np.stack([r0 * c0, r0 * s0, r1 * c1], -1).astype(F)


def emulate_keys(seed, env_ids, episode_index, step, defect=None):
    """emulate() from the key, so that the keying defects can be planted too"""
    if defect in KEY_DEFECTS:
        return emulate(words(seed, env_ids, episode_index, step, defect))
    return emulate(words(seed, env_ids, episode_index, step), defect)


def ratio(got, ref, bnd):
    """max err / bound; a zero bound demands err = 0; inf where got is not finite"""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != ref.shape or not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    return float(q.max(initial=0.0))
