"""Float64 restatement of the fused policy forwards, derived error bounds for the two kernels, and a numpy emulation of the f16x3
arithmetic with a table of defects (test infrastructure; no GPU, no C oracle).

The nets are the reference's PolicyNet / QValueNet (D -> 256 -> 256 -> 3 | 1, relu, relu; the actor ends in bound * tanh), given as
dicts fc1.weight ... fc3.bias of f32 numpy arrays in torch.nn.Linear layout.

THE BOUNDS.  u = 2^-24 is the unit roundoff of f32 and g(n) = n u / (1 - n u) the usual constant of a sum of n rounded terms in any
order.  A tilde marks what the kernel holds, x~ = x_ref + e with |e| <= err(x); xa = |x_ref| + err(x) bounds |x~|.  Every quantity
below is computed in float64 from the inputs and from the reference's own intermediates: nothing is measured.

Exact-f32 actor (armenv_actor.h actor_forward_wave).  Every layer is a chain of f32 MFMAs: K products and the bias, each product
rounded at most once and carried through at most K additions, so per output
    err(y) <= g(K + 2) (sum_k |w| xa + |b|)  +  sum_k |w| err(x_k)
(layer 1: K = D + 1, the bias rides on a constant-1 input and the sum starts from zero; layer 2: K = 256, the accumulators start from
b2; layer 3: K = 256 over two chains per lane, one lane exchange and b3).  relu is 1-Lipschitz: err(relu(y)) <= err(y).

f16x3 layers (layers 1 and 2 of actor_forward_wg_f16x3).  Both operands are split v = hi + lo + dv, hi = f16(v), lo = f16(v - hi)
(v - hi is exact in f32), and the kernel accumulates hi*hi + hi*lo + lo*hi in f32; f16 products are exact in f32.  For |v| <= 65504
    |v - hi| <= e1(v) = max(2^-11 |v|, 2^-25)      (2^-25: half the spacing 2^-24 of f16 subnormals, which hi is below 2^-14)
    |dv|     <= d(v)  = max(2^-22 |v|, 2^-25)      (lo is an f16 SUBNORMAL whenever |v - hi| < 2^-14, i.e. for all |v| < 2^-3:
                                                    the "2^-22 relative" of the split is an absolute 2^-25 there)
    |lo|     <= e1(v) + d(v)
For the weights, the biases and an observation the kernel sees exactly the f32 value the reference has, so hi, lo and dv are
computed here exactly instead (an entry with 11 significant bits has lo = dv = 0); for an activation, or an action that an earlier
pass of the kernel produced, the formulas are evaluated at xa (all three are monotone).  With w = wh + wl + dw, x~ = xh + xl + dx
    w x~ - (wh xh + wh xl + wl xh) = wl xl + dw x~ + (wh + wl) dx
so per output
    err(y) <= sum_k [ |wl| |xl| + |dw| xa + (|wh| + |wl|) |dx| ]                     split residuals and the dropped lo*lo
            + g(3 K + 2) (sum_k (|wh| + |wl|) (|xh| + |xl|) + |b|)                   3 K exact products and the bias, summed in f32
            + sum_k |w| err(x_k)                                                     incoming error
(a first-order sketch has 2^-22 |w| |x| for the dropped term; |wl| |xl| is the same when both los are normal and is the correct,
larger term when one of them is a subnormal).  Layer 1 has K = in_dim + 1: its bias is column in_dim of W1aug and is split like a weight,
against the input 1 = hi exactly.  Inside datd3_forward_wg every net runs with in_dim = OBS + 3 (the actors against three zero
inputs, which add no error).  The MFMA's own 16-term sums are taken to round each addition to nearest; the f32 accumulators are far
above 2^-126 on every case, so no underflow term.

Layer 3 is f32 in both kernels (layer3_column, v_mfma_f32_4x4x1): the exact-f32 formula with K = 256.

Output.  QValueNet: z itself.  PolicyNet: out = f32(bound * tanhf(z~)); |tanh'| <= 1, tanhf is taken as 4 ulp (the ROCm device
library's table of function accuracies is not shipped with the toolchain; 4 ulp is the figure assumed here -- the ONLY number in this
file that is not derived), an ulp of a value in [-1, 1] is at most 2^-23, and the final product rounds once:
    err(out) <= bound (err(z) + 4 * 2^-23) + u bound.

Domain: every |v| that is split must be <= 65504 (above, hi = inf, lo = -inf and the product sums are NaN).  The conversion rounds
to nearest, so the kernel's own value of an activation may sit above a reference value of 65504 by its error and still convert to
65504: the split formulas hold up to F16_ROUNDS_TO_INF = 65520, and bound_f16x3 raises when xa reaches it.

TAKE_ACTION.  datd3_forward_wg decides `picked = q1 >= q2 ? 0 : 1` (armenv_actor.h, the line after the loop over the four nets,
citing DATD3_mlp.py:107): actor 1 on a tie.  DADDPG is the same with critic2 the same object as critic1.  The critics see the
kernel's OWN actions, so err(a_i) enters their layer 1 as an incoming error.
"""
import numpy as np

KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
U = 2.0 ** -24
F16_MAX = 65504.0
F16_ROUNDS_TO_INF = 65520.0       # f32 values from here on convert to +-inf (round to nearest even)
TANHF_ULP = 4          # assumed (see the docstring): ulps of the device tanhf


def g(n):
    return n * U / (1.0 - n * U)


def _w(net):
    return [np.asarray(net[k], dtype=np.float32) for k in KEYS]


def forward64(net, x, bound, raw):
    """The MLP in float64.  Returns dict(out [n, rows], h1, h2 (after relu), z, s1, s2, s3 (per-layer sums of |w| |x| + |b|))."""
    W1, b1, W2, b2, W3, b3 = (a.astype(np.float64) for a in _w(net))
    x = np.asarray(x, dtype=np.float64)
    h1 = np.maximum(x @ W1.T + b1, 0.0)
    h2 = np.maximum(h1 @ W2.T + b2, 0.0)
    z = h2 @ W3.T + b3
    out = z if raw else float(np.float32(bound)) * np.tanh(z)
    return dict(out=out, h1=h1, h2=h2, z=z, s1=np.abs(x) @ np.abs(W1).T + np.abs(b1), s2=h1 @ np.abs(W2).T + np.abs(b2),
                s3=h2 @ np.abs(W3).T + np.abs(b3))


def take_action64(nets, s, bound):
    """(actor1, actor2, critic1, critic2) on states s in float64: a1, a2, q1, q2, picked (0 actor1 on q1 >= q2, 1 actor2), action,
    and the four forward64 results under "fwd"."""
    s = np.asarray(s, dtype=np.float64)
    f1, f2 = forward64(nets[0], s, bound, False), forward64(nets[1], s, bound, False)
    c1 = forward64(nets[2], np.concatenate([s, f1["out"]], 1), bound, True)
    c2 = forward64(nets[3], np.concatenate([s, f2["out"]], 1), bound, True)
    q1, q2 = c1["out"][:, 0], c2["out"][:, 0]
    picked = (~(q1 >= q2)).astype(np.uint8)
    return dict(a1=f1["out"], a2=f2["out"], q1=q1, q2=q2, picked=picked, action=np.where(picked[:, None] == 1, f2["out"], f1["out"]),
                fwd=(f1, f2, c1, c2))


# ----------------------------------------------------------------------------------------------------------- splits
def split16(v):
    """hi = f16(v), lo = f16(v - hi) of f32 values, as np.float16"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def _exact_split(v32):
    """|hi| + |lo|, |lo|, |v - hi - lo| of exactly known f32 values, in float64"""
    hi, lo = split16(v32)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    return np.abs(hi) + np.abs(lo), np.abs(lo), np.abs(v32.astype(np.float64) - hi - lo)


def _e1(v):
    return np.maximum(2.0 ** -11 * v, 2.0 ** -25)


def _d(v):
    return np.maximum(2.0 ** -22 * v, 2.0 ** -25)


def _split_terms(x_ref, ex):
    """(A, l, d, xa) >= (|xh| + |xl|, |xl|, |dx|, |x~|) of the kernel's input: exact where ex == 0 (the kernel holds f32(x_ref) = x_ref),
    from the formulas at xa = |x_ref| + ex elsewhere"""
    xa = np.abs(x_ref) + ex
    if xa.max(initial=0.0) >= F16_ROUNDS_TO_INF:
        raise ValueError("outside the f16x3 domain: |x| up to %g" % xa.max())
    A0, l0, d0 = _exact_split(x_ref.astype(np.float32))
    l1 = _e1(xa) + _d(xa)
    exact = ex == 0
    return np.where(exact, A0, xa + _e1(xa) + l1), np.where(exact, l0, l1), np.where(exact, d0, _d(xa)), xa


def _layer_f16x3(W32, b32, x_ref, ex, bias_in_mfma, K):
    """err of one f16x3 layer per (row, output).  bias_in_mfma: the bias is a split column against a constant 1 (layer 1)"""
    if bias_in_mfma:
        W32 = np.concatenate([W32, b32[:, None]], 1)
        x_ref = np.concatenate([x_ref, np.ones((x_ref.shape[0], 1))], 1)
        ex = np.concatenate([ex, np.zeros((ex.shape[0], 1))], 1)
        b_abs = 0.0
    else:
        b_abs = np.abs(b32.astype(np.float64))
    if np.abs(W32).max() > F16_MAX:
        raise ValueError("outside the f16x3 domain: a weight above 65504")
    Aw, lw, dw = _exact_split(W32)
    Ax, lx, dx, xa = _split_terms(x_ref, ex)
    split = lx @ lw.T + xa @ dw.T + dx @ Aw.T
    accum = g(3 * K + 2) * (Ax @ Aw.T + b_abs)
    return split + accum + ex @ np.abs(W32.astype(np.float64)).T


def _layer_f32(W32, b32, x_ref, ex, K):
    Wa = np.abs(W32.astype(np.float64))
    return g(K + 2) * ((np.abs(x_ref) + ex) @ Wa.T + np.abs(b32.astype(np.float64))) + ex @ Wa.T


def _out_err(ez, bound, raw):
    b = float(np.float32(bound))
    return ez if raw else b * (ez + TANHF_ULP * 2.0 ** -23) + U * b


def _bound(net, x, bound, raw, in_err, f16, k1):
    W1, b1, W2, b2, W3, b3 = _w(net)
    x = np.asarray(x, dtype=np.float64)
    ex = np.zeros_like(x) if in_err is None else np.asarray(in_err, dtype=np.float64)
    ref = forward64(net, x, bound, raw)
    K1 = (W1.shape[1] if k1 is None else k1) + 1
    if f16:
        e1 = _layer_f16x3(W1, b1, x, ex, True, K1)
        e2 = _layer_f16x3(W2, b2, ref["h1"], e1, False, 256)
    else:
        e1 = _layer_f32(W1, b1, x, ex, K1)
        e2 = _layer_f32(W2, b2, ref["h1"], e1, 256)
    ez = _layer_f32(W3, b3, ref["h2"], e2, 256)
    return dict(out=_out_err(ez, bound, raw), h1=e1, h2=e2, z=ez, ref=ref)


def bound_f32(net, x, bound, raw=False, in_err=None, full=False):
    """per-output bound on |actor_forward_wave - forward64| ([n, rows]); in_err: bound on the error of the inputs the kernel sees"""
    r = _bound(net, x, bound, raw, in_err, False, None)
    return r if full else r["out"]


def bound_f16x3(net, x, bound, raw=False, in_err=None, k1=None, full=False):
    """per-output bound on |actor_forward_wg_f16x3 - forward64|; k1: the in_dim the kernel runs the net with (datd3_forward_wg: OBS + 3)"""
    r = _bound(net, x, bound, raw, in_err, True, k1)
    return r if full else r["out"]


def bound_take_action(nets, s, bound):
    """bounds for datd3_forward_wg: dict(a1, a2 [n, 3], q1, q2 [n]) and the reference under "ref" """
    s = np.asarray(s, dtype=np.float64)
    ref = take_action64(nets, s, bound)
    k1 = s.shape[1] + 3
    ea1 = bound_f16x3(nets[0], s, bound, False, k1=k1)
    ea2 = bound_f16x3(nets[1], s, bound, False, k1=k1)
    z = np.zeros_like(s)
    eq1 = bound_f16x3(nets[2], np.concatenate([s, ref["a1"]], 1), bound, True, in_err=np.concatenate([z, ea1], 1))[:, 0]
    eq2 = bound_f16x3(nets[3], np.concatenate([s, ref["a2"]], 1), bound, True, in_err=np.concatenate([z, ea2], 1))[:, 0]
    return dict(a1=ea1, a2=ea2, q1=eq1, q2=eq2, ref=ref)


def clear_rows(b):
    """rows on which the reference's pick is decided beyond the two critics' bounds"""
    return np.abs(b["ref"]["q1"] - b["ref"]["q2"]) > b["q1"] + b["q2"]


# ----------------------------------------------------------------------------------------------------------- emulation
# name -> the agents it applies to ("any": every f16x3 forward; "two": the four-net pass only).  hl = hi(w) * lo(x), lh = lo(w) * hi(x).
DEFECTS = {
    "l1_drop_hh": "any", "l1_drop_hl": "any", "l1_drop_lh": "any",
    "l2_drop_hh": "any", "l2_drop_hl": "any", "l2_drop_lh": "any",
    "lo_flushed_when_subnormal": "any",        # every lo part below 2^-14 becomes 0 (an MFMA or a conversion that flushes)
    "lo_from_rounded": "any",                  # lo = f16(f16(x) - hi): identically 0
    "b1_hi_only": "any",                       # the bias column of W1aug without its lo part
    "w2_lo_of_other_net": "two",               # the W2 lo table of another net of the four (net i reads net (i + 2) % 4's)
}


def _lo(v32, defect):
    hi, lo = split16(v32)
    if defect == "lo_from_rounded":
        lo = np.zeros_like(lo)
    elif defect == "lo_flushed_when_subnormal":
        lo = np.where(np.abs(lo.astype(np.float32)) < 2.0 ** -14, np.float16(0), lo)
    return hi.astype(np.float32), lo.astype(np.float32)


def _emu_layer(W32, acc0, x32, defect, layer, w_lo_from=None):
    """three f32 GEMMs of f16-valued operands (exact products, f32 accumulation in the BLAS's fixed order) on top of acc0"""
    wh, wl = _lo(W32, defect)
    if w_lo_from is not None:
        wl = _lo(w_lo_from, defect)[1]
    xh, xl = _lo(x32, defect)
    acc = acc0
    for name, a, b in (("hh", xh, wh), ("hl", xl, wh), ("lh", xh, wl)):
        if defect != "l%d_drop_%s" % (layer, name):
            acc = (acc + a @ b.T).astype(np.float32)
    return acc


def emulate_f16x3(net, x, bound, raw, defect=None, other=None):
    """The f16x3 forward in numpy: np.float16 hi / lo splits, three products in float32, f32 accumulation.  defect: a key of DEFECTS
    (other: the net whose W2 lo table "w2_lo_of_other_net" reads).  Returns f32 [n, rows]."""
    assert defect is None or defect in DEFECTS, defect
    W1, b1, W2, b2, W3, b3 = _w(net)
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    W1a = np.concatenate([W1, b1[:, None]], 1)
    if defect == "b1_hi_only":
        W1a[:, -1] = split16(b1)[0].astype(np.float32)
    xa = np.concatenate([x, np.ones((n, 1), np.float32)], 1)
    relu = lambda v: np.maximum(v, np.float32(0))
    h1 = relu(_emu_layer(W1a, np.zeros((n, 256), np.float32), xa, defect, 1))
    lo_from = _w(other)[2] if defect == "w2_lo_of_other_net" else None
    h2 = relu(_emu_layer(W2, np.broadcast_to(b2, (n, 256)), h1, defect, 2, lo_from))
    z = (h2 @ W3.T + b3).astype(np.float32)
    if raw:
        return z
    return (np.tanh(z.astype(np.float64)).astype(np.float32) * np.float32(bound)).astype(np.float32)


def emulate_take_action(nets, s, bound, defect=None):
    """the four-net pass on the emulation: dict(a1, a2, q1, q2, picked, action) in f32"""
    s = np.asarray(s, dtype=np.float32)
    a1 = emulate_f16x3(nets[0], s, bound, False, defect, nets[2])
    a2 = emulate_f16x3(nets[1], s, bound, False, defect, nets[3])
    q1 = emulate_f16x3(nets[2], np.concatenate([s, a1], 1), bound, True, defect, nets[0])[:, 0]
    q2 = emulate_f16x3(nets[3], np.concatenate([s, a2], 1), bound, True, defect, nets[1])[:, 0]
    picked = (~(q1 >= q2)).astype(np.uint8)
    return dict(a1=a1, a2=a2, q1=q1, q2=q2, picked=picked, action=np.where(picked[:, None] == 1, a2, a1))


def take_action_ratios(got, b):
    """max (err / bound) of a take_action result (dict or (action, q1, q2, picked)) against bound_take_action's b: q1, q2 raw on every
    row, the action against the picked actor's bound on clear rows; and whether the picks agree on clear rows"""
    ref = b["ref"]
    clear = clear_rows(b)
    rq1 = np.abs(got["q1"].astype(np.float64) - ref["q1"]) / b["q1"]
    rq2 = np.abs(got["q2"].astype(np.float64) - ref["q2"]) / b["q2"]
    ea = np.where(ref["picked"][:, None] == 1, b["a2"], b["a1"])
    ra = (np.abs(got["action"].astype(np.float64) - ref["action"]) / ea)[clear]
    same = np.array_equal(np.asarray(got["picked"])[clear], ref["picked"][clear])
    return dict(q1=float(rq1.max()), q2=float(rq2.max()), action=float(ra.max(initial=0.0)), picks_agree=bool(same))


def head(b, n):
    """the first n rows of bound_take_action's result (the rows are independent)"""
    out = {k: b[k][:n] for k in ("a1", "a2", "q1", "q2")}
    out["ref"] = {k: b["ref"][k][:n] for k in ("a1", "a2", "q1", "q2", "picked", "action")}
    return out
