"""The cases of tests/test_actor_ref64.py and tests/test_gpu_actor_ref64.py (test infrastructure): nets and observations for the
fused policy forwards, built by seeded CPU generators as f32 numpy arrays, with the float64 reference and the derived bounds of
tests/actor_ref64.py computed once per case and shared.

Single-net cases run through both actor kernels (policy kinds "actor" and "actor_f16x3"; the cases tagged ddpg are the DDPG agent's
actor through the same kinds); four-net cases through datd3_forward (datd3, darc: four distinct nets; daddpg: critic2 IS critic1).

Conditions every case must meet (asserted on the CPU by tests/test_actor_ref64.py, with the reference alone):
  - at least SAT_MIN of the actor outputs have |z_ref| < 2 (tanh saturation would hide errors): where the requested layer scales give
    more, fc3 is scaled down by a power of two until the 90th percentile of |z| is at most 1 (`fit`);
  - four-net cases: at most AMB_MAX of the rows are ambiguous (|q1 - q2| <= bound(q1) + bound(q2)) and each pick occurs on at least
    PICK_MIN of the clear rows.  With two critics, critic2's b3 is shifted by the median of q1 - q2; then, and with DADDPG's one
    critic, the seed is advanced until the condition holds.  The identical-actors case is excepted: there q1 == q2 on every row by
    construction.

What the worst-case bounds cost the table.  The bounds sum |w| |x| and carry the result through |W2| and |W3|, so on a net whose
256-term sums cancel they are ~10^3 times the error a correct kernel makes, and a missing lo pass (2^-12 relative, random signs) stays
inside them.  Two families answer that: the COHERENT nets (all weights positive, lo parts of one sign, hidden-1 activations that are
exactly the bias on most units), on which every defect of actor_ref64.DEFECTS is 3 to 10 times the bound; and, for the four-net cases,
nets with fc2 >= 0 and one sign per fc3 row, without which no pick is clear of the two critics' bounds at any scale.  For the same
reason the four-net table has no 65504 entries (they swamp the critics' bounds) and no observation scale of 1e-3 (q would not depend
on the row): the single-net table has both.
"""
import functools

import numpy as np

import actor_ref64 as R

SAT_MIN, AMB_MAX, PICK_MIN = 0.9, 0.1, 0.1
N = 200                       # rows per case: three full waves and a ragged one
KEYS = R.KEYS
F = np.float32


def mlp(rng, D, rows, scales=(1.0, 1.0, 1.0)):
    """uniform in +-scale / sqrt(fan_in), weights and biases, as torch.nn.Linear draws them at scale 1"""
    net = {}
    for (name, fan_in, fan_out), sc in zip((("fc1", D, 256), ("fc2", 256, 256), ("fc3", 256, rows)), scales):
        b = sc / np.sqrt(fan_in)
        net[name + ".weight"] = rng.uniform(-b, b, (fan_out, fan_in)).astype(F)
        net[name + ".bias"] = rng.uniform(-b, b, fan_out).astype(F)
    return net


def observations(rng, n, D, scale):
    """uniform in +-scale; rows 0, 7 and n - 1 all zero; in rows 1..D feature (row - 1) dominates by 64x"""
    x = (rng.uniform(-1, 1, (n, D)) * scale).astype(F)
    for d in range(min(D, n - 2)):
        x[1 + d, d] *= F(64)
    for r in (0, 7, n - 1):
        if r < n:
            x[r] = 0
    return x


def fit(net, x, bound, up=False):
    """scale fc3 down by a power of two until the 90th percentile of |z_ref| is at most 1 (up: or up, into (0.5, 1])"""
    z = np.abs(R.forward64(net, x, bound, False)["z"])
    p = np.quantile(z, 0.9)
    if p > 1.0 or up:
        k = F(2.0 ** -np.ceil(np.log2(p)))
        net["fc3.weight"] = net["fc3.weight"] * k
        net["fc3.bias"] = net["fc3.bias"] * k
    return net


def ramp(n=256):
    return (2.0 ** np.linspace(-10, 2, n)).astype(F)


def nextafter32(v, up):
    return np.nextafter(F(v), F(np.inf if up else -np.inf), dtype=F)


def plant_boundaries(rng, net, big=True):
    """Entries at the edges of the f16 split in W2, W1 and b1: 2^-14 (smallest normal f16), 2^-24 (smallest subnormal), 2^-25 (half of
    it: the tie), the f32 neighbours of each, either sign; exactly 11 significant bits (lo = 0) and 22 (dv = 0); and 65504 -- each of
    the three 65504s on a unit whose consumers are scaled down so that the outputs stay informative."""
    vals = []
    for p in (2.0 ** -14, 2.0 ** -24, 2.0 ** -25):
        vals += [p, nextafter32(p, True), nextafter32(p, False)]
    vals += [1.0 + 2.0 ** -10, 0.75 * (1.0 + 2.0 ** -10), 1.5 + 2.0 ** -12 + 2.0 ** -22, 0.046875 * (1 + 2.0 ** -12)]
    vals = np.array(vals + [-v for v in vals], dtype=F)
    W1, b1, W2 = net["fc1.weight"], net["fc1.bias"], net["fc2.weight"]
    D = W1.shape[1]
    for i, v in enumerate(vals):
        W2[(7 * i + 3) % 256, (11 * i + 5) % 256] = v
        W1[(5 * i + 2) % 256, i % D] = v
        b1[(3 * i + 1) % 256] = v
    if not big:
        return net
    # 65504: W2[40][41] (row 40's fc3 column scaled down); W1[50][0] with feature 0 at most 0.4 (h1 <= 3e4) and b1[60] on a zero W1 row
    # (h1 = 65504 exactly) -- columns 50 and 60 of W2 scaled down
    W2[40, 41] = F(65504)
    net["fc3.weight"][:, 40] *= F(2.0 ** -18)
    W1[50, :] = 0; W1[50, 0] = F(65504); b1[50] = 0
    W1[60, :] = 0; b1[60] = F(65504)
    W2[:, 50] *= F(2.0 ** -16); W2[:, 60] *= F(2.0 ** -16)
    return net


def coherent_values(rng, shape, e, sign=+1):
    """h (1 + sign 2^-12) with h = (17 + r) / 16 * 2^e, r in 0..14: positive, hi = h and lo = sign h 2^-12 EXACTLY (dv = 0), so the lo
    parts of a whole row have one sign and a missing lo pass is a coherent error, not a random walk"""
    h = (17 + rng.integers(0, 15, shape)) / 16.0 * 2.0 ** np.asarray(e, dtype=np.float64)
    return (h * (1 + sign * 2.0 ** -12)).astype(F)


def coherent_net(rng, D, rows, live, sign=+1):
    """All weights positive with same-signed lo parts.  `live`: the share of hidden-1 units that see the input (tiny bias); the others
    have a zero W1 row and h1 = b1 exactly, so that the ACTIVATIONS' lo parts are coherent too.  W2 in [2^-8, 2^-7): its lo parts are
    f16 subnormals."""
    nl = int(round(256 * live))
    W1 = coherent_values(rng, (256, D), -3 + rng.integers(-3, 1, (1, D)), sign); W1[nl:] = 0     # (each net weighs the features its own way)
    b1 = coherent_values(rng, 256, -1, sign); b1[:nl] = coherent_values(rng, nl, -7, sign)
    W3 = coherent_values(rng, (rows, 256), -10, sign)
    if rows == 3:
        W3[1] = -W3[1]
    return {"fc1.weight": W1, "fc1.bias": b1, "fc2.weight": coherent_values(rng, (256, 256), -8, sign),
            "fc2.bias": coherent_values(rng, 256, -6, sign), "fc3.weight": W3, "fc3.bias": np.zeros(rows, F)}


def coherent_obs(rng, n, D):
    return coherent_values(rng, (n, D), rng.integers(-3, 1, (n, D)))


def domain_edge(net, x, bound):
    """fc1 scaled up by the power of two that puts the largest h1 in (3e4, 6e4], fc2 scaled down by the same"""
    m = R.forward64(net, x, bound, False)["h1"].max()
    k = np.floor(np.log2(6.0e4 / m))
    net["fc1.weight"] = net["fc1.weight"] * F(2.0 ** k); net["fc1.bias"] = net["fc1.bias"] * F(2.0 ** k)
    net["fc2.weight"] = net["fc2.weight"] * F(2.0 ** -k)
    return net


S = (2.0 ** -8, 2.0 ** -4, 2.0 ** 4)
LAYER_SCALES = ([(1.0, 1.0, 1.0)] + [(f, 1.0, 1.0) for f in S] + [(1.0, f, 1.0) for f in S] + [(1.0, 1.0, f) for f in S] +
                # what a trained net can show: small W2 under large W3, large W1 over small W2
                [(1.0, 2.0 ** -4, 2.0 ** 4), (1.0, 2.0 ** -8, 2.0 ** 4), (2.0 ** 4, 2.0 ** -4, 1.0), (2.0 ** 4, 2.0 ** -8, 2.0 ** 4),
                 (2.0 ** -4, 2.0 ** 4, 2.0 ** -4)])
OBS_SCALES = (1e-3, 1.0, 30.0)
MIXED = (2.0 ** 4, 2.0 ** -8, 2.0 ** 4)        # the mixed-scale net of the batch-size and fused-path tests


def _sc(s):
    return "x".join("%g" % np.log2(v) for v in s)


def _single_cases():
    out, seed = [], 100
    for i, sc in enumerate(LAYER_SCALES):
        for j, os_ in enumerate(OBS_SCALES):
            for D in ((6, 9) if i == 0 else ((6, 9)[(i + j) % 2],)):
                seed += 1
                out.append(dict(id="scale-%s-obs%g-D%d" % (_sc(sc), os_, D), kind="scales", scales=sc, obs=os_, D=D, seed=seed,
                                agent="ddpg" if (D == 6 and sc in (LAYER_SCALES[0], LAYER_SCALES[10])) else "actor"))
    for D in (6, 9):
        for kind in ("w2-row-ramp", "w2-col-ramp", "planted", "domain-edge", "coherent-live", "coherent-const"):
            seed += 1
            out.append(dict(id="%s-D%d" % (kind, D), kind=kind, scales=(1.0, 1.0, 1.0), obs=1.0, D=D, seed=seed, agent="actor"))
    for kind in ("coherent-live", "coherent-const"):
        seed += 1
        out.append(dict(id="ddpg-%s-D6" % kind, kind=kind, scales=(1.0, 1.0, 1.0), obs=1.0, D=6, seed=seed, agent="ddpg"))
    return out


def _four_cases():
    out, seed = [], 500
    for agent in ("datd3", "darc", "daddpg"):
        kinds = [("scales", (1.0, 1.0, 1.0), 1.0), ("scales", (1.0, 2.0 ** -4, 2.0 ** 4), 1.0), ("scales", (2.0 ** 4, 2.0 ** -8, 2.0 ** 4), 1.0),
                 ("w2-row-ramp", (1.0, 1.0, 1.0), 30.0), ("w2-col-ramp", (1.0, 1.0, 1.0), 1.0), ("planted", (1.0, 1.0, 1.0), 1.0),
                 ("coherent-live", None, 1.0), ("coherent-const", None, 1.0)]
        kinds.append(("identical-actors", (1.0, 1.0, 1.0), 1.0) if agent == "daddpg" else ("twin", (1.0, 1.0, 1.0), 1.0))
        for i, (kind, sc, os_) in enumerate(kinds):
            for D in ((6, 9) if kind in ("scales",) and i == 0 else ((6, 9)[i % 2],)):
                seed += 1
                tag = kind if kind != "scales" else "scale-%s-obs%g" % (_sc(sc), os_)
                out.append(dict(id="%s-%s-D%d" % (agent, tag, D), kind=kind, scales=sc, obs=os_, D=D, seed=seed, agent=agent))
    return out


SINGLE = _single_cases()
FOUR = _four_cases()
BOUND = 0.7


def by_id(cid):
    return next(c for c in SINGLE + FOUR if c["id"] == cid)


def _shape_net(rng, c, net, x, rows):
    kind = c["kind"]
    if kind == "w2-row-ramp":
        net["fc2.weight"] = net["fc2.weight"] * rng.permutation(ramp())[:, None]
    elif kind == "w2-col-ramp":
        net["fc2.weight"] = net["fc2.weight"] * rng.permutation(ramp())[None, :]
    elif kind == "planted":
        plant_boundaries(rng, net, big=rows == 3 and c["agent"] in ("actor", "ddpg"))
    elif kind == "domain-edge":
        domain_edge(net, x, BOUND)
    return net


def _one_net(rng, c, x, rows, one_sign=False):
    """a net of case c for inputs x ([n, D] for an actor, [n, D + 3] for a critic); one_sign: see _four_try"""
    D = x.shape[1]
    if c["kind"].startswith("coherent"):
        # the critics' lo parts have the other sign, so that a lo table read from another net of the four is a coherent error
        return coherent_net(rng, D, rows, 1.0 if c["kind"] == "coherent-live" else 0.25, +1 if rows == 3 else -1)
    net = mlp(rng, D, rows, c["scales"])
    if one_sign:
        net["fc2.weight"] = np.abs(net["fc2.weight"])
        net["fc3.weight"] = np.abs(net["fc3.weight"]) * rng.choice(F([-1, 1]), (rows, 1))
    return _shape_net(rng, c, net, x, rows)


def _critic(rng, c, xa):
    """A critic of a four-net case: the action columns of fc1 are scaled by ACTION_GAIN so that two different proposals are valued
    differently (DADDPG's one critic sees nothing else)."""
    net = _one_net(rng, c, xa, 1, True)
    net["fc1.weight"][:, -3:] *= F(ACTION_GAIN)
    return net


ACTION_GAIN = 4.0


@functools.lru_cache(maxsize=None)
def single(cid):
    """dict(net, x, bound, ref (forward64), b32, b16 (bound dicts with out, h1, h2, z)) of a single-net case"""
    c = by_id(cid)
    rng = np.random.default_rng(c["seed"])
    D = c["D"]
    coh = c["kind"].startswith("coherent")
    x = coherent_obs(rng, N, D) if coh else observations(rng, N, D, c["obs"])
    if c["kind"] == "planted":
        x[:, 0] = np.clip(x[:, 0], -0.4, 0.4)                   # under the 65504 of W1[50][0]
    net = fit(_one_net(rng, c, x, 3), x, BOUND)
    b16 = R.bound_f16x3(net, x, BOUND, full=True)
    return dict(net=net, x=x, bound=BOUND, ref=b16["ref"], b32=R.bound_f32(net, x, BOUND, full=True), b16=b16)


def _four_try(c, seed, n=N):
    """The bounds are worst-case sums over |w| |x| carried through |W2| and |W3| of two nets in a row, so a pick is clear only where
    q1 - q2 is large against those sums, not against |q|: with fc2 and fc3 of mixed signs (256 cancelling terms each) every row of
    every scale is ambiguous.  The nets of the four-net cases therefore have fc2 >= 0 and one sign per fc3 row (`one_sign`): the
    scales, ramps and planted values are the single-net cases', without the cancellation."""
    rng = np.random.default_rng(seed)
    D, kind = c["D"], c["kind"]
    coh = kind.startswith("coherent")
    x = coherent_obs(rng, n, D) if coh else observations(rng, n, D, c["obs"])
    if kind == "planted":
        x[:, 0] = np.clip(x[:, 0], -0.4, 0.4)
    a1 = fit(_one_net(rng, c, x, 3, True), x, BOUND)
    a2 = {k: v.copy() for k, v in a1.items()} if kind == "identical-actors" else fit(_one_net(rng, c, x, 3, True), x, BOUND)
    xa = np.concatenate([x, R.forward64(a1, x, BOUND, False)["out"].astype(F)], 1)
    c1 = _critic(rng, c, xa)
    if c["agent"] == "daddpg":
        c2 = c1                                                  # the same object: one critic values both proposals
    elif kind == "twin":
        c2 = {k: (v * (1 + 0.02 * rng.standard_normal(v.shape))).astype(F) for k, v in c1.items()}
    else:
        c2 = _critic(rng, c, xa)
    nets = (a1, a2, c1, c2)
    if c2 is not c1:                                             # balance the picks: q2 += median(q1 - q2)
        t = R.take_action64(nets, x, BOUND)
        c2["fc3.bias"] = (c2["fc3.bias"] + F(np.median(t["q1"] - t["q2"]))).astype(F)
    return nets, x


def four_conditions(b):
    """(share of ambiguous rows, share of the rarer pick among the clear rows)"""
    clear = R.clear_rows(b)
    p = b["ref"]["picked"][clear]
    return 1.0 - clear.mean(), (min(p.mean(), 1 - p.mean()) if p.size else 0.0)


def _four_build(c, n=N):
    for attempt in range(12):
        nets, x = _four_try(c, c["seed"] + 1000 * attempt, n)
        b = R.bound_take_action(nets, x, BOUND)
        amb, rare = four_conditions(b)
        if c["kind"] == "identical-actors" or (amb <= AMB_MAX and rare >= PICK_MIN):
            break
    return dict(nets=nets, x=x, bound=BOUND, b=b, attempts=attempt + 1)


@functools.lru_cache(maxsize=None)
def four(cid):
    """dict(nets (actor1, actor2, critic1, critic2), x, bound, b (bound_take_action, reference under b["ref"])) of a four-net case"""
    return _four_build(by_id(cid))


def mixed_single(D, n, seed=900):
    """the mixed-scale net (large W1, small W2, large W3; fc3 fitted) on n observations with dominated and zero rows"""
    rng = np.random.default_rng(seed + D)
    x = observations(rng, n, D, 1.0)
    return fit(mlp(rng, D, 3, MIXED), x, BOUND), x


@functools.lru_cache(maxsize=None)
def mixed_four(D, n, shared_critic):
    """the four-net case of the mixed scales on n rows (as four(): nets, x, bound, b)"""
    return _four_build(dict(kind="scales", scales=MIXED, obs=1.0, D=D, seed=950 + D, agent="daddpg" if shared_critic else "datd3"), n)
