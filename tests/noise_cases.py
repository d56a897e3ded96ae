"""The cases of tests/test_noise_ref.py and tests/test_gpu_noise_ref.py (test infrastructure): keys of the exploration noise
(tests/noise_ref.py) at which the f32 Box-Muller of csrc/armenv_env.h policy_noise can go wrong.

PLANTED EDGE KEYS (tests/golden/noise_edge_keys.npz, found by tests/tools/gen_noise_edge_keys.py).  A Philox word falls into one of
the classes below with probability 2^-23 .. 2^-25, so no random block ever draws one; the fixture holds tuples (env index, episode
index, step) at the fixed EDGE_SEED and EDGE_OFFSET -- both past 2^32 -- whose words do, at least two per class for the (w0, w1)
pair ("a": z0, z1) and for the (w2, w3) pair ("b": z2).  Every tuple can be planted through set_state(episode = index + 1, step =).

  rad-one          radius word >= 0xFFFFFF80: (float)w + 1 rounds to 2^32, u = 1.0, r = sqrt(-0): the draw must be +-0, not NaN
  rad-below-one    the last f32 step below that: u = 1 - 2^-24, r = 3.45e-4 (log2 next to 1)
  rad-tail         radius word < 2^8: the deep tail, |z| up to 6.66
  ang-one          angle word >= 0xFFFFFF80: u = 1.0, the quadrant k = 4
  ang-zero         angle word < 2^8
  ang-sign-{1,2,3} angle word within 2^8 of k 2^30: the sign changes of cos and sin
  ang-tie-{1,3,5,7} angle word within 2^8 of k 2^29: the rounding ties of the quadrant, |x| = pi / 4

RANDOM BLOCKS.  64 envs x 32 steps at each keying of BLOCKS: the existing parity test's (seed 21, offset 5), a seed with a high word, a
seed past 2^63, global ids across 2^32, and episode counters that wrap (counter 0xFFFFFFFF = running index 0xFFFFFFFE; the next
reset gives counter 0 and index 0xFFFFFFFF; the one after, counter 1 and index 0)."""
import functools
import os

import numpy as np

import noise_ref as NR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_edge_keys.npz")

EDGE_SEED = 2 ** 32 + 5
EDGE_OFFSET = 2 ** 32 - 32          # env indices 0..31 below 2^32, 32..63 at and above it
EDGE_ENVS = 64
EDGE_STEPS = 1024                   # step < 1024: handles that plant them need max_steps above it
NEAR = 2 ** 8
TOP = 0xFFFFFF80

KINDS = (["rad-one", "rad-below-one", "rad-tail", "ang-one", "ang-zero"] + ["ang-sign-%d" % k for k in (1, 2, 3)] +
         ["ang-tie-%d" % k for k in (1, 3, 5, 7)])
CLASSES = ["%s:%s" % (p, k) for p in ("a", "b") for k in KINDS]
MIN_PER_CLASS = 2


def classify(w):
    """bool [n, len(CLASSES)]: which classes the words w (uint64 [n, 4]) fall into"""
    w = np.asarray(w, dtype=np.int64)
    u = NR.uniforms(w)
    cols = []
    for rad, ang in ((0, 1), (2, 3)):
        r, a = w[:, rad], w[:, ang]
        cols += [r >= TOP, u[:, rad] == np.float32(1.0 - 2.0 ** -24), r < NEAR, a >= TOP, a < NEAR]
        cols += [np.abs(a - k * 2 ** 30) < NEAR for k in (1, 2, 3)]
        cols += [np.abs(a - k * 2 ** 29) < NEAR for k in (1, 3, 5, 7)]
    return np.stack(cols, -1)


@functools.lru_cache(maxsize=None)
def edge_keys():
    """dict(seed, offset, env, episode, step (int64 [m]), cls (index into CLASSES, [m]), names) of the committed fixture"""
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    return dict(seed=int(d["seed"]), offset=int(d["env_id_offset"]), env=d["env"].astype(np.int64),
                episode=d["episode_index"].astype(np.int64), step=d["step"].astype(np.int64), cls=d["cls"].astype(np.int64),
                names=[str(s) for s in d["class_names"]])


def edge_words(k=None):
    k = k or edge_keys()
    return NR.words(k["seed"], np.uint64(k["offset"]) + k["env"].astype(np.uint64), k["episode"], k["step"])


def edge_launches(k=None):
    """The distinct tuples of the fixture as launches of one EDGE_ENVS-env handle: a list of (episode counter u32 [64], step i32 [64],
    rows: indices into the fixture's tuples or -1).  An env without a tuple in a launch sits at counter 1, step 0."""
    k = k or edge_keys()
    out, placed = [], {}
    for j in range(len(k["env"])):
        key = (int(k["env"][j]), int(k["episode"][j]), int(k["step"][j]))
        if key in placed:
            continue
        li = 0
        while li < len(out) and out[li][2][key[0]] >= 0:
            li += 1
        if li == len(out):
            out.append((np.ones(EDGE_ENVS, dtype=np.uint32), np.zeros(EDGE_ENVS, dtype=np.int32), np.full(EDGE_ENVS, -1, dtype=np.int64)))
        out[li][0][key[0]] = (key[1] + 1) & 0xFFFFFFFF
        out[li][1][key[0]] = key[2]
        out[li][2][key[0]] = j
        placed[key] = li
    return out


# ---- random blocks ----

BLOCK_ENVS, BLOCK_STEPS = 64, 32
BLOCKS = (
    dict(id="seed21-offset5", seed=21, offset=5, counter=1),
    dict(id="seed-high-word", seed=2 ** 32 + 5, offset=0, counter=1),
    dict(id="seed-past-2^63", seed=2 ** 63 + 0x1234567, offset=1234, counter=7),
    dict(id="ids-across-2^32", seed=9, offset=2 ** 32 - 32, counter=3),
    dict(id="counter-wraps", seed=2 ** 63 + 11, offset=2 ** 32 - 32, counter=0xFFFFFFFF),
    dict(id="counter-zero", seed=2 ** 32 + 5, offset=2 ** 32 - 32, counter=0),
)


def block(bid):
    return next(b for b in BLOCKS if b["id"] == bid)


def block_keys(b, n=BLOCK_ENVS, steps=BLOCK_STEPS, done=None, step0=0):
    """(ids uint64 [steps, n], episode index [steps, n], step [steps, n]) of a block that starts at episode counter b["counter"] and
    step counter step0 on every env.  done (bool [steps, n], optional): the rollout's done flags -- an env that finished at row t
    was reset in place, so row t + 1 has the next episode and step 0.  Without it no env finishes."""
    ids = np.broadcast_to(np.uint64(b["offset"]) + np.arange(n, dtype=np.uint64), (steps, n))
    ep = np.zeros((steps, n), dtype=np.int64); sp = np.zeros((steps, n), dtype=np.int64)
    c, s = np.full(n, b["counter"], dtype=np.int64), np.full(n, step0, dtype=np.int64)
    for t in range(steps):
        ep[t], sp[t] = (c - 1) & 0xFFFFFFFF, s
        d = done[t] if done is not None else np.zeros(n, dtype=bool)
        c, s = np.where(d, (c + 1) & 0xFFFFFFFF, c), np.where(d, 0, s + 1)
    return ids, ep, sp


def block_reference(b, **kw):
    """(ref float64 [steps, n, 3], bound [steps, n, 3]) of block_keys(b, **kw)"""
    ids, ep, sp = block_keys(b, **kw)
    w = NR.words(b["seed"], ids, ep, sp)
    return NR.reference(w).reshape(ids.shape + (3,)), NR.bound(w).reshape(ids.shape + (3,))


# ---- the stream of the distribution test ----

STREAM = dict(seed=2 ** 32 + 5, offset=2 ** 32 - 2048, episode=0xFFFFFFFF, envs=4096, steps=128)
