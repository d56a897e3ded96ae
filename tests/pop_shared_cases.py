"""What the tests of the shared population sampler (armenv_her_pop_sample_shared, include/armenv.h) share (test infrastructure; no
device is needed): the draw rule restated in numpy over her_cases.philox_uniforms and one more Philox block for u4, the concatenation
model it is held against (the single sampler's picks over the members' episode lists laid end to end), and the seeds, draws and
store geometry of the GPU tests together with the conditions these must satisfy, so that a seed is chosen on the CPU.

A pick of the shared sampler is (member, episode within that member, step_state, use_her, step_goal); the inert row's is INERT."""
import numpy as np

from her_cases import KEY_XOR, M32, M64, philox_uniforms, picks_from_uniforms

INERT = (-1, -1, 0, 0, 0)
# the GPU tests' store: tests/test_gpu_pop_store.py's rings (_member_host), a full window that wraps, starting mid-episode
SEED, DRAWS, CAP, T, BASE, AT_RESET, HER_RATIO = 7, (0, 1), 40, 40, 31, 0, 0.8
EDGE_RATIOS = (2.0 ** -53, 1.0 - 2.0 ** -53)


def u4_uniforms(seed, draw, B):
    """u4 f64 [B] of rows 0..B-1: the u53 of words (0, 1) of the Philox block with fourth counter word 2, key and the other counter
    words as her_cases.philox_uniforms has them"""
    from learner_ref64 import philox4x32_10
    k = (int(seed) ^ KEY_XOR) & M64
    b = np.arange(B, dtype=np.uint64)
    key = np.broadcast_to(np.array([k & M32, k >> 32], np.uint64), (B, 2))
    ctr = np.stack([b & np.uint64(M32), b >> np.uint64(32), np.full_like(b, int(draw) & M32), np.full_like(b, 2)], -1)
    w = philox4x32_10(ctr, key)
    return (((w[:, 0] << np.uint64(32)) | w[:, 1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def shared_mask(seed, draw, P, B, share_ratio):
    """bool [P][B]: the rows that the rule draws from the union (u4 < share_ratio, member p's u4 under seed + p)"""
    return np.stack([u4_uniforms((seed + p) & M64, draw, B) < share_ratio for p in range(P)])


def model_picks(seed, draw, B, lists, her_ratio, use_her, share_ratio):
    """The draw rule, written out row by row: picks i32 [P][B][5] for the members' episode lists `lists` ([E_p][3] each)."""
    P = len(lists)
    counts = [len(e) for e in lists]
    total = sum(counts)
    out = np.zeros((P, B, 5), np.int32)
    for p in range(P):
        u = philox_uniforms((seed + p) & M64, draw, B)
        u4 = u4_uniforms((seed + p) & M64, draw, B)
        for b in range(B):
            if u4[b] < share_ratio:
                if total == 0:
                    out[p, b] = INERT
                    continue
                g, m, before = int(u[0, b] * np.float64(total)), 0, 0
                while not g < before + counts[m]:                 # the smallest m with g < E_0 + ... + E_m
                    before += counts[m]
                    m += 1
                ep = g - before
            else:
                if counts[p] == 0:
                    out[p, b] = INERT
                    continue
                m, ep = p, int(np.int32(u[0, b] * np.float64(counts[p])))
            L = int(lists[m][ep, 2])
            st = int(u[1, b] * np.float64(L))
            her = int(bool(use_her) and u[2, b] <= her_ratio)
            sg = st + 1 + int(u[3, b] * np.float64(L - st))
            out[p, b] = (m, ep, st, her, sg)
    return out


def split_picks(picks4, lists):
    """the single sampler's picks [B][4] over the concatenation of `lists` as shared picks [B][5]: (member, episode within it, ...)"""
    ends = np.cumsum([len(e) for e in lists])
    m = np.searchsorted(ends, picks4[:, 0], side="right")
    before = np.concatenate([[0], ends])[m]
    return np.concatenate([m[:, None], (picks4[:, 0] - before)[:, None], picks4[:, 1:]], -1).astype(np.int32)


def concatenation_picks(seed, draw, B, lists, her_ratio, use_her):
    """The concatenation model: member p's picks are the single sampler's (her_cases.picks_from_uniforms, seed + p) over all members'
    episode lists laid end to end -- random.sample(buffer, 1) over the joined buffer --, told apart by member again.  None if
    there is no episode at all."""
    joined = np.concatenate([np.asarray(e, np.int32).reshape(-1, 3) for e in lists])
    if len(joined) == 0:
        return None
    return np.stack([split_picks(picks_from_uniforms(philox_uniforms((seed + p) & M64, draw, B), joined, her_ratio, use_her), lists)
                     for p in range(len(lists))])


def own_picks(seed, draw, B, lists, her_ratio, use_her):
    """today's population sampler as shared picks: member p's single picks over its own list with p in front, INERT where it has none"""
    out = np.empty((len(lists), B, 5), np.int32)
    for p, eps in enumerate(lists):
        if len(eps) == 0:
            out[p] = INERT
        else:
            out[p, :, 0] = p
            out[p, :, 1:] = picks_from_uniforms(philox_uniforms((seed + p) & M64, draw, B), eps, her_ratio, use_her)
    return out


def gpu_store_lists(P, N, D, empty=()):
    """the episode lists of the GPU tests' store (oracle.her on the members' linear windows)"""
    from oracle import her
    from test_gpu_pop_store import _member_host
    return [her.index_episodes(_member_host(p, CAP, N, D, T, BASE, empty=p in empty)[1]["done"], starts_at_reset=bool(AT_RESET))
            for p in range(P)]
