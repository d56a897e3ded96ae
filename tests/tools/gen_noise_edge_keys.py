#!/usr/bin/env python3
"""Search for the planted edge keys of the exploration-noise tests and write tests/golden/noise_edge_keys.npz.

At the fixed seed and env_id_offset of tests/noise_cases.py (EDGE_SEED, EDGE_OFFSET) every (env index < 64, episode index, step < 1024)
is enumerated in that order of (episode, env, step), episode by episode, through the project's own Philox (tests/noise_ref.py
words()), and the first KEEP tuples of each class of noise_cases.CLASSES are kept.  The rarest classes have probability 2^-25 per
word: EPISODES episodes are 3.0e8 blocks, 9 expected hits.  numpy runs about 2e6 blocks a second and core, so this takes minutes,
once; the result is a few hundred integers.  CPU only.

    python tests/tools/gen_noise_edge_keys.py [--out tests/golden/noise_edge_keys.npz] [--jobs 8]

The output does not depend on --jobs.  tests/test_noise_ref.py recomputes every tuple's words and asserts its class.
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import noise_cases as NC  # noqa: E402
import noise_ref as NR  # noqa: E402

EPISODES = 4608
CHUNK = 16          # episodes per work item
KEEP = 3


def scan(ep0):
    """hits of episodes ep0 .. ep0 + CHUNK - 1: int64 [m, 4] = (episode, env, step, class), sorted"""
    ep, env, step = np.meshgrid(np.arange(ep0, ep0 + CHUNK, dtype=np.int64), np.arange(NC.EDGE_ENVS, dtype=np.int64),
                                np.arange(NC.EDGE_STEPS, dtype=np.int64), indexing="ij")
    ep, env, step = ep.reshape(-1), env.reshape(-1), step.reshape(-1)
    w = NR.words(NC.EDGE_SEED, np.uint64(NC.EDGE_OFFSET) + env.astype(np.uint64), ep, step)
    # a cheap prefilter: every class has a word within 2^9 of a multiple of 2^29 (mod 2^32)
    m = (((w.astype(np.int64) + 512) & (2 ** 29 - 1)) < 1024).any(1)
    idx = np.nonzero(m)[0]
    rows, cls = np.nonzero(NC.classify(w[idx]))
    return np.stack([ep[idx[rows]], env[idx[rows]], step[idx[rows]], cls], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=NC.GOLDEN)
    ap.add_argument("--jobs", type=int, default=min(8, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    starts = list(range(0, EPISODES, CHUNK))
    if args.jobs > 1:
        with multiprocessing.Pool(args.jobs) as pool:
            parts = pool.map(scan, starts)            # in the order of `starts`
    else:
        parts = [scan(s) for s in starts]
    hits = np.concatenate(parts)
    keep = []
    for c in range(len(NC.CLASSES)):
        h = hits[hits[:, 3] == c][:KEEP]
        if len(h) < NC.MIN_PER_CLASS:
            raise SystemExit("class %s: %d tuples in %d episodes" % (NC.CLASSES[c], len(h), EPISODES))
        keep.append(h)
    keep = np.concatenate(keep)
    np.savez(args.out, seed=np.uint64(NC.EDGE_SEED), env_id_offset=np.uint64(NC.EDGE_OFFSET), env=keep[:, 1].astype(np.int32),
             episode_index=keep[:, 0].astype(np.int64), step=keep[:, 2].astype(np.int32), cls=keep[:, 3].astype(np.int32),
             class_names=np.array(NC.CLASSES))
    print("%d tuples, %d classes, all hits %d -> %s" % (len(keep), len(NC.CLASSES), len(hits), args.out))


if __name__ == "__main__":
    main()
