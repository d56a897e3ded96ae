"""What the DATD3 / DARC tests share: loading the training fixtures G17 / G18 (tests/golden/gen_datd3_fixtures.py writes each as
three files under the repository's size limit) and their comparison rule."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETS = ("actor1", "actor2", "critic1", "critic2", "target_actor1", "target_actor2", "target_critic1", "target_critic2")
KEYS = ("states", "actions", "next_states", "rewards", "dones")


def load_train_fixture(name):
    """one dict over the three files of `name` (datd3_train_seed0 / darc_train_seed0)"""
    g = {}
    for suffix in ("", "_b", "_c"):
        with np.load(os.path.join(GOLDEN, name + suffix + ".npz")) as z:
            g.update({k: z[k] for k in z.files})
    assert all(f"{n}__fc1_weight" in g for n in NETS), sorted(g)
    return g


def expected_losses(g, darc, w=0.005):
    """the stepped critic's loss of each of the eight updates, from the recorded F.mse_loss values, in the reference's arithmetic
    (DARC: mse + w * mse, the product in f32 as torch's scalar multiply rounds it)"""
    m = g["mse"]
    if not darc:
        return [float(x) for x in m]
    return [float(np.float32(a) + np.float32(w) * np.float32(b)) for a, b in m]


def batch(g, i):
    import torch
    return {k: torch.from_numpy(g[f"b{i}_{k}"]) for k in KEYS}
