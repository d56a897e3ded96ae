#!/usr/bin/env python3
"""Generates the DATD3 / DARC training fixtures under tests/golden/ from the reference checkout (companion of gen_fixtures.py, same
rules: needs the reference at generation time only; what it writes is data -- inputs, recorded draws, recorded results).

  G17 datd3_train_seed0*.npz   four DATD3_MLP.train() calls = eight updates (algo/DATD3/DATD3_mlp.py:140-211) from
                               torch.manual_seed(0) construction (6, 3, 0.7) on np.random.default_rng(17) batches of 64 rows, with
                               torch.manual_seed(123) before the first train
  G18 darc_train_seed0*.npz    the same for DARC_MLP (algo/DARC/DARC_mlp.py:134-222) with default_rng(18)

Recorded: the four batches (b<i>_<key>), every torch.randn_like draw of the run (noise [8][64][3], one per update), every value
F.mse_loss returned (mse: DATD3 [8], DARC [8][2] = the target term and the regulariser's, in call order) and the final parameters of
all eight nets.  The reference's update returns nothing, so both are taken by wrapping the two torch functions in THIS process.

Eight nets of 68 k floats are 2.2 MB; no committed file may exceed 1 MiB, and four nets are 1.05 MiB, so each fixture is three files:
  <name>.npz        batches, noise, mse, actor1, actor2, critic1
  <name>_b.npz      critic2, target_actor1, target_actor2
  <name>_c.npz      target_critic1, target_critic2
tests read them through `load_train_fixture` in tests/datd3_golden.py."""
import os
import sys

import numpy as np

REF = os.environ.get("ARMENV_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
PARTS = (("", ("actor1", "actor2", "critic1")), ("_b", ("critic2", "target_actor1", "target_actor2")),
         ("_c", ("target_critic1", "target_critic2")))


def gen(module, cls_name, rng_seed, fname):
    sys.path.insert(0, REF)
    import importlib
    import torch
    import torch.nn.functional as F
    cls = getattr(importlib.import_module(module), cls_name)
    torch.manual_seed(0)
    agent = cls(6, 3, 0.7, device=torch.device("cpu"))
    rng = np.random.default_rng(rng_seed)
    B = 64
    batches = []
    for _ in range(4):
        st = rng.uniform(0.2, 0.6, (B, 6)).astype(np.float32)
        ns = st.copy(); ns[:, :3] += rng.normal(0, 0.01, (B, 3)).astype(np.float32)
        batches.append(dict(states=st, actions=rng.uniform(-0.7, 0.7, (B, 3)).astype(np.float32), next_states=ns,
                            rewards=rng.choice([-0.1, 1.0], B).astype(np.float32), dones=rng.integers(0, 2, B).astype(np.uint8)))
    noise, mse = [], []
    randn_like, mse_loss = torch.randn_like, F.mse_loss

    def rec_randn_like(x, *a, **kw):
        z = randn_like(x, *a, **kw)
        noise.append(z.detach().numpy().copy())
        return z

    def rec_mse_loss(*a, **kw):
        v = mse_loss(*a, **kw)
        mse.append(float(v.detach()))
        return v

    torch.randn_like, F.mse_loss = rec_randn_like, rec_mse_loss
    try:
        torch.manual_seed(123)
        for b in batches:
            agent.train({k: v.tolist() if k in ("rewards", "dones") else v for k, v in b.items()}, B)
    finally:
        torch.randn_like, F.mse_loss = randn_like, mse_loss
    assert len(noise) == 8 and len(mse) in (8, 16), (len(noise), len(mse))
    run = {"noise": np.stack(noise), "mse": np.array(mse).reshape(8, -1).squeeze()}
    for i, b in enumerate(batches):
        for k, v in b.items():
            run[f"b{i}_{k}"] = v
    for suffix, names in PARTS:
        out = dict(run) if suffix == "" else {}
        for name in names:
            for k, v in getattr(agent, name).state_dict().items():
                out[f"{name}__{k.replace('.', '_')}"] = v.detach().numpy().copy()
        path = os.path.join(OUT, fname + suffix + ".npz")
        np.savez(path, **out)
        assert os.path.getsize(path) < (1 << 20), path


if __name__ == "__main__":
    gen("algo.DATD3.DATD3_mlp", "DATD3_MLP", 17, "datd3_train_seed0")
    gen("algo.DARC.DARC_mlp", "DARC_MLP", 18, "darc_train_seed0")
    print("fixtures written to", OUT)
