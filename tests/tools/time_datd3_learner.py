#!/usr/bin/env python3
"""Milliseconds per UPDATE of the fused DATD3 and DARC updates (armenv_datd3_update, darc 0 / 1) against the fused DADDPG update
(armenv_daddpg_update: the same kernels and the same 16-stage chain, untouched code) at B in {256, 2048, 8192}, with the torch DATD3
and DARC learners replayed from their hipGraphs for context -- in one process, warmed up, five repeats with the learners
alternating, each repeat a device-synchronised host clock around 30 steps.  One step of a DATD3 / DARC learner is one `train` = TWO
updates (k = 1 then k = 2 on the batch), one step of DADDPG is one update; every row reports ms_per_update and, for the double-critic
agents, ms_per_train = 2 ms_per_update -- never compare a DATD3 train with a DADDPG update.  The last rows per B are the ratios
DATD3 update / DADDPG update and DARC update / DATD3 update, from the medians and from the extreme repeats (spread).
The protocol of time_daddpg_learner.py.

    python tests/tools/time_datd3_learner.py [--out profiles/datd3_fused_time_learner.json] [--batches 256,2048,8192]
    python tests/tools/time_datd3_learner.py --only fused_datd3 --batches 2048     # one learner alone (for rocprofv3 --stats)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "drl-on-robot-arm_amd")]
import torch  # noqa: E402

from armenv.datd3 import DARC, DATD3  # noqa: E402
from armenv.fused_daddpg import FusedDADDPG  # noqa: E402
from armenv.fused_datd3 import FusedDARC, FusedDATD3  # noqa: E402

F32_MATRIX_PEAK = 157.3e12     # MI355X, v_mfma_f32_*: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz
UPDATES_PER_STEP = dict(fused_daddpg=1, fused_datd3=2, fused_darc=2, torch_graphed_datd3=2, torch_graphed_darc=2)


def flop_per_update(B, D, darc, H=256, A=3):
    """DADDPG's count (time_daddpg_learner.py: the same problem list -- two target actors, two target-critic passes, one stepped critic,
    one stepped actor); DARC adds the other critic's forward over cat(s, a)."""
    K1 = D + A
    lin = lambda i, o: 2 * B * i * o
    mlp = lambda i, o: lin(i, H) + lin(H, H) + lin(H, o)
    critic = 2 * mlp(D, A) + 2 * mlp(K1, 1) + mlp(K1, 1) + lin(H, 1) + lin(H, H) + mlp(K1, 1)
    actor = mlp(D, A) + mlp(K1, 1) + lin(H, 1) + lin(H, H) + lin(K1, H) + lin(H, A) + lin(H, H) + mlp(D, A)
    return critic + actor + (mlp(K1, 1) if darc else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,2048,8192")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=sorted(UPDATES_PER_STEP))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    rows = []
    for B in [int(x) for x in a.batches.split(",")]:
        torch.manual_seed(0)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        batch = dict(states=torch.rand(B, 6, device=dev, generator=gen), actions=torch.rand(B, 3, device=dev, generator=gen) - 0.5,
                     next_states=torch.rand(B, 6, device=dev, generator=gen), rewards=torch.rand(B, device=dev, generator=gen),
                     dones=(torch.rand(B, device=dev, generator=gen) < 0.1).to(torch.uint8))
        keep, step = [], {}

        def fused(cls):
            f = cls(6, 3, 0.7, device=dev)
            buf = f.batch_buffers(B)
            for k, v in buf.items():
                v.copy_(batch[k])
            keep.append((f, buf))
            return lambda: f.train(buf)

        def graphed(cls):
            t = cls(6, 3, 0.7, device=dev)
            static = t.capture(B)
            for k, v in static.items():
                v.copy_(batch[k])
            keep.append((t, static))
            return lambda: t.train_graphed(static)

        makers = dict(fused_daddpg=lambda: fused(FusedDADDPG), fused_datd3=lambda: fused(FusedDATD3), fused_darc=lambda: fused(FusedDARC),
                      torch_graphed_datd3=lambda: graphed(DATD3), torch_graphed_darc=lambda: graphed(DARC))
        for name, mk in makers.items():
            if a.only in (None, name):
                step[name] = mk()
        for name, fn in step.items():            # warm-up: allocations, optimiser state, code objects, clocks
            for _ in range(12):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in step}            # ms per UPDATE
        for _ in range(a.repeats):
            for name, fn in step.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / (a.steps * UPDATES_PER_STEP[name]))
        for name, ts in times.items():
            med, n = statistics.median(ts), UPDATES_PER_STEP[name]
            fl = flop_per_update(B, 6, name.endswith("darc"))
            rec = dict(batch=B, learner=name, ms_per_update=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                       updates_per_step=n, repeats=a.repeats, steps_per_repeat=a.steps, gflop_per_update=round(fl / 1e9, 4),
                       tflops=round(fl / (med * 1e-3) / 1e12, 3), share_of_f32_matrix_peak=round(fl / (med * 1e-3) / F32_MATRIX_PEAK, 5))
            if n == 2:
                rec["ms_per_train"] = round(2 * med, 4)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        for num, den in (("fused_datd3", "fused_daddpg"), ("fused_darc", "fused_datd3"), ("fused_datd3", "torch_graphed_datd3"),
                         ("fused_darc", "torch_graphed_darc")):
            if num in times and den in times:
                x, y = times[num], times[den]
                rec = dict(batch=B, update_of=num, over_update_of=den, ratio=round(statistics.median(x) / statistics.median(y), 3),
                           ratio_min=round(min(x) / max(y), 3), ratio_max=round(max(x) / min(y), 3))
                rows.append(rec)
                print(json.dumps(rec), flush=True)
        del keep, step
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
