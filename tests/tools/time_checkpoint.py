"""What a checkpoint costs at ``python -m armenv.train_pop``'s defaults (16 members, 64 envs each, window 1536), for td3 and datd3:
the wall time of one ``save_run``, of the whole checkpoint step (``state_dict()`` of every object, device to host, plus ``save_run``),
of one resume, and the file's size -- beside the time of one training iteration of the same run, so that ``checkpoint_every`` can be
chosen.  HOST CLOCK values (time.perf_counter around Python calls, the device synchronised before a reading), not device timers.

    python tests/tools/time_checkpoint.py [--out profiles/checkpoint_cost.json]

32 iterations, a checkpoint after every 8th.  ``iteration_s``: the median over iterations 26..32, which run their updates (the
stores are ready long before; ``iterations_with_updates`` says how many did); the interval of iteration 25 holds the checkpoint step of
iteration 24, so ``checkpoint_step_s`` is that interval minus ``iteration_s``.  ``resume_s``: a call that builds its objects, loads the
file of iteration 32 and has no iteration left to run; ``build_s``: the same call without ``resume`` and with ``iterations=0``."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "drl-on-robot-arm_amd"))

import torch  # noqa: E402

from armenv import checkpoint, train_pop  # noqa: E402

ITERATIONS, EVERY = 32, 8


def measure(algo, tmp):
    saves, walls = [], []

    def timed_save(path, state):
        t = time.perf_counter()
        checkpoint.save_run(path, state)
        saves.append(time.perf_counter() - t)

    def stamp(line):
        torch.cuda.synchronize()
        walls.append(time.perf_counter())

    train_pop.save_run = timed_save
    try:
        path = os.path.join(tmp, algo + ".ckpt")
        pop, _ = train_pop.train_reach_population(iterations=ITERATIONS, log_every=1, algo=algo, checkpoint=path, checkpoint_every=EVERY, log=stamp)
    finally:
        train_pop.save_run = checkpoint.save_run
    steps = [b - a for a, b in zip(walls, walls[1:])]              # steps[k]: the interval that ends with iteration k + 2
    late = steps[3 * EVERY:]                                        # iterations 26..32
    iteration_s = statistics.median(late)
    per_train = 2 if algo in ("datd3", "darc") else 1              # total_it counts updates: two per train for these agents
    torch.cuda.synchronize()
    t = time.perf_counter()
    train_pop.train_reach_population(iterations=ITERATIONS, log_every=1, algo=algo, resume=path, log=stamp)
    torch.cuda.synchronize()
    resume_s = time.perf_counter() - t
    t = time.perf_counter()
    train_pop.train_reach_population(iterations=0, algo=algo, log=stamp)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t
    return dict(file_bytes=os.path.getsize(path), save_run_s=statistics.median(saves), save_run_s_each=saves,
                checkpoint_step_s=steps[3 * EVERY - 1] - iteration_s, iteration_s=iteration_s, iteration_s_26_to_32=late,
                iterations_with_updates=pop.total_it // (40 * per_train), resume_s=resume_s, build_s=build_s,
                load_and_restore_s=resume_s - build_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_cost.json"))
    a = ap.parse_args()
    out = dict(what="cost of armenv.checkpoint at python -m armenv.train_pop's defaults: members 16, num_envs 64, rollout_steps 32, "
                    "updates 40, batch_size 256, window_steps 1536, store population; %d iterations, checkpoint_every %d" % (ITERATIONS, EVERY),
               clock="HOST clock: time.perf_counter() around Python calls, device synchronised before each reading; seconds",
               tool="tests/tools/time_checkpoint.py", device=torch.cuda.get_device_name(0), runs={})
    with tempfile.TemporaryDirectory() as tmp:
        for algo in ("td3", "datd3"):
            out["runs"][algo] = measure(algo, tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
