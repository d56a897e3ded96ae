"""On-device training loop: the reference's ``run()`` (/root/reference/main.py:77-162) with its four stages kept on the
GPU -- fused-policy rollouts (armenv_rollout), trajectory store + HER batches (armenv_her_sample), the agent's updates (torch),
success accounting (armenv_counters).  One iteration = `rollout_steps` env steps of `num_envs` envs followed by
`updates` updates; the reference does 40 updates of 256 samples after every (<= 501-step) episode of its single env.
The agent: `--algo td3` (train_reach_with_TD3's, main.py:165-231) or `--algo daddpg` -- opt.algo's default, what `run()` itself
instantiates (config.py:33, main.py:93): two actors and one critic, take_action fused into the rollout kernel; or `--algo datd3` /
`--algo darc` -- two actors AND two critics (armenv.datd3), whose one loop "update" is one `train` = two reference updates on the
batch, as the reference's run() counts them.

    python -m armenv.train --iterations 200
    python -m armenv.train --iterations 200 --algo daddpg
    python -m armenv.train --iterations 200 --learner hip      # the fused HIP TD3 update (armenv.fused_td3)
    python -m armenv.train --iterations 200 --algo daddpg --learner fused    # the agent's own fused HIP update (armenv.fused_daddpg)
    python -m armenv.train --iterations 200 --algo datd3 --learner fused     # ... armenv.fused_datd3 (also --algo darc)
    python -m armenv.train --iterations 100 --learner fused --checkpoint run.ckpt --checkpoint-every 20 --save agent --save-best
    python -m armenv.train --iterations 200 --learner fused --resume run.ckpt --checkpoint run.ckpt      # the same bits as 200 in one go

``save`` / ``save_best``: the trained agent in the reference's files (armenv.checkpoint.save_agent; main.py:148-154 saves at every
best success rate).  ``checkpoint`` / ``checkpoint_every`` / ``resume``: the whole run's state -- learner, store, env, the loop's
variables -- in one file, written after every ``checkpoint_every``-th iteration and after the last; a resumed run (``resume=``, every
other argument but ``iterations``, ``log_every`` and the paths as in the saved one) continues at the next iteration and equals the
uninterrupted run bit for bit.  For the fused learners: the torch learner's noise comes from torch's device generator.
"""
import argparse
import json
import time

import torch

from . import envs
from .checkpoint import (BestKeeper, add_cli_arguments, check_cli_arguments, check_config, check_loop_arguments, checkpoint_due, load_run,
                         save_agent, save_run, to_cpu)
from .replay import TrajectoryStore
from .daddpg import DADDPG
from .datd3 import DARC, DATD3
from .fused_daddpg import FusedDADDPG
from .fused_datd3 import FusedDARC, FusedDATD3
from .fused_td3 import FusedTD3
from .td3 import TD3


ALGOS = ("td3", "daddpg", "datd3", "darc")
_TORCH = dict(td3=TD3, daddpg=DADDPG, datd3=DATD3, darc=DARC)
# --task: the environment, its state_dim and the action bound (main.py:87, :455-457); armenv.train_pop reads it too
_TASKS = dict(reach=(envs.BatchedReachEnv, 6, 0.7), push=(envs.BatchedPushEnv, 9, 0.4), pick=(envs.BatchedPickEnv, 9, 0.4))


def _check_learner(algo, learner):
    if algo not in ALGOS:
        raise ValueError("algo must be one of %s" % ", ".join(ALGOS))
    if learner not in ("torch", "hip", "fused"):
        raise ValueError("learner must be 'torch', 'hip' or 'fused'")
    if learner == "hip" and algo != "td3":
        raise ValueError("learner='hip' is the fused TD3 update: it needs algo='td3' (learner='fused' is the agent's own fused update)")


def _make_agent(algo, learner, state_dim, action_bound, device, batch_size, use_graphs, seed):
    """(agent, static input buffers or None, whether the updates are replayed from hipGraphs)"""
    if learner in ("hip", "fused"):       # "hip": FusedTD3 (td3 only); "fused": the agent's own fused update
        if algo == "daddpg":
            agent = FusedDADDPG(state_dim, 3, action_bound, device=device)
        elif algo in ("datd3", "darc"):
            agent = (FusedDARC if algo == "darc" else FusedDATD3)(state_dim, 3, action_bound, device=device, seed=seed)
        else:
            agent = FusedTD3(state_dim, 3, action_bound, device=device, seed=seed)
        return agent, agent.batch_buffers(batch_size), False
    agent = _TORCH[algo](state_dim, 3, action_bound, device=device)   # getattr(algo, opt.algo)(...)
    static = agent.capture(batch_size) if use_graphs else None     # TD3 update as hipGraphs: launch-bound otherwise
    return agent, static, use_graphs


def _install_policy(env, algo, agent, actor_kind, action_bound, sigma, clip):
    """take_action + exploration noise of `agent` (a learner, or a member of a population) as the fused policy of `env`'s rollouts
    (main.py:114-124): TD3's actor as `actor_kind`, the two-actor agents' own take_action"""
    if algo == "td3":
        env.set_policy(actor_kind, action_bound=action_bound, noise_sigma=sigma, noise_clip=clip, actor_state_dict=agent.actor_state_dict())
    else:
        install = dict(daddpg=env.set_policy_daddpg, datd3=env.set_policy_datd3, darc=env.set_policy_darc)[algo]
        install(*agent.policy_state_dicts(), action_bound=action_bound, noise_sigma=sigma, noise_clip=clip)


def _train(task, sigma, clip, num_envs, iterations, rollout_steps, updates, batch_size, her_ratio, seed, device,
           actor_kind, log_every, log, window_steps, minimal_episodes, max_steps, use_graphs, algo, learner,
           checkpoint=None, checkpoint_every=0, resume=None, save=None, save_best=False):
    """The loop behind train_reach and train_push: a task's environment class, state_dim and action_bound (a row of ``_TASKS``) and its
    exploration noise N(0, sigma) clipped at `clip`."""
    Env, state_dim, action_bound = _TASKS[task]
    _check_learner(algo, learner)
    check_loop_arguments(learner, checkpoint, checkpoint_every, resume, save, save_best)
    # every argument that shapes the run: a resumed run must repeat them (checked before anything is created on the device)
    config = dict(task=task, algo=algo, learner=learner, num_envs=num_envs, rollout_steps=rollout_steps, updates=updates,
                  batch_size=batch_size, her_ratio=her_ratio, seed=seed, actor_kind=actor_kind, expl_sigma=sigma, window_steps=window_steps,
                  minimal_episodes=minimal_episodes, max_steps=max_steps)
    saved = None
    if resume is not None:
        saved = load_run(resume)
        check_config(saved["config"], config)
    torch.manual_seed(seed)
    env = Env(num_envs, device=device, seed=seed, max_steps=max_steps)
    agent, static, use_graphs = _make_agent(algo, learner, state_dim, action_bound, device, batch_size, use_graphs, seed)  # main.py:93
    store = TrajectoryStore(device=device, seed=seed, capacity_steps=window_steps)   # last `window_steps` steps of every env
    obs = env.reset()
    history, bufs = [], {}
    c_prev = env.counters()
    best = BestKeeper(save) if save_best else None
    first, wall0 = 0, 0.0
    if saved is not None:          # continue at iteration saved + 1 with the saved run's objects and variables
        agent.load_state_dict(saved["agent"])
        store.load_state_dict(saved["store"])
        env.load_state_dict(saved["env"])
        obs, history, c_prev = saved["obs"].to(env.device), saved["history"], saved["c_prev"]
        first, wall0 = saved["iteration"], saved["wall_s"]
        if best and saved["best"] is not None:
            best.load_state_dict(saved["best"])
    t0 = time.perf_counter()
    for it in range(first, iterations):
        _install_policy(env, algo, agent, actor_kind, action_bound, sigma, clip)
        obs0 = obs.clone()
        out = env.rollout(rollout_steps, None, out=bufs, want_actions=True, want_terminal_obs=True)
        obs = out["obs"][-1]
        store.add_rollout(obs0, out, starts_at_reset=(it == 0))    # traj.store_step / add_trajectory (main.py:128-129)
        # replay_buffer.size() >= minimal_episodes (main.py:135), re-checked every iteration: the ring window can lose its
        # complete episodes again, and the sampler then returns inert all-zero batches that must not be trained on
        if store.size() >= minimal_episodes:
            for _ in range(updates):                              # main.py:136-138
                if use_graphs:     # HER batch written straight into the captured update's static buffers
                    agent.train_graphed(store.sample(batch_size, use_her=True, her_ratio=her_ratio, out=static))
                elif static is not None:     # fused learner: HER batch written into its static input buffers
                    agent.train(store.sample(batch_size, use_her=True, her_ratio=her_ratio, out=static))
                else:
                    agent.train(store.sample(batch_size, use_her=True, her_ratio=her_ratio))
        if (it + 1) % log_every == 0:
            c = env.counters()
            ep = c["episodes"] - c_prev["episodes"]
            rate = (c["successes"] - c_prev["successes"]) / max(1, ep)
            c_prev = c
            rec = dict(iteration=it + 1, env_steps=c["env_steps"], episodes=c["episodes"], success_rate=rate,
                       wall_s=wall0 + (time.perf_counter() - t0))
            history.append(rec)
            log(json.dumps(rec))
            if best:               # main.py:151-153
                best.offer(rate, agent)
        if checkpoint_due(it + 1, iterations, checkpoint, checkpoint_every):
            save_run(checkpoint, dict(config=config, iteration=it + 1, agent=agent.state_dict(), store=store.state_dict(),
                                      env=env.state_dict(), obs=to_cpu(obs), history=history, c_prev=c_prev,
                                      wall_s=wall0 + (time.perf_counter() - t0), best=best.state_dict() if best else None))
    if save is not None:
        save_agent(agent, save)
    env.close()
    return agent, history


def train_reach(num_envs=1024, iterations=200, rollout_steps=32, updates=48, batch_size=2048, her_ratio=0.8, seed=0,
                device="cuda:0", actor_kind="actor_f16x3", expl_sigma=0.7 * 0.98, log_every=10, log=print,
                window_steps=1536, minimal_episodes=5, max_steps=500, use_graphs=True, algo="td3", learner="torch",
                checkpoint=None, checkpoint_every=0, resume=None, save=None, save_best=False):
    # learner="hip": the TD3 update is libarmenv's fused one (armenv.fused_td3.FusedTD3), issued directly: no capture, no graph.
    # learner="fused": the agent's own fused update -- FusedTD3 for td3, armenv.fused_daddpg.FusedDADDPG for daddpg,
    # armenv.fused_datd3.FusedDATD3 / FusedDARC for datd3 / darc.
    # use_graphs: the agent's update replayed from hipGraphs (GraphedLearner.capture): the update is ~130 small kernels, launch-bound
    # when issued one by one (160 iterations: 7 s against 14 s).  Round 6 found the replayed updates no longer learning and why: a
    # hipMemsetAsync captured into a hipGraph works on the first replay only on this ROCm build, torch's multi-block reductions
    # initialise their semaphores with one, so every captured bias gradient went wrong from the second replay on.  The captured update
    # now contains no such reduction (armenv.td3._CaptureSafeLinear; profiles/r06_td3_hipgraph_learning.txt) and learns like the eager one.
    # Exploration noise N(0, expl_sigma) clipped at the action bound, 0.7.
    # checkpoint, checkpoint_every, resume, save, save_best: the module's docstring.
    action_bound = _TASKS["reach"][2]
    return _train("reach", expl_sigma, action_bound, num_envs, iterations, rollout_steps, updates, batch_size,
                  her_ratio, seed, device, actor_kind, log_every, log, window_steps, minimal_episodes, max_steps, use_graphs, algo, learner,
                  checkpoint, checkpoint_every, resume, save, save_best)


def train_push(num_envs=1024, iterations=300, rollout_steps=32, updates=48, batch_size=2048, her_ratio=0.8, seed=0,
               device="cuda:0", actor_kind="actor_f16x3", log_every=10, log=print, window_steps=1536, minimal_episodes=5,
               max_steps=500, task="push", use_graphs=True, algo="td3", learner="torch",
               checkpoint=None, checkpoint_every=0, resume=None, save=None, save_best=False):
    """``train_push_with_TD3`` (/root/reference/main.py:449-515) on the device: state_dim 9, action_bound 0.4 (:455-457),
    unclipped exploration noise N(0, 0.4 * 0.98) (:484), push HER relabel rule (utils/rl_utils.py:171-188).  The cube
    follows the build's simplified push-out model, so learning curves are not comparable with the reference's.
    ``task="pick"`` is ``train_pick_with_TD3`` (main.py:518-585), the same loop around RLPickEnv.  ``checkpoint``, ``checkpoint_every``,
    ``resume``, ``save``, ``save_best``: as train_reach's."""
    task = "push" if task == "push" else "pick"
    action_bound = _TASKS[task][2]
    return _train(task, action_bound * 0.98, 1e9, num_envs, iterations, rollout_steps, updates, batch_size,
                  her_ratio, seed, device, actor_kind, log_every, log, window_steps, minimal_episodes, max_steps, use_graphs, algo, learner,
                  checkpoint, checkpoint_every, resume, save, save_best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="reach", choices=list(_TASKS))
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--rollout-steps", type=int, default=32)
    ap.add_argument("--updates", type=int, default=48)
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--actor", default="actor_f16x3", choices=["actor", "actor_f16x3"])
    ap.add_argument("--sigma", type=float, default=0.7 * 0.98)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--window-steps", type=int, default=1536)
    ap.add_argument("--max-steps", type=int, default=500, help="opt.max_steps_one_episode")
    ap.add_argument("--graphs", type=int, default=1, help="1: the agent's updates replayed from hipGraphs (default); 0: issued eagerly")
    ap.add_argument("--algo", default="td3", choices=list(ALGOS), help="the agent (config.py:33's default is DADDPG_MLP)")
    ap.add_argument("--learner", default="torch", choices=["torch", "hip", "fused"],
                    help="torch: the agent's update in torch (default); hip: libarmenv's fused TD3 update (--algo td3 only); "
                         "fused: the agent's own fused HIP update (FusedTD3, FusedDADDPG, FusedDATD3 or FusedDARC)")
    add_cli_arguments(ap)
    a = ap.parse_args()
    check_cli_arguments(ap, a, a.learner)
    files = dict(checkpoint=a.checkpoint, checkpoint_every=a.checkpoint_every, resume=a.resume, save=a.save, save_best=a.save_best)
    if a.task != "reach":
        train_push(a.num_envs, a.iterations, a.rollout_steps, a.updates, a.batch_size, seed=a.seed, actor_kind=a.actor,
                   window_steps=a.window_steps, max_steps=a.max_steps, task=a.task, use_graphs=a.graphs == 1, algo=a.algo,
                   learner=a.learner, **files)
        return
    train_reach(a.num_envs, a.iterations, a.rollout_steps, a.updates, a.batch_size, seed=a.seed, actor_kind=a.actor,
                expl_sigma=a.sigma, window_steps=a.window_steps, max_steps=a.max_steps, algo=a.algo,
                use_graphs=a.graphs == 1, learner=a.learner, **files)


if __name__ == "__main__":
    main()
