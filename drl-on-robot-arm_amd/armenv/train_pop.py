"""A population of agents trained side by side on the device: armenv.train's loop (the reference's run() / train_reach_with_TD3 /
train_push_with_TD3 / train_pick_with_TD3) for P independent agents -- a seed sweep -- whose updates are ONE fused HIP update of
the whole population at the reference's own operating point, 40 updates of 256 samples.  The agent: ``--algo td3`` (the default,
armenv.fused_td3_pop.FusedTD3Population), ``--algo daddpg`` -- the reference's default agent --
(armenv.fused_daddpg_pop.FusedDADDPGPopulation), or ``--algo datd3`` / ``--algo darc`` (armenv.fused_datd3_pop), whose one loop
update is one ``train`` = two reference updates on the batch, as in armenv.train.

    python -m armenv.train_pop --members 16 --iterations 200
    python -m armenv.train_pop --members 16 --iterations 200 --algo daddpg
    python -m armenv.train_pop --members 4 --sweep actor_lr=1e-3,5e-4,2e-4,1e-4 --sweep tau=0.005,0.005,0.01,0.01
    python -m armenv.train_pop --members 8 --iterations 60 --pbt-every 10
    python -m armenv.train_pop --members 8 --iterations 100 --share-replay 0.5

``sweep`` (``--sweep NAME=v0,v1,...``, one value per member): the members' own values of the agent's sweepable hyper-parameters
(``sweepable_names(algo)``: the learning rates, tau, gamma, the target-policy noise's two, DARC's two weights) and of ``expl_sigma``,
the rollout's exploration sigma -- a hyper-parameter sweep at the price of one run; every history record then carries them.

``pbt`` (``--pbt-every N``, ``--pbt-fraction F``, ``--pbt-perturb LO,HI``): population-based training, armenv.pbt.PBTSchedule.  After
every N iterations the members are ranked by their success rate since the last such step; the bottom fraction become copies of
members of the top (``pop.exploit``: nets, targets, moments and hyper-parameters, ONE launch) and their hyper-parameters -- and
``expl_sigma`` -- are perturbed (``explore``).  A replaced member keeps its environments, its replay ring and its noise seed.  Each
step is logged and kept in the history as a ``kind="pbt"`` record; every record then carries the members' current values.

``share_ratio`` (``--share-replay F``, F in [0, 1], ``store="population"`` only): a shared replay buffer.  Every row of a member's
batch is drawn, with probability F, from the trajectories of ALL members -- uniformly over the union of their episodes -- and from
its own otherwise (``PopulationTrajectoryStore.sample(share_ratio=F)``: still one launch per batch).  A member replaced by a PBT
step then no longer learns from the discarded policy's data alone.  0 (the default): the loop and its launches as without it.

Member p has its own environments, trajectory store, initial weights and noise, all seeded ``seed + p``.  Rollouts are P launches,
one per member, each with that member's policy (TD3: its actor; the two-actor agents: their own take_action, fused into the rollout
kernel).  ``store="population"`` (the default): the members' stores are one armenv.replay.PopulationTrajectoryStore -- the rollouts
write into its staging block, ONE ``add_rollouts`` per iteration moves them into the stacked rings and indexes every member, and
every update is ONE ``sample`` of the whole stacked batch and ONE ``pop.train``.  ``store="members"``: P TrajectoryStores, each
appended to, asked for its size and sampled into that member's slice of the stacked batch on its own -- the same bits, member by
member, kept for A/B runs (``--store``).

Lockstep rule: the members share the step schedule, so an iteration runs its updates only when EVERY member's store is ready (holds
``minimal_episodes`` complete episodes); while one member is not, no member is updated.  The members' stores fill at about the same
rate, so this delays the first update by a few iterations at most.

Stopping and continuing (armenv.checkpoint): ``checkpoint`` / ``checkpoint_every`` (``--checkpoint FILE --checkpoint-every N``) write
the whole run's state -- the population, the store(s), every env, the PBT schedule, the members' sigmas, the loop's variables -- after
every N-th iteration (after its PBT step) and after the last; ``resume`` (``--resume FILE``, every other argument but ``iterations``,
``log_every`` and the paths as in the saved run) continues at the next iteration and equals the uninterrupted run bit for bit, PBT
steps included.  ``save`` (``--save NAME``): every trained member p in the reference's files ``NAME.m<p>_actor.pt``, ...; with
``save_best`` also as ``NAME.m<p>.best_...`` whenever that member's logged success rate reaches its best."""
import argparse
import json
import time

from .checkpoint import (BestKeeper, add_cli_arguments, check_cli_arguments, check_config, check_loop_arguments, checkpoint_due, load_run,
                         save_run, to_cpu)
from .fused_daddpg_pop import FusedDADDPGPopulation
from .fused_datd3_pop import FusedDARCPopulation, FusedDATD3Population
from .fused_td3_pop import FusedTD3Population
from .pbt import PBTSchedule
from .replay import PopulationTrajectoryStore, TrajectoryStore
from .train import _TASKS, ALGOS, _install_policy

STORES = ("population", "members")
_POPULATIONS = dict(td3=FusedTD3Population, daddpg=FusedDADDPGPopulation, datd3=FusedDATD3Population, darc=FusedDARCPopulation)


def sweepable_names(algo):
    """the names that ``sweep`` may hold for agent `algo`"""
    return _POPULATIONS[algo].sweepable() + ("expl_sigma",)


def _checked_sweep(sweep, algo, members):
    """`sweep` as {name: [float] * members}; an unknown name or a wrong count raises ValueError"""
    out = {}
    for name, values in (sweep or {}).items():
        if name not in sweepable_names(algo):
            raise ValueError("sweep: %s is not one of %s's %s" % (name, algo, ", ".join(sweepable_names(algo))))
        values = [float(v) for v in values]
        if len(values) != members:
            raise ValueError("sweep: %s has %d values for %d members" % (name, len(values), members))
        out[name] = values
    return out


def _checked_pbt(pbt, algo, members, seed=0):
    """`pbt` (None, a PBTSchedule or a dict of its arguments, whose ``seed`` defaults to `seed`) as a schedule bound to agent
    `algo`'s names, or None; ValueError for arguments that PBTSchedule refuses, a name the agent does not have, or a population of
    one"""
    if pbt is None:
        return None
    if not isinstance(pbt, PBTSchedule):
        pbt = PBTSchedule(**dict(dict(seed=seed), **pbt))
    if members < 2:
        raise ValueError("pbt: population-based training needs members >= 2, not %d" % members)
    return pbt.bind(sweepable_names(algo))


def train_reach_population(members=16, num_envs=64, iterations=200, rollout_steps=32, updates=40, batch_size=256, her_ratio=0.8,
                           seed=0, device="cuda:0", actor_kind="actor_f16x3", expl_sigma=None, log_every=10, log=print,
                           window_steps=1536, minimal_episodes=5, max_steps=500, task="reach", algo="td3", store="population",
                           sweep=None, pbt=None, checkpoint=None, checkpoint_every=0, resume=None, save=None, save_best=False,
                           share_ratio=0.0):
    """Returns (population, history); a history record holds the members' success rates over the last ``log_every`` iterations.
    ``task="push" | "pick"``: armenv.train.train_push's settings (state_dim 9, action_bound 0.4, unclipped exploration noise).
    ``algo``: the agent; the two-actor agents explore as armenv.train has them explore on that task (the same sigma and clip).
    ``store``: "population" (one PopulationTrajectoryStore) or "members" (P TrajectoryStores); both train the same bits.
    ``sweep``: a dict from a name of ``sweepable_names(algo)`` to one value per member; every record then holds it as ``hyper``.
    Without it the members share every hyper-parameter and the records and the trained bits are what they always were.
    ``pbt``: an armenv.pbt.PBTSchedule, or a dict of its arguments (``dict(every=10)``; its seed defaults to `seed`):
    population-based training over the members, which must be two at least; checked, like ``sweep``, before anything is created on
    the device.  The history then also holds one ``kind="pbt"`` record per PBT step -- iteration, the fitness (success rates since
    the last step), ``src`` and the replaced members' new values -- and every record holds the members' current values as
    ``hyper``.  Without it the loop, the records and the trained bits are what they are without the argument.
    ``share_ratio``: the module's docstring; in [0, 1], and 0 with ``store="members"``, or ValueError before anything is created on
    the device.  It is part of the run's configuration: a resume with another value is refused.
    ``checkpoint``, ``checkpoint_every``, ``resume``, ``save``, ``save_best``: the module's docstring; a `resume` whose saved arguments
    are not this call's raises ValueError naming the first that differs, before anything is created on the device."""
    if task not in _TASKS:
        raise ValueError("task must be one of %s" % ", ".join(_TASKS))
    if algo not in ALGOS:
        raise ValueError("algo must be one of %s" % ", ".join(ALGOS))
    if store not in STORES:
        raise ValueError("store must be one of %s" % ", ".join(STORES))
    share_ratio = float(share_ratio)
    if not 0.0 <= share_ratio <= 1.0:
        raise ValueError("share_ratio must be in [0, 1], not %r" % share_ratio)
    if share_ratio and store != "population":
        raise ValueError('share_ratio = %r needs store="population": the members\' own stores cannot read each other' % share_ratio)
    Env, state_dim, action_bound = _TASKS[task]
    sigma = expl_sigma if expl_sigma is not None else action_bound * 0.98
    noise_clip = action_bound if task == "reach" else 1e9
    P = int(members)
    sweep = _checked_sweep(sweep, algo, P)
    pbt = _checked_pbt(pbt, algo, P, seed)
    check_loop_arguments("fused", checkpoint, checkpoint_every, resume, save, save_best)
    # every argument that shapes the run: a resumed run must repeat them
    config = dict(task=task, algo=algo, learner="fused", members=P, num_envs=num_envs, rollout_steps=rollout_steps, updates=updates,
                  batch_size=batch_size, her_ratio=her_ratio, seed=seed, actor_kind=actor_kind, expl_sigma=sigma, window_steps=window_steps,
                  minimal_episodes=minimal_episodes, max_steps=max_steps, store=store, sweep=sweep,
                  pbt=None if pbt is None else {k: v for k, v in pbt.state_dict().items() if k != "rng"})
    if share_ratio:                # recorded where it is used: a run without it writes, and resumes from, the checkpoints it always did
        config["share_ratio"] = share_ratio
    saved = None
    if resume is not None:
        saved = load_run(resume)
        check_config(saved["config"], config)
    sigmas = list(sweep.get("expl_sigma", [sigma] * P))
    pop = _POPULATIONS[algo](P, state_dim, 3, action_bound, device=device, seed=seed,
                             **{name: values for name, values in sweep.items() if name != "expl_sigma"})
    es = [Env(num_envs, device=device, seed=seed + p, max_steps=max_steps) for p in range(P)]
    batch = pop.batch_buffers(batch_size)
    obs = [e.reset() for e in es]
    if store == "population":
        pstore = PopulationTrajectoryStore(P, device=device, seed=seed, capacity_steps=window_steps)
        bufs = pstore.rollout_buffers(rollout_steps, num_envs, state_dim)
        obs0 = obs[0].new_empty((P,) + tuple(obs[0].shape))
    else:
        stores = [TrajectoryStore(device=device, seed=seed + p, capacity_steps=window_steps) for p in range(P)]
        slices = [pop.member_buffers(p) for p in range(P)]
        bufs = [{} for _ in range(P)]
    prev = [e.counters() for e in es]
    prev_pbt = prev
    history = []

    def rows():
        """the members' current values: the population's own and the rollout's sigma"""
        return [dict(pop.hyper(p), expl_sigma=sigmas[p]) for p in range(P)]

    def current():
        """... as a history record holds them: by name, for the swept and the perturbed names"""
        names = [n for n in sweepable_names(algo) if n in sweep or n in pbt.names]
        return {n: [row[n] for row in rows()] for n in names}

    bests = [BestKeeper("%s.m%d" % (save, p)) for p in range(P)] if save_best else None
    first, wall0 = 0, 0.0
    if saved is not None:          # continue at iteration saved + 1 with the saved run's objects and variables
        pop.load_state_dict(saved["population"])
        if store == "population":
            pstore.load_state_dict(saved["stores"][0])
        else:
            for st, sd in zip(stores, saved["stores"]):
                st.load_state_dict(sd)
            obs = [t.to(e.device) for t, e in zip(saved["obs"], es)]
        for e, sd in zip(es, saved["envs"]):
            e.load_state_dict(sd)
        if pbt:
            pbt.load_state_dict(saved["pbt"])
        sigmas[:] = saved["sigmas"]
        prev, prev_pbt, history = saved["prev"], saved["prev_pbt"], saved["history"]
        first, wall0 = saved["iteration"], saved["wall_s"]
        for keeper, sd in zip(bests or (), saved["bests"] or ()):
            keeper.load_state_dict(sd)
    t0 = time.perf_counter()
    for it in range(first, iterations):
        if store == "population":
            for p, e in enumerate(es):
                _install_policy(e, algo, pop.member(p), actor_kind, action_bound, sigmas[p], noise_clip)
                if it == 0:
                    obs0[p].copy_(obs[p])                  # the window's first observation: read by the first add_rollouts only
                e.rollout(rollout_steps, None, out=bufs[p], want_actions=True, want_terminal_obs=True)
            pstore.add_rollouts(obs0, starts_at_reset=(it == 0))
            # lockstep: re-checked every iteration (a ring window can lose its complete episodes again, see armenv.train)
            if pstore.ready(minimal_episodes):
                for _ in range(updates):
                    pstore.sample(batch_size, use_her=True, her_ratio=her_ratio, out=batch, share_ratio=share_ratio)
                    pop.train(batch)                      # datd3 / darc: two updates, as the reference's run() counts them
        else:
            for p, e in enumerate(es):
                _install_policy(e, algo, pop.member(p), actor_kind, action_bound, sigmas[p], noise_clip)
                obs0 = obs[p].clone()
                out = e.rollout(rollout_steps, None, out=bufs[p], want_actions=True, want_terminal_obs=True)
                obs[p] = out["obs"][-1]
                stores[p].add_rollout(obs0, out, starts_at_reset=(it == 0))
            # lockstep: re-checked every iteration (a ring window can lose its complete episodes again, see armenv.train)
            if all(st.size() >= minimal_episodes for st in stores):
                for _ in range(updates):
                    for p, st in enumerate(stores):
                        st.sample(batch_size, use_her=True, her_ratio=her_ratio, out=slices[p])
                    pop.train(batch)                      # datd3 / darc: two updates, as the reference's run() counts them
        if (it + 1) % log_every == 0:
            cs = [e.counters() for e in es]
            rates = [(c["successes"] - c0["successes"]) / max(1, c["episodes"] - c0["episodes"]) for c, c0 in zip(cs, prev)]
            prev = cs
            rec = dict(iteration=it + 1, env_steps=sum(c["env_steps"] for c in cs), episodes=[c["episodes"] for c in cs],
                       success_rate=rates, wall_s=wall0 + (time.perf_counter() - t0))
            if pbt:
                rec["hyper"] = current()
            elif sweep:
                rec["hyper"] = sweep
            history.append(rec)
            log(json.dumps(rec))
            for p, keeper in enumerate(bests or ()):      # main.py:151-153, per member
                keeper.offer(rates[p], pop.member(p))
        if pbt and pbt.due(it + 1):
            cs = [e.counters() for e in es]
            fitness = [(c["successes"] - c0["successes"]) / max(1, c["episodes"] - c0["episodes"]) for c, c0 in zip(cs, prev_pbt)]
            prev_pbt = cs
            src, new = pbt.step(fitness, rows())
            if new:
                pop.exploit(src, hyper=True)
                for p, row in new.items():
                    sigmas[p] = row.pop("expl_sigma")
                    pop.set_hyper(p, **row)
            rec = dict(kind="pbt", iteration=it + 1, fitness=fitness, src=src,
                       new=[dict(member=p, source=src[p], hyper=dict(pop.hyper(p), expl_sigma=sigmas[p])) for p in new],
                       hyper=current())
            history.append(rec)
            log(json.dumps(rec))
        if checkpoint_due(it + 1, iterations, checkpoint, checkpoint_every):
            save_run(checkpoint, dict(config=config, iteration=it + 1, population=pop.state_dict(),
                                      stores=[st.state_dict() for st in ([pstore] if store == "population" else stores)],
                                      envs=[e.state_dict() for e in es], pbt=pbt.state_dict() if pbt else None, sigmas=list(sigmas),
                                      prev=prev, prev_pbt=prev_pbt, obs=[to_cpu(t) for t in obs], history=history,
                                      wall_s=wall0 + (time.perf_counter() - t0),
                                      bests=[k.state_dict() for k in bests] if bests else None))
    if save is not None:
        pop.save(save)
    for e in es:
        e.close()
    return pop, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="reach", choices=list(_TASKS))
    ap.add_argument("--algo", default="td3", choices=list(ALGOS), help="the agent (config.py:33's default is DADDPG_MLP)")
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--num-envs", type=int, default=64, help="environments per member")
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--rollout-steps", type=int, default=32)
    ap.add_argument("--updates", type=int, default=40)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--actor", default="actor_f16x3", choices=["actor", "actor_f16x3"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--window-steps", type=int, default=1536)
    ap.add_argument("--max-steps", type=int, default=500)
    ap.add_argument("--store", default="population", choices=list(STORES),
                    help="population: one stacked store, indexed and sampled in one launch each; members: one store per member")
    ap.add_argument("--sweep", action="append", default=[], metavar="NAME=v0,v1,...",
                    help="the members' own values of a hyper-parameter (or of expl_sigma), exactly --members of them; repeatable")
    ap.add_argument("--pbt-every", type=int, default=None, metavar="N",
                    help="population-based training: after every N iterations the bottom members copy top members and perturb "
                         "their hyper-parameters")
    ap.add_argument("--pbt-fraction", type=float, default=0.25, metavar="F", help="the bottom's (and the top's) share of the members, in (0, 0.5]")
    ap.add_argument("--pbt-perturb", default="0.8,1.2", metavar="LO,HI", help="the two factors a perturbed value is multiplied by")
    ap.add_argument("--share-replay", type=float, default=0.0, metavar="F",
                    help="the share, in [0, 1], of every member's batch that is drawn from all members' trajectories (--store population)")
    add_cli_arguments(ap)
    a = ap.parse_args()
    check_cli_arguments(ap, a, "fused")
    if not 0.0 <= a.share_replay <= 1.0 or (a.share_replay and a.store != "population"):
        ap.error("--share-replay: a number in [0, 1], and 0 unless --store population")
    pbt = None
    if a.pbt_every is not None:
        try:
            pbt = _checked_pbt(dict(every=a.pbt_every, fraction=a.pbt_fraction, perturb=[float(v) for v in a.pbt_perturb.split(",")]),
                                a.algo, a.members, a.seed)
        except ValueError as e:
            ap.error("--pbt-*: %s" % e)
    sweep = {}
    for item in a.sweep:
        name, _, values = item.partition("=")
        try:
            sweep[name] = [float(v) for v in values.split(",")]
        except ValueError:
            ap.error("--sweep %s: NAME=v0,v1,... with numbers" % item)
    try:
        sweep = _checked_sweep(sweep, a.algo, a.members)
    except ValueError as e:
        ap.error(str(e))
    train_reach_population(a.members, a.num_envs, a.iterations, a.rollout_steps, a.updates, a.batch_size, seed=a.seed,
                           actor_kind=a.actor, window_steps=a.window_steps, max_steps=a.max_steps, task=a.task, algo=a.algo, store=a.store,
                           sweep=sweep or None, pbt=pbt, checkpoint=a.checkpoint, checkpoint_every=a.checkpoint_every, resume=a.resume,
                           save=a.save, save_best=a.save_best, share_ratio=a.share_replay)


if __name__ == "__main__":
    main()
