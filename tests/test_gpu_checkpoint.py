"""Checkpoint and resume on cuda:0, held to equality: an uninterrupted run A, a run B that writes its state every third iteration
and a run C that builds fresh objects, resumes from B's file of iteration 3 and runs to 6 must agree in every tensor of the learner
(nets, targets, moments), its counters, the store's rings, draw counter and episode index, every env's ``get_state()`` fields and
``counters()``, and the history without ``wall_s`` -- ``torch.equal`` everywhere, no tolerance.  The shapes are the smallest at which
the checkpoint of iteration 3 already holds a wrapped ring (24 steps through a window of 16), finished episodes (5 steps long, 8
steps a rollout), ready stores and TD3's delayed actor step (2 updates an iteration, policy_freq 3); the tests assert that it does.
No new kernel: the existing ones, across a save and a restore."""
import os
import shutil

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = dict(num_envs=64, rollout_steps=8, window_steps=16, max_steps=5, minimal_episodes=5, updates=2, batch_size=64, iterations=6, log_every=2)
FIELDS = ("cap", "base", "T", "N", "D", "at_reset")
RINGS = ("obs0", "obs_after", "next_obs", "action", "reward", "done")


class Recorder:
    """Makes armenv.train's and armenv.train_pop's loops hand over what they otherwise drop: every store they create, every env's
    state and counters as it is closed, and a copy ``<file>.it<k>`` of every checkpoint written."""

    def __init__(self, monkeypatch):
        from armenv import checkpoint, replay, train, train_pop
        self.stores, self.envs = [], []

        def recording_store(cls):
            def make(*args, **kw):
                store = cls(*args, **kw)
                self.stores.append(store)
                return store
            return make

        def recording_env(cls):
            def make(*args, **kw):
                env = cls(*args, **kw)
                close = env.close

                def closing():
                    if env._h is not None:
                        self.envs.append((env, {k: v.cpu() for k, v in env.get_state().items()}, env.counters()))
                    close()
                env.close = closing
                return env
            return make

        def save_and_copy(path, state):
            checkpoint.save_run(path, state)
            shutil.copyfile(path, "%s.it%d" % (path, state["iteration"]))

        for module in (train, train_pop):
            monkeypatch.setattr(module, "TrajectoryStore", recording_store(replay.TrajectoryStore))
            monkeypatch.setattr(module, "save_run", save_and_copy)
        monkeypatch.setattr(train_pop, "PopulationTrajectoryStore", recording_store(replay.PopulationTrajectoryStore))
        for task, (cls, D, bound) in list(train._TASKS.items()):          # train_pop reads the same dict
            monkeypatch.setitem(train._TASKS, task, (recording_env(cls), D, bound))

    def run(self, fn, **kw):
        """one run of a loop as a dict of everything that is compared"""
        del self.stores[:], self.envs[:]
        agent, history = fn(log=lambda line: None, **kw)
        torch.cuda.synchronize(DEV)
        stores = []
        for st in self.stores:
            r = st._ring
            n = r["num_episodes"].reshape(-1).tolist()
            episodes = r["episodes"].reshape((len(n), -1, 3))
            stores.append(dict(geometry=[r[k] for k in FIELDS], rings={k: r[k].clone() for k in RINGS}, draw=st._draw, seed=st.seed,
                               num_episodes=n, episodes=[episodes[p, :n[p]].clone() for p in range(len(n))]))
        return dict(tensors={name: [t.clone() for t in ts] for name, ts in agent._state_tensors().items()},
                    counters={name: getattr(agent, name) for name in agent._COUNTERS}, rows=getattr(agent, "_rows", None),
                    stores=stores, envs=[(state, counters) for _, state, counters in self.envs],
                    history=[{k: v for k, v in rec.items() if k != "wall_s"} for rec in history], agent=agent)


@pytest.fixture
def recorder(monkeypatch):
    return Recorder(monkeypatch)


def _tensors_equal(x, y):
    return all(sorted(x) == sorted(y) and len(x[k]) == len(y[k]) and all(torch.equal(a, b) for a, b in zip(x[k], y[k])) for k in x)


def assert_same_run(x, y, what):
    bad = [(name, k) for name in x["tensors"] for k, (a, b) in enumerate(zip(x["tensors"][name], y["tensors"][name])) if not torch.equal(a, b)]
    assert sorted(x["tensors"]) == sorted(y["tensors"]) and not bad, (what, bad)
    assert x["counters"] == y["counters"] and x["rows"] == y["rows"], what
    assert len(x["stores"]) == len(y["stores"]) > 0, what
    for k, (s, t) in enumerate(zip(x["stores"], y["stores"])):
        assert s["geometry"] == t["geometry"] and (s["draw"], s["seed"]) == (t["draw"], t["seed"]), (what, k)
        assert s["num_episodes"] == t["num_episodes"] and min(s["num_episodes"]) > 0, (what, k)
        assert all(torch.equal(s["rings"][r], t["rings"][r]) for r in RINGS), (what, k)
        assert all(torch.equal(a, b) for a, b in zip(s["episodes"], t["episodes"])), (what, k)
    assert len(x["envs"]) == len(y["envs"]) > 0, what
    for k, ((sx, cx), (sy, cy)) in enumerate(zip(x["envs"], y["envs"])):
        assert sorted(sx) == sorted(sy) and "trig" in sx and all(torch.equal(sx[f], sy[f]) for f in sx), (what, k)
        assert cx == cy and cx["episodes"] > 0 and cx["env_steps"] == 6 * 8 * 64, (what, k)
    assert x["history"] == y["history"], what


def _abc(recorder, tmp_path, fn, **kw):
    """runs A, B and C of `fn`; returns them and the path of B's state of iteration 3"""
    kw = dict(SHAPES, **kw)
    fresh = kw.pop("fresh", lambda: {})                           # arguments that hold state of their own: made anew for every run
    a = recorder.run(fn, **dict(kw, **fresh()))
    path = str(tmp_path / "run.ckpt")
    b = recorder.run(fn, checkpoint=path, checkpoint_every=3, **dict(kw, **fresh()))
    assert sorted(os.listdir(tmp_path)) == ["run.ckpt", "run.ckpt.it3", "run.ckpt.it6"]
    c = recorder.run(fn, resume=path + ".it3", **dict(kw, **fresh()))
    assert_same_run(a, b, "A, B")
    assert_same_run(a, c, "A, C")
    return a, b, c, path + ".it3"


def _check_the_checkpoint_is_mid_run(path, learner_key, store_key, env_key):
    """what the shapes were chosen for: at iteration 3 the ring has wrapped, episodes have finished, the updates have run"""
    from armenv.checkpoint import load_run
    state = load_run(path)
    assert state["iteration"] == 3
    store = state[store_key][0] if store_key == "stores" else state[store_key]
    env = state[env_key][0] if env_key == "envs" else state[env_key]
    assert store["ring"]["base"] != 0 and store["ring"]["T"] == 16 and store["draw"] > 0 and store["ring"]["at_reset"] is False
    assert env["counters"]["episodes"] > 0 and int(env["fields"]["episode"].min()) > 1
    counters = state[learner_key]["counters"]
    assert counters["total_it"] >= 3 and all(v > 0 for v in counters.values()), counters
    return state


@pytest.mark.parametrize("algo", ["td3", "daddpg", "datd3"])
def test_train_reach_resumes_bit_for_bit(recorder, tmp_path, algo):
    from armenv.train import train_reach
    a, _, c, path = _abc(recorder, tmp_path, train_reach, algo=algo, learner="fused", seed=3)
    state = _check_the_checkpoint_is_mid_run(path, "agent", "store", "env")
    assert [rec["iteration"] for rec in a["history"]] == [2, 4, 6] and state["history"] == [dict(c["history"][0], wall_s=state["history"][0]["wall_s"])]
    assert a["counters"]["total_it"] > state["agent"]["counters"]["total_it"]
    assert not _tensors_equal(a["tensors"], {k: [t.to(DEV) for t in ts] for k, ts in state["agent"]["tensors"].items()})


def test_train_push_resumes_bit_for_bit(recorder, tmp_path):
    """the push task: the cube's state (aux) is part of what is restored"""
    from armenv.train import train_push
    a, _, _, path = _abc(recorder, tmp_path, train_push, algo="td3", learner="fused", seed=2)
    state = _check_the_checkpoint_is_mid_run(path, "agent", "store", "env")
    assert "aux" in state["env"]["fields"] and "goal" not in state["env"]["fields"] and "aux" in a["envs"][0][0]
    assert state["store"]["ring"]["D"] == 9


@pytest.mark.parametrize("store", ["population", "members"])
@pytest.mark.parametrize("algo", ["td3", "datd3"])
def test_train_reach_population_resumes_bit_for_bit(recorder, tmp_path, algo, store):
    """P = 3, swept actor_lr, PBT every 2 iterations: the steps fall before the checkpoint (2) and after it (4, 6)"""
    from armenv.train_pop import train_reach_population
    a, b, c, path = _abc(recorder, tmp_path, train_reach_population, members=3, algo=algo, store=store, seed=1,
                         sweep=dict(actor_lr=[1e-3, 5e-4, 2e-4]), pbt=dict(every=2))
    state = _check_the_checkpoint_is_mid_run(path, "population", "stores", "envs")
    assert len(a["stores"]) == (1 if store == "population" else 3) and len(a["envs"]) == 3
    assert [(rec.get("kind"), rec["iteration"]) for rec in a["history"]] == [(None, 2), ("pbt", 2), (None, 4), ("pbt", 4), (None, 6), ("pbt", 6)]
    assert [rec for rec in c["history"] if rec.get("kind") == "pbt"] == [rec for rec in a["history"] if rec.get("kind") == "pbt"]
    assert state["pbt"]["rng"][0] == 3 and len(state["sigmas"]) == 3 and len(state["history"]) == 2


def test_a_population_resumes_across_exploit_steps(recorder, tmp_path):
    """A schedule whose plan is fixed, so that members ARE replaced whatever the success rates, before and after the checkpoint: the
    replaced members' bits, their perturbed values and the records agree."""
    from armenv.pbt import PBTSchedule
    from armenv.train_pop import train_reach_population

    class Fixed(PBTSchedule):
        def plan(self, fitness):
            return [1, 1, 2]

    a, _, c, path = _abc(recorder, tmp_path, train_reach_population, members=3, algo="td3", seed=4, sweep=dict(actor_lr=[1e-3, 5e-4, 2e-4]),
                         fresh=lambda: dict(pbt=Fixed(every=2, seed=5)))
    steps = [rec for rec in c["history"] if rec.get("kind") == "pbt"]
    assert [rec["iteration"] for rec in steps] == [2, 4, 6] and all([n["member"] for n in rec["new"]] == [0] for rec in steps)
    assert all(rec["src"] == [1, 1, 2] and rec["new"][0]["source"] == 1 for rec in steps)
    assert all(torch.equal(t[0], t[1]) and not torch.equal(t[1], t[2]) for t in a["tensors"]["actor"])
    assert a["rows"][0] != a["rows"][1] and a["agent"].entry_point.endswith("_hyper")


def test_negative_control_a_zeroed_draw_counter_changes_the_run(recorder, tmp_path):
    """the comparison can fail: resumed with the store's draw counter at 0, the learner ends elsewhere"""
    from armenv.checkpoint import load_run, save_run
    from armenv.train import train_reach
    a, _, _, path = _abc(recorder, tmp_path, train_reach, algo="td3", learner="fused", seed=3)
    state = load_run(path)
    assert state["store"]["draw"] > 0
    state["store"]["draw"] = 0
    save_run(str(tmp_path / "spoilt.ckpt"), state)
    d = recorder.run(train_reach, resume=str(tmp_path / "spoilt.ckpt"), **dict(SHAPES, algo="td3", learner="fused", seed=3))
    assert d["counters"] == a["counters"] and d["stores"][0]["draw"] < a["stores"][0]["draw"]
    assert not _tensors_equal(a["tensors"], d["tensors"])


def test_set_state_with_trig_continues_bit_for_bit_and_without_it_is_recorded(record_property):
    """``load_state_dict`` restores ``trig``, the (cos q, sin q) pair that the engine carries: with it two handles continue alike in
    every bit.  Without it the pair is re-derived from q and the trajectories are ALLOWED to differ: whether they do at these
    shapes is recorded (``trig_matters``), not asserted."""
    from armenv import envs
    made = [envs.BatchedReachEnv(64, device=DEV, seed=7, max_steps=50) for _ in range(3)]
    gen = torch.Generator(device=DEV).manual_seed(1)
    actions = (torch.rand(40, 64, 3, device=DEV, generator=gen) * 1.4 - 0.7).contiguous()
    for e in made:
        e.reset()
    made[0].rollout(20, actions[:20].contiguous())
    sd = made[0].state_dict()
    made[1].load_state_dict(sd)
    made[2].set_state(**{k: v for k, v in sd["fields"].items() if k != "trig"})
    outs = [e.rollout(20, actions[20:].contiguous()) for e in made]
    torch.cuda.synchronize(DEV)
    finals = [e.get_state() for e in made]
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in ("obs", "reward", "done_u8", "success_u8"))
    assert all(torch.equal(finals[0][k], finals[1][k]) for k in finals[0])
    assert made[1].counters() == made[0].counters() and made[1].counters()["env_steps"] == 40 * 64
    trig_matters = not all(torch.equal(finals[0][k], finals[2][k]) for k in finals[0])
    record_property("trig_matters", trig_matters)
    print("set_state without trig: trajectories %s" % ("differ" if trig_matters else "are equal at these shapes"))
    for e in made:
        e.close()


@pytest.mark.parametrize("algo", ["td3", "daddpg", "datd3"])
def test_a_fused_learners_files_load_into_the_torch_learner(tmp_path, algo):
    """``save=`` writes the reference's files; ``load_agent`` reads them into the torch learner of the same agent, whose
    ``take_action`` on 8 fixed states is the fused learner's, bit for bit"""
    from armenv.checkpoint import load_agent
    from armenv.train import _TORCH, train_reach
    name = str(tmp_path / "agent")
    fused, _ = train_reach(log=lambda line: None, save=name, **dict(SHAPES, algo=algo, learner="fused", seed=5))
    assert fused.total_it > 0
    torch.manual_seed(9)
    learner = _TORCH[algo](6, 3, 0.7, device=DEV)
    load_agent(learner, name)
    states = torch.rand(8, 6, generator=torch.Generator().manual_seed(2)).tolist()
    for s in states:
        got, want = learner.take_action(s), fused.take_action(s)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    for net, target in zip(learner._nets()[:len(learner._nets()) // 2], learner._nets()[len(learner._nets()) // 2:]):
        assert all(torch.equal(p, q) for p, q in zip(net.parameters(), target.parameters()))


def test_save_best_writes_at_the_first_window_and_whenever_the_best_is_reached(monkeypatch, tmp_path):
    from armenv import checkpoint, train
    offers = []

    class Watched(checkpoint.BestKeeper):
        def offer(self, rate, agent):
            wrote = super().offer(rate, agent)
            files = {n: torch.load("%s.best_%s.pt" % (self.filename, n), weights_only=True) for n in ("actor", "critic")}
            offers.append((rate, wrote, files))
            return wrote

    monkeypatch.setattr(train, "BestKeeper", Watched)
    name = str(tmp_path / "agent")
    agent, history = train.train_reach(log=lambda line: None, save=name, save_best=True, **dict(SHAPES, algo="td3", learner="fused", seed=6))
    rates = [rec["success_rate"] for rec in history]
    assert [o[0] for o in offers] == rates and len(rates) == 3
    assert [o[1] for o in offers] == [k == 0 or rate >= max(rates[:k]) for k, rate in enumerate(rates)] and offers[0][1]
    for k in range(1, 3):          # a window that did not reach the best leaves the files as they were; one that did rewrites them
        unchanged = all(torch.equal(offers[k][2][n][key], offers[k - 1][2][n][key]) for n in ("actor", "critic") for key in offers[k][2][n])
        assert unchanged != offers[k][1], k
    assert sorted(os.listdir(tmp_path)) == ["agent.best_actor.pt", "agent.best_critic.pt", "agent_actor.pt", "agent_critic.pt"]
    final = torch.load(name + "_actor.pt", weights_only=True)
    assert all(torch.equal(final[k], v.cpu()) for k, v in agent.actor.state_dict().items())
    # the scripted sequence through the loop's helper: armenv.checkpoint.BestKeeper
    writes = []
    keeper = checkpoint.BestKeeper(name, write=lambda a, f: writes.append(f))
    assert [keeper.offer(r, None) for r in (0.25, 0.125, 0.25, 0.5, 0.375)] == [True, False, True, True, False]
    assert writes == [name + ".best"] * 3
