"""CPU tests of armenv.checkpoint and of the state that the loops' objects give and take: the agents' files against the reference's
(tests/golden/agent_state_keys.json: names and shapes read off the reference's modules by tests/golden/gen_agent_state_keys.py),
``save`` / ``load`` round trips and refusals, ``state_dict`` / ``load_state_dict`` of the fused learners, their populations, both
stores and the PBT schedule, the run file, and what the loops and the two CLIs refuse before they touch a device.  Everything here is
a copy or a refusal: equality is the only bar."""
import os
import random
import re
import sys

import pytest
import torch

from conftest import golden_json
from learner_host import classes

KINDS = ("td3", "daddpg", "datd3", "darc")
FIXTURE = golden_json("agent_state_keys.json")


def _torch_class(kind):
    from armenv.train import _TORCH
    return _TORCH[kind]


def _agent(flavour, kind, D=6, seed=0):
    """a torch learner, a fused learner or member 1 of a population of three, on the host"""
    torch.manual_seed(seed)
    if flavour == "torch":
        return _torch_class(kind)(D, 3, 0.7, device="cpu")
    Pop, Single, _ = classes(kind)
    if flavour == "fused":
        return Single(D, 3, 0.7, device="cpu") if kind == "daddpg" else Single(D, 3, 0.7, device="cpu", seed=seed)
    pop = Pop(3, D, 3, 0.7, device="cpu", seed=seed)
    member = pop.member(1)
    member._population = pop              # keeps the stacks' owner alive for the test
    return member


def _nets(agent):
    from armenv.checkpoint import agent_nets
    names = agent_nets(agent)
    return [getattr(agent, n) for n in names], [getattr(agent, "target_" + n) for n in names]


def _tensors(agent):
    return [t for nets in _nets(agent) for net in nets for t in net.state_dict().values()]


def same(x, y):
    """deep equality of nested dicts / lists of tensors and plain values; tensors by torch.equal and dtype"""
    if torch.is_tensor(x) or torch.is_tensor(y):
        return torch.is_tensor(x) and torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and sorted(x) == sorted(y) and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(same(a, b) for a, b in zip(x, y))
    return type(x) is type(y) and x == y


def plain(x):
    """whether x is CPU tensors and plain numbers, strings, lists and dicts only"""
    if torch.is_tensor(x):
        return x.device.type == "cpu"
    if isinstance(x, dict):
        return all(isinstance(k, str) and plain(v) for k, v in x.items())
    if isinstance(x, list):
        return all(plain(v) for v in x)
    return x is None or type(x) in (int, float, str, bool)


# ------------------------------------------------------------------------------------------------ the agents' files

@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", ["torch", "fused", "member"])
def test_saved_files_are_the_references(tmp_path, flavour, kind, D):
    agent = _agent(flavour, kind, D)
    written = agent.save(str(tmp_path / "agent"))
    want = FIXTURE[str(D)][kind]
    assert sorted(os.listdir(tmp_path)) == sorted("agent" + suffix for suffix in want)
    assert sorted(os.path.basename(p) for p in written) == sorted(os.listdir(tmp_path))
    for suffix, keys in want.items():
        sd = torch.load(str(tmp_path / ("agent" + suffix)), map_location="cpu", weights_only=True)
        assert [[k, list(v.shape)] for k, v in sd.items()] == keys, suffix
        assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in sd.values())


def test_save_agent_is_the_method_and_a_population_writes_every_member(tmp_path):
    from armenv.checkpoint import load_agent, save_agent
    agent = _agent("fused", "td3")
    save_agent(agent, str(tmp_path / "a"))
    agent.save(str(tmp_path / "b"))
    for suffix in ("_critic.pt", "_actor.pt"):
        assert same(torch.load(str(tmp_path / ("a" + suffix)), weights_only=True), torch.load(str(tmp_path / ("b" + suffix)), weights_only=True))
    Pop = classes("daddpg")[0]
    pop, other = Pop(3, 6, 3, 0.7, device="cpu", seed=0), Pop(3, 6, 3, 0.7, device="cpu", seed=9)
    pop.save(str(tmp_path / "pop"))
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("pop")) == sorted(
        "pop.m%d_%s.pt" % (p, n) for p in range(3) for n in ("critic", "actor1", "actor2"))
    other.load(str(tmp_path / "pop"))
    load_agent(other.member(2), str(tmp_path / "pop.m0"))
    for name in ("actor1", "actor2", "critic"):
        for t, u in zip(pop.stacks[name], other.stacks[name]):
            assert torch.equal(t[:2], u[:2]) and torch.equal(u[2], t[0])
        for t, u in zip(other.stacks[name], other.stacks["target_" + name]):
            assert torch.equal(t, u)
    with pytest.raises(TypeError):
        save_agent(object(), str(tmp_path / "x"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", ["torch", "fused", "member"])
def test_agent_round_trip(tmp_path, flavour, kind):
    """save, then load into an agent of another seed: its nets are the saved ones, its targets are copies of ITS nets (the saved
    agent's targets, which differ from its nets here, are not in the files), its moments and counters are untouched."""
    a, b = _agent(flavour, kind, seed=1), _agent(flavour, kind, seed=2)
    with torch.no_grad():
        for target in _nets(a)[1]:
            for t in target.state_dict().values():
                t.add_(0.25)
    moments = []
    if flavour != "torch":
        owner = b._population if flavour == "member" else b
        moments = [t for name, ts in owner._state_tensors().items() if name.endswith(("_m", "_v")) for t in ts]
        assert moments
        for k, t in enumerate(moments):
            t.fill_(0.5 + k)
        for k, name in enumerate(owner._COUNTERS):
            setattr(owner, name, 3 + k)
    else:
        owner = b
        b.total_it = 7
    kept = [t.clone() for t in moments]
    counters = {n: getattr(owner, n) for n in getattr(owner, "_COUNTERS", ("total_it",))}
    assert not any(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b)))
    a.save(str(tmp_path / "agent"))
    b.load(str(tmp_path / "agent"))
    for net_a, target_a, net_b, target_b in zip(*_nets(a), *_nets(b)):
        assert same(dict(net_a.state_dict()), dict(net_b.state_dict()))
        assert same(dict(net_b.state_dict()), dict(target_b.state_dict()))
        assert not same(dict(target_a.state_dict()), dict(target_b.state_dict()))
    assert all(torch.equal(x, y) for x, y in zip(kept, moments))
    assert {n: getattr(owner, n) for n in counters} == counters
    if flavour == "member":           # through the views: the stacks hold it, the other members are as they were
        fresh = classes(kind)[0](3, 6, 3, 0.7, device="cpu", seed=2)
        for name in fresh._NETS:
            for t, u in zip(owner.stacks[name], fresh.stacks[name]):
                assert torch.equal(t[0], u[0]) and torch.equal(t[2], u[2]) and not torch.equal(t[1], u[1])


def _rewrite(path, change):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    change(sd)
    torch.save(sd, path)


LOAD_REFUSALS = [
    ("missing file", lambda path: os.remove(path), None),
    ("missing key", lambda path: _rewrite(path, lambda sd: sd.pop("fc2.bias")), "fc2.bias"),
    ("extra key", lambda path: _rewrite(path, lambda sd: sd.update({"fc9.weight": torch.zeros(2)})), "fc9.weight"),
    ("wrong shape", lambda path: _rewrite(path, lambda sd: sd.update({"fc1.weight": torch.zeros(256, 5)})), "fc1.weight"),
]


@pytest.mark.parametrize("which", [0, -1])
@pytest.mark.parametrize("what,spoil,key", LOAD_REFUSALS)
@pytest.mark.parametrize("flavour,kind", [("torch", "td3"), ("fused", "daddpg"), ("member", "datd3"), ("fused", "darc"), ("member", "td3")])
def test_load_refusals_name_file_and_key_and_change_nothing(tmp_path, flavour, kind, what, spoil, key, which):
    """the spoilt file is the first or the last one read: every file is checked before the first tensor is written"""
    a, b = _agent(flavour, kind, seed=1), _agent(flavour, kind, seed=2)
    paths = a.save(str(tmp_path / "agent"))
    spoil(paths[which])
    before = [t.clone() for t in _tensors(b)]
    with pytest.raises(ValueError) as err:
        b.load(str(tmp_path / "agent"))
    assert os.path.basename(paths[which]) in str(err.value), what
    assert key is None or repr(key) in str(err.value), what
    assert all(torch.equal(x, y) for x, y in zip(before, _tensors(b)))


# ------------------------------------------------------------------------------------------------ the learners' whole state

def _mid_run(learner, seed):
    """random nets, targets and moments everywhere and counters that are not a fresh learner's"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for ts in learner._state_tensors().values():
            for t in ts:
                t.copy_(torch.rand(t.shape, generator=gen))
    for k, name in enumerate(learner._COUNTERS):
        setattr(learner, name, 5 + k)
    return learner


def _single(kind, seed, D=6):
    Single = classes(kind)[1]
    torch.manual_seed(seed)
    return Single(D, 3, 0.7, device="cpu") if kind == "daddpg" else Single(D, 3, 0.7, device="cpu", seed=seed)


@pytest.mark.parametrize("kind", KINDS)
def test_single_learner_state_round_trip(kind):
    a, b = _mid_run(_single(kind, 1), 10), _single(kind, 2)
    b._args = b._one = object()
    sd = a.state_dict()
    assert plain(sd) and sd["kind"] == type(a).__name__ and sd["counters"] == {n: 5 + k for k, n in enumerate(a._COUNTERS)}
    assert len(sd["tensors"]) == 4 * len(a._LEARNING) and sd["seed"] == (None if kind == "daddpg" else 1)
    assert all(t.data_ptr() != u.data_ptr() for name, ts in a._state_tensors().items() for t, u in zip(ts, sd["tensors"][name]))
    assert not same(sd, b.state_dict())
    b.load_state_dict(sd)
    assert same(sd, b.state_dict()) and same(sd, a.state_dict())
    assert b._args is None and b._one is None                 # the next train binds anew
    assert {n: getattr(b, n) for n in b._COUNTERS} == sd["counters"] and getattr(b, "seed", None) == sd["seed"]
    assert torch.equal(b.actor.fc1.weight, a.actor.fc1.weight)        # in place: the modules show it


@pytest.mark.parametrize("kind", KINDS)
def test_population_state_round_trip(kind):
    Pop = classes(kind)[0]
    a = _mid_run(Pop(3, 6, 3, 0.7, device="cpu", seed=1, actor_lr=[1e-3, 5e-4, 2e-4]), 11)
    a.set_hyper(2, tau=0.01)
    b = Pop(3, 6, 3, 0.7, device="cpu", seed=7)
    views = [t.data_ptr() for t in b.member(1).actor.parameters()]
    b._args = b._one = object()
    sd = a.state_dict()
    assert plain(sd) and sd["members"] == 3 and sd["seed"] == 1 and sorted(sd["tensors"]) == sorted(a.stacks)
    assert sd["rows"] == [a.hyper(p) for p in range(3)] and [r["actor_lr"] for r in sd["rows"]] == [1e-3, 5e-4, 2e-4]
    assert b.uniform() and not same(sd, b.state_dict())
    b.load_state_dict(sd)
    assert same(sd, b.state_dict())
    assert b._args is None and b._one is None and b.seed == 1
    assert [b.hyper(p) for p in range(3)] == sd["rows"] and b.actor_lr == (1e-3, 5e-4, 2e-4) and b.tau == (0.005, 0.005, 0.01)
    assert not b.uniform() and b.entry_point.endswith("_hyper")
    assert {n: getattr(b, n) for n in b._COUNTERS} == sd["counters"]
    assert views == [t.data_ptr() for t in b.member(1).actor.parameters()]       # the members are still views into the stacks
    assert torch.equal(b.member(1).actor.fc1.weight, a.member(1).actor.fc1.weight)


def _spoilt(sd, path, value):
    """a copy of the nested `sd` with the entry at `path` replaced"""
    if not path:
        return value
    out = dict(sd) if isinstance(sd, dict) else list(sd)
    out[path[0]] = _spoilt(sd[path[0]], path[1:], value)
    return out


def test_learner_state_mismatches_are_refused_with_the_field_named():
    Pop, Single, _ = classes("td3")
    single, pop = _mid_run(_single("td3", 1), 12), _mid_run(Pop(3, 6, 3, 0.7, device="cpu", seed=1), 13)
    good_s, good_p = single.state_dict(), pop.state_dict()
    cases = [
        (single, _single("datd3", 1).state_dict(), "kind"),
        (single, _single("td3", 1, D=9).state_dict(), "state_dim"),
        (single, _spoilt(good_s, ("hidden_dim",), 128), "hidden_dim"),
        (single, _spoilt(good_s, ("counters",), dict(total_it=1)), "counters"),
        (single, _spoilt(good_s, ("tensors",), {k: v for k, v in good_s["tensors"].items() if k != "actor_m"}), "tensors"),
        (single, _spoilt(good_s, ("tensors", "critic_v", 3), torch.zeros(255)), r"critic_v\[3\]"),
        (single, _spoilt(good_s, ("tensors", "actor", 0), torch.zeros(256, 6, dtype=torch.float64)), r"actor\[0\]"),
        (single, _spoilt(good_s, ("seed",), None), "seed"),
        (single, good_p, "kind"),
        (pop, good_s, "kind"),
        (pop, Pop(2, 6, 3, 0.7, device="cpu").state_dict(), "members"),
        (pop, _spoilt(good_p, ("tensors", "q1", 0), torch.zeros(2, 256, 9)), r"q1\[0\]"),
        (pop, _spoilt(good_p, ("rows",), good_p["rows"][:2]), "rows"),
        (pop, _spoilt(good_p, ("rows", 1), dict(tau=0.1)), r"rows\[1\]"),
        (pop, _spoilt(good_p, ("rows", 2, "tau"), 1.5), "tau"),
    ]
    for learner, sd, field in cases:
        before = learner.state_dict()
        with pytest.raises(ValueError, match=field):
            learner.load_state_dict(sd)
        assert same(before, learner.state_dict()), field


# ------------------------------------------------------------------------------------------------ the stores

@pytest.fixture
def indexed(monkeypatch):
    """armenv.replay with the index launches counted and left out, so that the stores' host side runs on the cpu device"""
    from armenv import replay
    calls = []
    monkeypatch.setattr(replay.TrajectoryStore, "_index", lambda self: calls.append(self))
    monkeypatch.setattr(replay.PopulationTrajectoryStore, "_index", lambda self: calls.append(self))
    return replay, calls


def _filled(replay, population, seed, cap=20, Tc=8, N=3, D=6, chunks=4):
    gen = torch.Generator().manual_seed(5)
    lead = (3,) if population else ()
    st = replay.PopulationTrajectoryStore(3, device="cpu", seed=seed, capacity_steps=cap) if population \
        else replay.TrajectoryStore(device="cpu", seed=seed, capacity_steps=cap)
    f = lambda *shape: torch.rand(lead + shape, generator=gen)
    if population:
        st.rollout_buffers(Tc, N, D)
    for c in range(chunks):
        out = dict(obs=f(Tc, N, D), terminal_obs=f(Tc, N, D), actions=f(Tc, N, 3), reward=f(Tc, N), done_u8=(f(Tc, N) < 0.3).to(torch.uint8))
        if population:
            for k, t in out.items():
                st._staging[k].copy_(t)
            st.add_rollouts(f(N, D), starts_at_reset=(c == 0))
        else:
            st.add_rollout(f(N, D), out, starts_at_reset=(c == 0))
    return st


@pytest.mark.parametrize("population", [False, True])
def test_store_state_round_trip(indexed, population):
    replay, calls = indexed
    a = _filled(replay, population, seed=3)
    a._draw = 17
    r = a._ring
    assert (r["cap"], r["base"], r["T"], r["at_reset"]) == (20, 12, 20, False)        # wrapped
    sd = a.state_dict()
    assert plain(sd) and sd["draw"] == 17 and sd["seed"] == 3 and sd["started"] is True and sd["capacity"] == 20
    assert sorted(sd["ring"]) == sorted(("cap", "base", "T", "N", "D", "at_reset", "obs0", "obs_after", "next_obs", "action", "reward", "done"))
    b = (replay.PopulationTrajectoryStore(3, device="cpu", seed=9, capacity_steps=20) if population
         else replay.TrajectoryStore(device="cpu", seed=9, capacity_steps=20))
    b._bound = object()
    del calls[:]
    b.load_state_dict(sd)
    assert calls == [b]                                                                # the index is made again, not loaded
    assert same(sd, b.state_dict()) and (b.seed, b._draw, b._started) == (3, 17, True)
    assert all(b._ring[k] == r[k] for k in ("cap", "base", "T", "N", "D", "at_reset"))
    for k in ("counts", "offsets", "episodes", "num_episodes"):
        assert k in b._ring
    # into a store that already holds a ring: in place
    c = _filled(replay, population, seed=4, chunks=1)
    ptr = c._ring["obs_after"].data_ptr()
    c.load_state_dict(sd)
    assert same(sd, c.state_dict()) and c._ring["obs_after"].data_ptr() == ptr
    # an empty store's state
    empty = type(a)(3, device="cpu", capacity_steps=20) if population else type(a)(device="cpu", capacity_steps=20)
    assert empty.state_dict()["ring"] is None
    c.load_state_dict(empty.state_dict())
    assert c.chunk is None and not c._started


def test_store_state_mismatches_are_refused_with_the_field_named(indexed):
    replay, _ = indexed
    single, pop = _filled(replay, False, 1), _filled(replay, True, 1)
    good = single.state_dict()
    cases = [(single, pop.state_dict(), "kind"), (pop, good, "kind"),
             (pop, replay.PopulationTrajectoryStore(2, device="cpu", capacity_steps=20).state_dict(), "members"),
             (single, replay.TrajectoryStore(device="cpu", capacity_steps=24).state_dict(), "capacity"),
             (single, _filled(replay, False, 1, N=4).state_dict(), r": N is 4 "),
             (single, _filled(replay, False, 1, D=9).state_dict(), r": D is 9 "),
             (single, _spoilt(good, ("ring", "reward"), torch.zeros(20, 4)), "reward"),
             (single, _spoilt(good, ("ring", "done"), torch.zeros(20, 3)), "done"),
             (single, _spoilt(good, ("ring", "base"), 20), "base")]
    for store, sd, field in cases:
        before = store.state_dict()
        with pytest.raises(ValueError, match=field):
            store.load_state_dict(sd)
        assert same(before, store.state_dict()), field


# ------------------------------------------------------------------------------------------------ the PBT schedule

def test_pbt_schedule_state():
    """two schedules, one restored from the other's state after three steps, return equal steps for ten more"""
    from armenv.pbt import PBTSchedule
    from armenv.train_pop import sweepable_names
    names = sweepable_names("td3")
    a = PBTSchedule(every=2, fraction=0.5, seed=4).bind(names)
    rows = [dict({n: 0.1 * (p + 1) for n in names}) for p in range(6)]
    fit = random.Random(1)
    for _ in range(3):
        a.step([fit.random() for _ in range(6)], rows)
    sd = a.state_dict()
    assert plain(sd) and sd["names"] == list(a.names) and sd["every"] == 2 and sd["fraction"] == 0.5 and sd["seed"] == 4
    b = PBTSchedule(every=2, fraction=0.5, seed=4)
    assert b.names is None
    b.load_state_dict(sd)
    assert b.names == a.names and same(sd, b.state_dict())
    fresh = PBTSchedule(every=2, fraction=0.5, seed=4).bind(names)
    differs = False
    for _ in range(10):
        fitness = [fit.random() for _ in range(6)]
        got = a.step(fitness, rows)
        assert b.step(fitness, rows) == got
        differs = differs or fresh.step(fitness, rows) != got
    assert differs                                            # the generator's state is what was restored, not the seed
    for kw, field in ((dict(every=3), "every"), (dict(fraction=0.25), "fraction"), (dict(perturb=(0.5, 2.0)), "perturb"), (dict(seed=5), "seed")):
        other = PBTSchedule(**dict(dict(every=2, fraction=0.5, seed=4), **kw))
        state = other.rng.getstate()
        with pytest.raises(ValueError, match=field):
            other.load_state_dict(sd)
        assert other.names is None and other.rng.getstate() == state


# ------------------------------------------------------------------------------------------------ the file

def test_run_file_round_trip_and_format(tmp_path):
    from armenv import _lib as L
    from armenv.checkpoint import FORMAT, load_run, save_run
    path = str(tmp_path / "run.ckpt")
    state = dict(iteration=3, wall_s=1.25, name="x", none=None, flag=True, sigmas=[0.5, 0.25],
                 nested=dict(t=torch.arange(6, dtype=torch.int32).view(2, 3), deeper=[dict(u=torch.rand(4, dtype=torch.float64)), 7]))
    save_run(path, state)
    assert os.listdir(tmp_path) == ["run.ckpt"]
    assert same(load_run(path), state)
    blob = torch.load(path, map_location="cpu", weights_only=True)          # nothing but tensors and plain containers
    assert blob["format"] == FORMAT and blob["abi"] == L.ABI_VERSION == 9 and list(blob)[:2] == ["format", "abi"]
    torch.save(dict(format=FORMAT + 98, abi=L.ABI_VERSION, state=state), path)
    with pytest.raises(ValueError, match="format"):
        load_run(path)
    torch.save(dict(format=FORMAT, abi=L.ABI_VERSION - 1, state=state), path)
    with pytest.raises(ValueError, match="ABI"):
        load_run(path)
    torch.save([1, 2], path)
    with pytest.raises(ValueError, match="format"):
        load_run(path)


def test_a_failed_save_leaves_the_previous_file(tmp_path, monkeypatch):
    from armenv import checkpoint
    path = str(tmp_path / "run.ckpt")
    checkpoint.save_run(path, dict(iteration=1))
    with open(path, "rb") as fh:
        before = fh.read()

    def dies_midway(obj, f, *args, **kw):
        with open(f, "wb") as fh:
            fh.write(b"half a file")
        raise OSError("no space left on device")

    monkeypatch.setattr(checkpoint.torch, "save", dies_midway)
    with pytest.raises(OSError):
        checkpoint.save_run(path, dict(iteration=2))
    monkeypatch.undo()
    with open(path, "rb") as fh:
        assert fh.read() == before
    assert os.listdir(tmp_path) == ["run.ckpt"]
    assert checkpoint.load_run(path) == dict(iteration=1)


# ------------------------------------------------------------------------------------------------ save_best

def test_best_keeper_writes_at_the_first_rate_and_whenever_the_best_is_reached(tmp_path):
    from armenv.checkpoint import BestKeeper
    written = []
    keeper = BestKeeper(str(tmp_path / "agent"), write=lambda agent, filename: written.append((agent, filename)))
    rates = [0.0, 0.0, 0.25, 0.125, 0.25, 0.5, 0.375, float("nan"), 0.5]
    wrote = [keeper.offer(rate, k) for k, rate in enumerate(rates)]
    assert wrote == [True, True, True, False, True, True, False, False, True]
    assert written == [(k, str(tmp_path / "agent") + ".best") for k, w in enumerate(wrote) if w]
    assert keeper.state_dict() == dict(best=0.5)
    later = BestKeeper(str(tmp_path / "agent"), write=lambda *a: written.append(a))
    later.load_state_dict(keeper.state_dict())
    assert later.offer(0.375, None) is False and later.offer(0.5, None) is True
    real = BestKeeper(str(tmp_path / "real"))
    assert real.offer(0.0, _agent("fused", "td3"))
    assert sorted(os.listdir(tmp_path)) == ["real.best_actor.pt", "real.best_critic.pt"]


# ------------------------------------------------------------------------------------------------ what the loops refuse

REACH_CONFIG = dict(task="reach", algo="td3", learner="fused", num_envs=64, rollout_steps=8, updates=2, batch_size=64, her_ratio=0.8, seed=0,
                    actor_kind="actor_f16x3", expl_sigma=0.7 * 0.98, window_steps=16, minimal_episodes=5, max_steps=5)
REACH_CALL = dict(algo="td3", learner="fused", num_envs=64, rollout_steps=8, updates=2, batch_size=64, her_ratio=0.8, seed=0,
                  actor_kind="actor_f16x3", expl_sigma=0.7 * 0.98, window_steps=16, minimal_episodes=5, max_steps=5)
REACH_CHANGES = dict(algo="datd3", learner="hip", num_envs=32, rollout_steps=4, updates=3, batch_size=128, her_ratio=0.5, seed=1,
                     actor_kind="actor", expl_sigma=0.5, window_steps=32, minimal_episodes=4, max_steps=6)


def _checkpoint_with(tmp_path, config):
    from armenv.checkpoint import save_run
    path = str(tmp_path / "run.ckpt")
    save_run(path, dict(config=config, iteration=3))
    return path


@pytest.mark.parametrize("field", sorted(REACH_CHANGES))
def test_train_reach_refuses_a_resume_with_another_config(tmp_path, field):
    from armenv.train import train_reach
    path = _checkpoint_with(tmp_path, REACH_CONFIG)
    with pytest.raises(ValueError, match="resume: %s " % field):
        train_reach(**dict(REACH_CALL, device="cpu", iterations=0, resume=path, **{field: REACH_CHANGES[field]}))


def test_train_refuses_the_task_and_accepts_its_own_config(tmp_path):
    from armenv import _lib as L
    from armenv.train import train_push, train_reach
    path = _checkpoint_with(tmp_path, REACH_CONFIG)
    push = {k: v for k, v in REACH_CALL.items() if k != "expl_sigma"}
    with pytest.raises(ValueError, match="resume: task "):
        train_push(**dict(push, device="cpu", iterations=0, resume=path))
    # the same config with other iterations, log_every and paths passes the check: the loop gets as far as the device, which is none
    with pytest.raises(L.ArmEnvError):
        train_reach(**dict(REACH_CALL, device="cpu", iterations=9, log_every=3, resume=path, checkpoint=str(tmp_path / "other"), save=str(tmp_path / "a")))
    with pytest.raises(ValueError, match="format"):
        torch.save(dict(format=0), path)
        train_reach(**dict(REACH_CALL, device="cpu", iterations=0, resume=path))


POP_CALL = dict(members=3, num_envs=64, rollout_steps=8, updates=2, batch_size=64, her_ratio=0.8, seed=0, actor_kind="actor_f16x3",
                window_steps=16, minimal_episodes=5, max_steps=5, task="reach", algo="td3", store="population",
                sweep=dict(actor_lr=[1e-3, 5e-4, 2e-4]), pbt=dict(every=2))
POP_CHANGES = dict(members=4, num_envs=32, rollout_steps=4, updates=3, batch_size=128, her_ratio=0.5, seed=1, actor_kind="actor",
                   expl_sigma=0.5, window_steps=32, minimal_episodes=4, max_steps=6, task="push", algo="datd3", store="members",
                   sweep=dict(actor_lr=[1e-3, 5e-4, 1e-4]), pbt=dict(every=3))


def _pop_config():
    from armenv.pbt import PBTSchedule
    from armenv.train_pop import sweepable_names
    pbt = PBTSchedule(every=2, seed=0).bind(sweepable_names("td3")).state_dict()
    del pbt["rng"]
    config = {k: v for k, v in POP_CALL.items() if k != "pbt"}
    return dict(config, learner="fused", expl_sigma=0.7 * 0.98, pbt=pbt)


@pytest.mark.parametrize("field", sorted(POP_CHANGES))
def test_train_reach_population_refuses_a_resume_with_another_config(tmp_path, field):
    from armenv.train_pop import train_reach_population
    path = _checkpoint_with(tmp_path, _pop_config())
    call = dict(POP_CALL, **{field: POP_CHANGES[field]})
    if field == "members":
        call["sweep"] = dict(actor_lr=[1e-3, 5e-4, 2e-4, 1e-4])
    with pytest.raises(ValueError, match="resume: %s " % ("members" if field == "members" else field)):
        train_reach_population(**dict(call, device="cpu", iterations=0, resume=path))


def test_train_reach_population_accepts_its_own_config(tmp_path):
    from armenv import _lib as L
    from armenv.train_pop import train_reach_population
    path = _checkpoint_with(tmp_path, _pop_config())
    with pytest.raises(L.ArmEnvError):          # past the check: the population is made on the host, the first env needs a device
        train_reach_population(**dict(POP_CALL, device="cpu", iterations=9, log_every=3, resume=path))
    with pytest.raises(ValueError, match="resume: pbt "):
        train_reach_population(**dict(POP_CALL, device="cpu", iterations=0, resume=path, pbt=None))


def test_the_loops_refuse_what_cannot_be_checkpointed(tmp_path):
    from armenv.train import train_push, train_reach
    from armenv.train_pop import train_reach_population
    path = str(tmp_path / "run.ckpt")
    for kw in (dict(checkpoint=path), dict(resume=path)):
        with pytest.raises(ValueError, match="learner"):
            train_reach(device="cpu", iterations=0, learner="torch", **kw)
        with pytest.raises(ValueError, match="learner"):
            train_push(device="cpu", iterations=0, learner="torch", **kw)
    for train, kw in ((train_reach, dict(learner="fused")), (train_reach_population, {})):
        with pytest.raises(ValueError, match="checkpoint_every"):
            train(device="cpu", iterations=0, checkpoint_every=2, **kw)
        with pytest.raises(ValueError, match="checkpoint_every"):
            train(device="cpu", iterations=0, checkpoint=path, checkpoint_every=-1, **kw)
        with pytest.raises(ValueError, match="save_best"):
            train(device="cpu", iterations=0, save_best=True, **kw)
    assert not os.path.exists(path)


CLI_ERRORS = [
    ("armenv.train", ["--learner", "torch", "--checkpoint", "x.ckpt"], "learner"),
    ("armenv.train", ["--resume", "x.ckpt"], "learner"),
    ("armenv.train", ["--learner", "fused", "--checkpoint-every", "3"], "checkpoint_every"),
    ("armenv.train", ["--learner", "fused", "--save-best"], "save_best"),
    ("armenv.train", ["--learner", "fused", "--resume", "no/such/file.ckpt"], "no such file"),
    ("armenv.train_pop", ["--checkpoint-every", "3"], "checkpoint_every"),
    ("armenv.train_pop", ["--checkpoint", "x.ckpt", "--checkpoint-every", "-2"], "checkpoint_every"),
    ("armenv.train_pop", ["--save-best"], "save_best"),
    ("armenv.train_pop", ["--resume", "no/such/file.ckpt"], "no such file"),
]


@pytest.mark.parametrize("module,argv,message", CLI_ERRORS)
def test_cli_flag_errors(monkeypatch, capsys, module, argv, message):
    import importlib
    main = importlib.import_module(module).main
    monkeypatch.setattr(sys, "argv", [module] + argv)
    with pytest.raises(SystemExit) as err:
        main()
    assert err.value.code == 2 and re.search(message, capsys.readouterr().err)


@pytest.mark.parametrize("module", ["armenv.train", "armenv.train_pop"])
def test_cli_knows_the_flags(monkeypatch, capsys, module):
    import importlib
    monkeypatch.setattr(sys, "argv", [module, "--help"])
    with pytest.raises(SystemExit) as err:
        importlib.import_module(module).main()
    out = capsys.readouterr().out
    assert err.value.code == 0 and all(flag in out for flag in ("--checkpoint FILE", "--checkpoint-every N", "--resume FILE", "--save NAME", "--save-best"))
