"""The population trajectory store (armenv.replay.PopulationTrajectoryStore over armenv_pop_count_episodes, armenv_pop_write_episodes
and armenv_her_pop_sample) on cuda:0.  Its oracles: oracle.her on the CPU for the episode index and the reference's own draws, and
the single store -- armenv_count_episodes / armenv_write_episodes / armenv_her_sample on member p's arrays, seed + p and the same draw
-- which every member's slices must equal BIT FOR BIT.  The rings are filled from seeded numpy data; only the loop test creates
environments."""
import json

import numpy as np
import pytest
import torch

from conftest import golden_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RINGS = ("obs_after", "next_obs", "action", "reward", "done")
BATCH = ("states", "actions", "next_states", "rewards", "dones")
CAP = 40
SEED = 7


def _member_host(p, cap, N, D, T, base, empty=False):
    """Member p's arrays from np.random.default_rng(100 + p), drawn in LOGICAL time (step t lives in physical row (base + t) % cap;
    the rows beyond the window, t >= T, hold data of the same kind that nothing may read).  Episodes are 1 to 12 steps long (the shorter of two
    uniform draws: with uniform lengths, members 3 and 4 hold a single complete episode in a 23-step window of one env); the
    first three dims (the positions the relabelling compares) span 0.16, so that both sides of the 0.1 threshold occur.
    Returns (physical arrays as the ring holds them, the linear window [T] for the CPU oracle)."""
    rng = np.random.default_rng(100 + p)
    f = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)
    logical = dict(obs_after=f(cap, N, D), next_obs=f(cap, N, D), action=f(cap, N, 3), reward=f(cap, N))
    for k in ("obs_after", "next_obs"):
        logical[k][..., :3] *= 0.08
    done = np.zeros((cap, N), np.uint8)
    for n in range(N):
        t = -1
        while not empty:
            t += 1 + int(rng.integers(0, 12, 2).min())          # 1..12 steps, short ones more often
            if t >= cap:
                break
            done[t, n] = 1
    logical["done"] = done
    obs0 = f(N, D)
    obs0[..., :3] *= 0.08
    rows = (base + np.arange(cap)) % cap
    physical = {k: np.empty_like(v) for k, v in logical.items()}
    for k, v in logical.items():
        physical[k][rows] = v
    physical["obs0"] = obs0
    linear = {k: v[:T] for k, v in logical.items()}
    linear["obs0"] = obs0
    return physical, linear


def _store(P, N, D, T, base, at_reset, empty=(), cap=CAP):
    """a PopulationTrajectoryStore whose rings hold _member_host's arrays, indexed; and the members' linear windows"""
    from armenv.replay import PopulationTrajectoryStore
    st = PopulationTrajectoryStore(P, device=DEV, seed=SEED, capacity_steps=cap)
    r = st._allocate(N, D)
    host = [_member_host(p, cap, N, D, T, base, empty=p in empty) for p in range(P)]
    for k in RINGS + ("obs0",):
        r[k].copy_(torch.from_numpy(np.stack([h[0][k] for h in host])))
    r["base"], r["T"], r["at_reset"] = base, T, bool(at_reset)
    st._started = True
    st._index()
    return st, [h[1] for h in host]


def _single_on(st, p, reindex=False):
    """a TrajectoryStore with seed + p over member p's views; `reindex`: with its own episode index, from its own launches"""
    from armenv.replay import TrajectoryStore
    single = TrajectoryStore(device=DEV, seed=st.seed + p)
    view = st.member_view(p)
    if reindex:
        del view["episodes"], view["num_episodes"]
        single._ring = view
        single._index()
    else:
        single.chunk = view
    return single


def _complete_episodes(linear, at_reset):
    from oracle import her
    return her.index_episodes(linear["done"], starts_at_reset=bool(at_reset))


# ------------------------------------------------------------------------------------------------ C1

@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("P", [1, 2, 5])
def test_every_members_index_is_the_single_index(P, N):
    for T, base in ((40, 0), (40, 31), (23, 0), (23, 31)):
        for at_reset in (0, 1):
            st, linear = _store(P, N, 6, T, base, at_reset)
            sizes = st.sizes()
            assert len(sizes) == P and st.ready(2) and not st.ready(max(sizes) + 1)
            for p in range(P):
                ref = _complete_episodes(linear[p], at_reset)
                assert len(ref) >= 2, (p, T, base, at_reset)          # the shared inputs' precondition
                assert sizes[p] == len(ref), (p, T, base, at_reset)
                mine = st._ring["episodes"][p, : sizes[p]]
                assert np.array_equal(mine.cpu().numpy(), ref), (p, T, base, at_reset)
                single = _single_on(st, p, reindex=True)
                assert single.size() == sizes[p]
                assert torch.equal(single.chunk["episodes"][: sizes[p]], mine), (p, T, base, at_reset)


# ------------------------------------------------------------------------------------------------ C2

def _assert_members_equal_single(st, out, draw, B, use_her, members):
    for p in members:
        single = _single_on(st, p)
        single._draw = draw
        ref = single.sample(B, use_her=use_her, her_ratio=0.8, return_picks=True)
        for k in BATCH + ("picks",):
            assert torch.equal(out[k][p], ref[k]), (p, k, draw, use_her)


@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [1, 257, 1000])
@pytest.mark.parametrize("P", [1, 2, 5])
def test_every_members_batch_is_the_single_sample_bit_for_bit(P, B, D):
    st, linear = _store(P, 3, D, 40, 31, 0)
    assert all(len(_complete_episodes(w, 0)) >= 2 for w in linear)
    seen = []
    for use_her in (True, False):
        for _ in range(2):                                            # two consecutive draws
            draw = st._draw
            out = st.sample(B, use_her=use_her, her_ratio=0.8, return_picks=True)
            assert st._draw == draw + 1
            assert all(tuple(out[k].shape[:2]) == (P, B) for k in BATCH + ("picks",))
            _assert_members_equal_single(st, out, draw, B, use_her, range(P))
            seen.append({k: out[k].clone() for k in BATCH + ("picks",)})
    if B >= 257:
        pk = seen[0]["picks"]
        assert 0 < int(pk[..., 2].sum()) < pk[..., 2].numel() and int(seen[2]["picks"][..., 2].sum()) == 0
        assert 0 < int(seen[0]["dones"].sum()) < seen[0]["dones"].numel()
        assert not torch.equal(seen[0]["picks"], seen[1]["picks"])   # the draw counter moved
        if P > 1:
            assert not torch.equal(seen[0]["picks"][0], seen[0]["picks"][1])     # seed + p


# ------------------------------------------------------------------------------------------------ C3

@pytest.mark.parametrize("D", [6, 9])
def test_an_empty_member_gets_the_inert_batch_and_disturbs_nobody(D):
    B = 257
    st, linear = _store(3, 3, D, 40, 31, 0, empty=(1,))
    full, _ = _store(3, 3, D, 40, 31, 0)
    assert st.sizes()[1] == 0 and int(st._ring["done"][1].sum()) == 0 and not st.ready(1)
    assert len(_complete_episodes(linear[0], 0)) >= 2 and len(_complete_episodes(linear[2], 0)) >= 2
    for use_her in (True, False):
        draw = full._draw = st._draw
        out = dict(states=torch.full((3, B, D), 3.0, device=DEV), actions=torch.full((3, B, 3), 3.0, device=DEV),
                   next_states=torch.full((3, B, D), 3.0, device=DEV), rewards=torch.full((3, B), 3.0, device=DEV),
                   dones=torch.full((3, B), 3, dtype=torch.uint8, device=DEV),
                   picks=torch.full((3, B, 4), 3, dtype=torch.int32, device=DEV))                  # stale data to overwrite
        out = st.sample(B, use_her=use_her, her_ratio=0.8, out=out, return_picks=True)
        ref = full.sample(B, use_her=use_her, her_ratio=0.8, return_picks=True)
        for k in ("states", "next_states", "actions", "rewards"):
            assert float(out[k][1].abs().max()) == 0.0, k
        assert bool((out["dones"][1] == 1).all())
        assert bool((out["picks"][1] == torch.tensor([-1, 0, 0, 0], dtype=torch.int32, device=DEV)).all())
        _assert_members_equal_single(st, out, draw, B, use_her, (0, 1, 2))    # the single sampler's inert batch is the same one
        for p in (0, 2):
            for k in BATCH + ("picks",):
                assert torch.equal(out[k][p], ref[k][p]), (p, k)


# ------------------------------------------------------------------------------------------------ C4

@pytest.mark.parametrize("task", ["reach", "push"])
def test_every_member_reproduces_the_references_own_draws(task):
    """test_her_sampler_matches_reference_golden's check and bounds for three members: the golden chunk, the same chunk with the batch
    order of its picks reversed, and the chunk again -- fed through the store's own path (staging block, add_rollouts)."""
    from armenv.replay import PopulationTrajectoryStore
    g = golden_npz(f"her_{task}_seed0.npz")
    T, N, D = g["obs_after"].shape
    P, B = 3, len(g["picks"])
    st = PopulationTrajectoryStore(P, device=DEV, seed=5, capacity_steps=T)
    bufs = st.rollout_buffers(T, N, D)
    for p in range(P):
        for dst, src in (("obs", "obs_after"), ("terminal_obs", "next_obs"), ("actions", "action"), ("reward", "reward"), ("done_u8", "done")):
            bufs[p][dst].copy_(torch.from_numpy(g[src]))
    st.add_rollouts(torch.from_numpy(np.stack([g["obs0"]] * P)).to(DEV), starts_at_reset=True)
    assert st.sizes() == [len(g["episodes"])] * P
    order = [np.arange(B), np.arange(B)[::-1].copy(), np.arange(B)]
    picks = np.stack([g["picks"][o] for o in order])
    out = st.sample(B, use_her=True, dis_threshold=float(g["dis_threshold"]), her_ratio=float(g["her_ratio"]), picks=picks,
                    return_picks=True)
    for p in range(P):
        o = order[p]
        assert np.array_equal(st._ring["episodes"][p, : len(g["episodes"])].cpu().numpy(), g["episodes"])
        got = {k: out[k][p].cpu().numpy() for k in BATCH + ("picks",)}
        assert np.array_equal(got["picks"], g["picks"][o])
        assert np.array_equal(got["states"].astype(np.float64), g["states"][o])
        assert np.array_equal(got["next_states"].astype(np.float64), g["next_states"][o])
        assert np.array_equal(got["actions"], g["actions"][o]) and np.array_equal(got["dones"], g["dones"][o])
        assert np.abs(got["rewards"].astype(np.float64) - g["rewards"][o]).max() < 1e-7


# ------------------------------------------------------------------------------------------------ C5

GUARD = 64          # canary elements on either side


def _guarded(t, guards):
    """`t`'s contents in the middle of a larger allocation whose two margins hold a canary pattern; the margins are recorded"""
    big = torch.empty(t.numel() + 2 * GUARD, dtype=t.dtype, device=t.device)
    canary = torch.arange(2 * GUARD, device=t.device) % 97 + 13
    big[:GUARD] = canary[:GUARD].to(t.dtype)
    big[-GUARD:] = canary[GUARD:].to(t.dtype)
    inner = big[GUARD:GUARD + t.numel()].view(t.shape)
    inner.copy_(t)
    guards.append((big, torch.cat([big[:GUARD], big[-GUARD:]]).clone()))
    return inner


def _guards_intact(guards):
    return all(torch.equal(torch.cat([big[:GUARD], big[-GUARD:]]), was) for big, was in guards)


def test_nothing_is_written_outside_the_stores_arrays():
    from armenv.replay import PopulationTrajectoryStore
    P, B, N, D, Tc = 3, 257, 3, 6, 25
    guards = []
    st = PopulationTrajectoryStore(P, device=DEV, seed=SEED, capacity_steps=CAP)
    st.rollout_buffers(Tc, N, D)
    st._staging = {k: _guarded(t, guards) for k, t in st._staging.items()}
    r = st._allocate(N, D)
    for k, t in list(r.items()):
        if torch.is_tensor(t):
            r[k] = _guarded(t, guards)
    out = dict(states=torch.zeros(P, B, D), actions=torch.zeros(P, B, 3), next_states=torch.zeros(P, B, D), rewards=torch.zeros(P, B),
               dones=torch.zeros(P, B, dtype=torch.uint8), picks=torch.zeros(P, B, 4, dtype=torch.int32))
    out = {k: _guarded(t.to(DEV), guards) for k, t in out.items()}
    pointers = {k: t.data_ptr() for k, t in out.items()}
    assert len(guards) == 6 + 10 + 6
    obs0 = torch.rand(P, N, D, device=DEV)
    for chunk in range(2):                                            # the second chunk drops 10 steps and wraps
        for p in range(P):
            host, _ = _member_host(p + 10 * chunk, Tc, N, D, Tc, 0)
            for dst, src in (("obs", "obs_after"), ("terminal_obs", "next_obs"), ("actions", "action"), ("reward", "reward"), ("done_u8", "done")):
                st._staging[dst][p].copy_(torch.from_numpy(host[src]))
        r["episodes"].fill_(-77)
        st.add_rollouts(obs0, starts_at_reset=(chunk == 0))
        sizes = st.sizes()
        assert min(sizes) >= 2
        for p in range(P):
            assert bool((r["episodes"][p, sizes[p]:] == -77).all()) and bool((r["episodes"][p, : sizes[p]] != -77).all())
        for use_her in (True, False):
            draw = st._draw
            got = st.sample(B, use_her=use_her, her_ratio=0.8, out=out, return_picks=True)
            assert got is out and {k: t.data_ptr() for k, t in out.items()} == pointers        # written in place, picks included
            _assert_members_equal_single(st, out, draw, B, use_her, range(P))
        assert _guards_intact(guards), chunk
    assert (r["base"], r["T"], r["at_reset"]) == (10, 40, False)


# ------------------------------------------------------------------------------------------------ C6

def test_the_same_call_gives_the_same_bytes_on_any_stream():
    P, B = 3, 257
    st, _ = _store(P, 3, 9, 40, 31, 0)
    runs = []
    side = torch.cuda.Stream(device=DEV)
    for where in ("current", "current", "side"):
        st._draw = 4
        if where == "side":
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                st._ring["episodes"].fill_(-1)
                st._index()
                out = st.sample(B, use_her=True, her_ratio=0.8, return_picks=True)
            side.synchronize()
        else:
            out = st.sample(B, use_her=True, her_ratio=0.8, return_picks=True)
        torch.cuda.synchronize()
        runs.append(dict(out, episodes=st._ring["episodes"].clone(), num_episodes=st._ring["num_episodes"].clone()))
    sizes = st.sizes()
    for other in runs[1:]:
        for k in BATCH + ("picks", "num_episodes"):
            assert torch.equal(runs[0][k].view(torch.uint8), other[k].view(torch.uint8)), k
        for p in range(P):
            assert torch.equal(runs[0]["episodes"][p, : sizes[p]], other["episodes"][p, : sizes[p]])


# ------------------------------------------------------------------------------------------------ C7

@pytest.mark.parametrize("algo", ["td3", "daddpg"])
def test_the_loop_trains_the_same_bits_with_either_store(algo):
    """armenv.train_pop with store="members" and store="population": every tensor of the population's stacks and every history record
    (but its wall time) are equal.  log_every = 2 only adds records to compare."""
    from armenv.train_pop import train_reach_population
    runs = {}
    for store in ("members", "population"):
        lines = []
        pop, history = train_reach_population(members=3, num_envs=64, iterations=12, rollout_steps=32, updates=4, batch_size=64,
                                              max_steps=20, seed=5, algo=algo, store=store, device=DEV, log_every=2, log=lines.append)
        assert len(history) == 6 and [json.loads(l)["iteration"] for l in lines] == [2, 4, 6, 8, 10, 12]
        runs[store] = (pop, [{k: v for k, v in rec.items() if k != "wall_s"} for rec in history])
    (a, ha), (b, hb) = runs["members"], runs["population"]
    assert a.total_it == b.total_it and a.total_it >= 8 * 4          # precondition: updates ran in at least 8 of the 12 iterations
    assert ha == hb
    assert sorted(a.stacks) == sorted(b.stacks)
    for name in a.stacks:
        for x, y in zip(a.stacks[name], b.stacks[name]):
            assert torch.equal(x, y), name


# ------------------------------------------------------------------------------------------------ C8

@pytest.mark.parametrize("D", [6, 9])
def test_the_single_store_hands_the_single_entry_point_its_arguments(D):
    """armenv_her_sample called through ctypes with an ArmEnvHerArgs filled here by hand, against TrajectoryStore.sample over the same
    ring (N = 3, cap 40, a wrapped window of 23 steps that starts mid-episode): the same bytes.  The store's second draw goes into the
    first one's `out`, so it runs on the kept argument struct and writes `picks` in place."""
    import ctypes as C

    from armenv import _lib as L
    from armenv.replay import TrajectoryStore
    st, linear = _store(1, 3, D, 23, 31, 0)
    assert len(_complete_episodes(linear[0], 0)) >= 2                 # the shared inputs' precondition
    view = st.member_view(0)
    lib, stream = L.load(), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for B in (1, 257):
        for use_her in (True, False):
            single = TrajectoryStore(device=DEV, seed=SEED)
            single.chunk = view
            got = None
            for d in (0, 1):
                ref = dict(states=torch.full((B, D), 3.0, device=DEV), actions=torch.full((B, 3), 3.0, device=DEV),
                           next_states=torch.full((B, D), 3.0, device=DEV), rewards=torch.full((B,), 3.0, device=DEV),
                           dones=torch.full((B,), 3, dtype=torch.uint8, device=DEV),
                           picks=torch.full((B, 4), 3, dtype=torch.int32, device=DEV))
                a = L.ArmEnvHerArgs()
                a.T, a.N, a.ring_base, a.ring_cap, a.obs_dim, a.use_her = 23, 3, 31, CAP, D, int(use_her)
                a.obs0_dev, a.obs_after_dev, a.next_obs_dev = view["obs0"].data_ptr(), view["obs_after"].data_ptr(), view["next_obs"].data_ptr()
                a.action_dev, a.reward_dev, a.done_dev = view["action"].data_ptr(), view["reward"].data_ptr(), view["done"].data_ptr()
                a.episodes_dev, a.num_episodes_dev = view["episodes"].data_ptr(), view["num_episodes"].data_ptr()
                a.batch, a.picks_dev, a.seed, a.draw, a.her_ratio, a.dis_threshold = B, None, SEED, d, 0.8, 0.1
                a.states_dev, a.actions_dev, a.next_states_dev = ref["states"].data_ptr(), ref["actions"].data_ptr(), ref["next_states"].data_ptr()
                a.rewards_dev, a.dones_dev, a.picks_out_dev = ref["rewards"].data_ptr(), ref["dones"].data_ptr(), ref["picks"].data_ptr()
                L.check(lib.armenv_her_sample(0, C.byref(a), stream))
                single._draw = d
                picks = None if got is None else got["picks"].data_ptr()
                got = single.sample(B, use_her=use_her, her_ratio=0.8, return_picks=True, out=got)
                assert single._draw == d + 1 and picks in (None, got["picks"].data_ptr())
                for k in BATCH + ("picks",):
                    assert torch.equal(got[k], ref[k]), (B, use_her, d, k)
