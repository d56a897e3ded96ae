"""CPU tests of the host side of the population trajectory store (armenv_her_pop_sample, armenv_pop_count_episodes,
armenv_pop_write_episodes, include/armenv.h; armenv.replay.PopulationTrajectoryStore): the ctypes struct agrees with the header, every
argument is refused before any HIP call -- by the single entry points too, which run the same checks --, the population kernels are
in the built code object without scratch or LDS, the stacked rings keep TrajectoryStore's books, and both stores' host side
(armenv.replay._Store) keeps its contracts on device="cpu"."""
import ctypes as C

import pytest
import torch

from learner_host import all_kernels, ctypes_layout, header_layout, refused as _refused

POINTERS = ("obs0_dev", "obs_after_dev", "next_obs_dev", "action_dev", "reward_dev", "done_dev", "episodes_dev", "num_episodes_dev",
            "states_dev", "actions_dev", "next_states_dev", "rewards_dev", "dones_dev")


# ------------------------------------------------------------------------------------------------ H1: ABI layout

def test_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = ctypes_layout(L.ArmEnvHerPopArgs)
    assert [m for m, _ in members][-2:] == ["members", "episodes_stride"] and ("one.picks_out_dev", L.ArmEnvHerArgs.picks_out_dev.offset) in members
    sizes, offsets = header_layout(L.ArmEnvHerPopArgs, extra=("sizeof(ArmEnvHerArgs)",))
    assert sizes == [C.sizeof(L.ArmEnvHerPopArgs), C.sizeof(L.ArmEnvHerArgs)]
    assert offsets == [o for _, o in members], members
    assert L.ArmEnvHerPopArgs.members.offset == C.sizeof(L.ArmEnvHerArgs)


def test_the_symbols_resolve_and_the_abi_version_did_not_move():
    from armenv import _lib as L
    lib = L.load()
    assert lib.armenv_abi_version() == 9 and L.ABI_VERSION == 9
    for name in ("armenv_her_pop_sample", "armenv_pop_count_episodes", "armenv_pop_write_episodes"):
        assert name in L.SYMBOLS and getattr(lib, name) is not None


# ------------------------------------------------------------------------------------------------ H2: refusals

def _args(P=3, B=64, D=6):
    """Arguments that pass every check but the one a test breaks: fake (never dereferenced) device pointers.
    NOT to be passed unmodified -- a valid set would be enqueued."""
    from armenv import _lib as L
    pa = L.ArmEnvHerPopArgs()
    pa.members, pa.episodes_stride = P, 40 * 8
    a = pa.one
    a.T, a.N, a.ring_base, a.ring_cap, a.obs_dim, a.use_her, a.batch = 23, 8, 31, 40, D, 1, B
    a.her_ratio, a.dis_threshold, a.seed, a.draw = 0.8, 0.1, 5, 0
    for k, name in enumerate(POINTERS):
        setattr(a, name, 0x10000000 + 0x1000000 * k)
    return pa


def _one(field, value):
    return lambda pa: setattr(pa.one, field, value)


SAMPLE_REFUSALS = [
    ("members", lambda pa: setattr(pa, "members", 0)),
    ("members", lambda pa: setattr(pa, "members", 65)),
    ("members", lambda pa: setattr(pa, "members", -1)),
    ("episodes_stride", lambda pa: setattr(pa, "episodes_stride", 0)),
    ("episodes_stride", lambda pa: setattr(pa, "episodes_stride", -3)),
    ("obs_dim", _one("obs_dim", 7)),
    ("obs_dim", _one("obs_dim", 0)),
    ("batch", _one("batch", -1)),
    ("T", _one("T", 0)),
    ("N", _one("N", 0)),
    ("ring_cap", _one("ring_cap", 22)),
    ("ring_base", _one("ring_base", -1)),
    ("her_ratio", _one("her_ratio", 1.5)),
    ("her_ratio", _one("her_ratio", -0.1)),
    ("her_ratio", _one("her_ratio", float("nan"))),
] + [(name, _one(name, None)) for name in POINTERS]


@pytest.mark.parametrize("field,mutate", SAMPLE_REFUSALS)
def test_bad_sample_arguments_are_refused_before_any_device_call(field, mutate):
    pa = _args()
    mutate(pa)
    assert field in _refused("armenv_her_pop_sample", 0, C.byref(pa), None)


def test_null_sample_args_are_refused():
    assert "args" in _refused("armenv_her_pop_sample", 0, None, None)


@pytest.mark.parametrize("members", [1, 64])
def test_the_member_bounds_are_accepted(members):
    """1 and 64 pass the `members` check: the call is then refused for the next broken field, still before any device call; and an
    empty batch is ARMENV_OK without a launch."""
    from armenv import _lib as L
    pa = _args(P=members)
    pa.one.obs_dim = 7
    assert "obs_dim" in _refused("armenv_her_pop_sample", 0, C.byref(pa), None)
    pa = _args(P=members, B=0)
    assert L.load().armenv_her_pop_sample(0, C.byref(pa), None) == 0


GOOD_INDEX = dict(members=3, T=23, N=8, ring_base=31, ring_cap=40, done=0x10000000, counts=0x20000000, offsets=0x30000000,
                  episodes=0x40000000, stride=320)
INDEX_REFUSALS = [("members", dict(members=0)), ("members", dict(members=65)), ("T", dict(T=-1)), ("N", dict(N=0)),
                  ("ring_cap", dict(ring_cap=22)), ("ring_cap", dict(T=0, ring_cap=0)), ("ring_base", dict(ring_base=-1)),
                  ("done_dev", dict(done=None)), ("counts_dev", dict(counts=None))]


@pytest.mark.parametrize("field,change", INDEX_REFUSALS)
def test_bad_count_arguments_are_refused_before_any_device_call(field, change):
    g = dict(GOOD_INDEX, **change)
    assert field in _refused("armenv_pop_count_episodes", 0, g["members"], g["T"], g["N"], g["ring_base"], g["ring_cap"], g["done"], 1,
                             g["counts"], None)


@pytest.mark.parametrize("field,change", INDEX_REFUSALS + [("offsets_dev", dict(offsets=None)), ("episodes_dev", dict(episodes=None)),
                                                           ("episodes_stride", dict(stride=0))])
def test_bad_write_arguments_are_refused_before_any_device_call(field, change):
    g = dict(GOOD_INDEX, **change)
    assert field in _refused("armenv_pop_write_episodes", 0, g["members"], g["T"], g["N"], g["ring_base"], g["ring_cap"], g["done"], 1,
                             g["counts"], g["offsets"], g["episodes"], g["stride"], None)


# The single entry points run the same checks with members = 1: the tables above without their `members` / `episodes_stride` rows.
SINGLE_SAMPLE_REFUSALS = [row for row in SAMPLE_REFUSALS if row[0] not in ("members", "episodes_stride")]
SINGLE_INDEX_REFUSALS = [row for row in INDEX_REFUSALS if row[0] != "members"]


@pytest.mark.parametrize("field,mutate", SINGLE_SAMPLE_REFUSALS)
def test_the_single_sample_refuses_the_same_fields_before_any_device_call(field, mutate):
    pa = _args()
    mutate(pa)
    assert field in _refused("armenv_her_sample", 0, C.byref(pa.one), None)


def test_the_single_sample_refuses_null_args_and_accepts_an_empty_batch():
    from armenv import _lib as L
    assert "args" in _refused("armenv_her_sample", 0, None, None)
    pa = _args(B=0)
    assert L.load().armenv_her_sample(0, C.byref(pa.one), None) == 0


@pytest.mark.parametrize("field,change", SINGLE_INDEX_REFUSALS)
def test_the_single_count_refuses_the_same_fields_before_any_device_call(field, change):
    g = dict(GOOD_INDEX, **change)
    assert field in _refused("armenv_count_episodes", 0, g["T"], g["N"], g["ring_base"], g["ring_cap"], g["done"], 1, g["counts"], None)


@pytest.mark.parametrize("field,change", SINGLE_INDEX_REFUSALS + [("offsets_dev", dict(offsets=None)), ("episodes_dev", dict(episodes=None))])
def test_the_single_write_refuses_the_same_fields_before_any_device_call(field, change):
    g = dict(GOOD_INDEX, **change)
    assert field in _refused("armenv_write_episodes", 0, g["T"], g["N"], g["ring_base"], g["ring_cap"], g["done"], 1, g["counts"],
                             g["offsets"], g["episodes"], None)


# ------------------------------------------------------------------------------------------------ H3: kernels present

@pytest.fixture(scope="module")
def store_kernels():
    return {dm.replace("void ", "").split("(")[0].replace("armenv::", ""): (md, ins) for _, dm, md, ins in all_kernels()
            if "her_sample" in dm or "index_episodes" in dm}


def test_population_store_kernels_are_in_the_code_object(store_kernels):
    want = ("her_sample_pop_kernel<6>", "her_sample_pop_kernel<9>", "index_episodes_pop_kernel")
    assert set(want) <= set(store_kernels), sorted(store_kernels)
    assert {"her_sample_kernel<6>", "her_sample_kernel<9>", "index_episodes_kernel"} <= set(store_kernels)
    for k in want:
        md, ins = store_kernels[k]
        assert md["scratch"] == 0 and md["lds"] == 0 and md["spill_vgpr"] == 0 and len(ins) > 0, (k, md)
        mnems = {i.mnem for i in ins}
        assert not any("atomic" in m or m.startswith(("ds_", "scratch_")) for m in mnems), (k, sorted(mnems))


# ------------------------------------------------------------------------------------------------ H4: ring bookkeeping

def test_ring_append_is_the_window_arithmetic():
    from armenv.replay import ring_append
    assert ring_append(80, 0, 0, True, 25) == (0, 25, True, [(0, 0, 25)])
    assert ring_append(80, 0, 75, True, 25) == (20, 80, False, [(75, 0, 5), (0, 5, 20)])
    assert ring_append(80, 20, 80, False, 25) == (45, 80, False, [(20, 0, 25)])
    assert ring_append(40, 0, 0, False, 40) == (0, 40, False, [(0, 0, 40)])


def test_population_rings_keep_the_single_stores_books(monkeypatch):
    """Six chunks of 25 steps through cap = 80, on the host (the index launches are left out): after every chunk the population
    store's base, T and at_reset are TrajectoryStore's, and every member's ring rows are the rows that member's own store holds."""
    from armenv import replay
    monkeypatch.setattr(replay.TrajectoryStore, "_index", lambda self: None)
    monkeypatch.setattr(replay.PopulationTrajectoryStore, "_index", lambda self: None)
    P, N, D, Tc, cap = 3, 4, 6, 25, 80
    pop = replay.PopulationTrajectoryStore(P, device="cpu", seed=0, capacity_steps=cap)
    singles = [replay.TrajectoryStore(device="cpu", seed=p, capacity_steps=cap) for p in range(P)]
    bufs = pop.rollout_buffers(Tc, N, D)
    assert all(set(b) == {"obs", "reward", "done_u8", "success_u8", "actions", "terminal_obs"} for b in bufs)
    assert all(t.is_contiguous() and t.shape[:2] == (Tc, N) for b in bufs for t in b.values())
    assert bufs[1]["obs"].data_ptr() == pop._staging["obs"][1].data_ptr()
    gen = torch.Generator().manual_seed(3)
    obs0 = torch.rand(P, N, D, generator=gen)
    seen = []
    for chunk in range(6):
        for p in range(P):
            for k, t in bufs[p].items():
                t.copy_(torch.rand(t.shape, generator=gen) if t.dtype == torch.float32 else (torch.rand(t.shape, generator=gen) < 0.2))
            singles[p].add_rollout(obs0[p], bufs[p], starts_at_reset=(chunk == 0))
        pop.add_rollouts(obs0, starts_at_reset=(chunk == 0))
        r = pop._ring
        for p, s in enumerate(singles):
            view = pop.member_view(p)
            assert (view["cap"], view["base"], view["T"], view["at_reset"], view["N"], view["D"]) == \
                   (s._ring["cap"], s._ring["base"], s._ring["T"], s._ring["at_reset"], N, D), (chunk, p)
            rows = [(r["base"] + t) % cap for t in range(r["T"])]
            for k in ("obs_after", "next_obs", "action", "reward", "done"):
                assert torch.equal(view[k][rows], s._ring[k][rows]), (chunk, p, k)
                assert view[k].data_ptr() == r[k][p].data_ptr()
            assert torch.equal(view["obs0"], s._ring["obs0"])
        seen.append((r["base"], r["T"], r["at_reset"]))
    assert seen == [(0, 25, True), (0, 50, True), (0, 75, True), (20, 80, False), (45, 80, False), (70, 80, False)]


# ------------------------------------------------------------------------------------------------ H5: one code path

@pytest.fixture
def unindexed(monkeypatch):
    """armenv.replay with the index launches left out, so that the stores' host side runs on the cpu device"""
    from armenv import replay
    monkeypatch.setattr(replay.TrajectoryStore, "_index", lambda self: None)
    monkeypatch.setattr(replay.PopulationTrajectoryStore, "_index", lambda self: None)
    return replay


def _rollout(gen, lead, Tc, N, D):
    f = lambda *shape: torch.rand(lead + shape, generator=gen)
    return dict(obs=f(Tc, N, D), terminal_obs=f(Tc, N, D), actions=f(Tc, N, 3), reward=f(Tc, N), done_u8=(f(Tc, N) < 0.3).to(torch.uint8))


def test_a_store_without_capacity_holds_the_rollouts_own_tensors(unindexed):
    Tc, N, D = 7, 3, 6
    gen = torch.Generator().manual_seed(4)
    out, obs0 = _rollout(gen, (), Tc, N, D), torch.rand(N, D, generator=gen)
    st = unindexed.TrajectoryStore(device="cpu")
    assert st.chunk is None and st.capacity is None
    st.add_rollout(obs0, out, starts_at_reset=False)
    ch = st.chunk
    assert (ch["cap"], ch["base"], ch["T"]) == (Tc, 0, Tc) and (ch["N"], ch["D"], ch["at_reset"]) == (N, D, False)
    for ring, src in (("obs_after", "obs"), ("next_obs", "terminal_obs"), ("action", "actions"), ("reward", "reward"), ("done", "done_u8")):
        assert ch[ring].data_ptr() == out[src].data_ptr(), ring
    assert ch["obs0"].data_ptr() == obs0.data_ptr()


def test_host_trajectories_join_the_ring_with_their_own_first_state(unindexed):
    """Episodes of 3 and 2 steps: the second one's first state stands where the sampler looks for it, in obs_after at the first
    episode's last row, and that row's next_obs -- the first episode's own last state -- is not touched."""
    D = 6
    gen = torch.Generator().manual_seed(5)
    episodes = []
    for length in (3, 2):
        states = torch.rand(length + 1, D, generator=gen)
        traj = unindexed.Trajectory(states[0].numpy())
        for t in range(length):
            traj.store_step(torch.rand(3, generator=gen).numpy(), states[t + 1].numpy(), -0.1 * (t + 1), t == length - 1)
        episodes.append((traj, states))
    st = unindexed.TrajectoryStore(device="cpu", capacity_steps=8)
    st.add_trajectory(episodes[0][0])
    r = st.chunk
    assert (r["T"], r["at_reset"]) == (3, True) and torch.equal(r["obs_after"][:3, 0], episodes[0][1][1:])
    st.add_trajectory(episodes[1][0])
    assert st.chunk is r and (r["cap"], r["base"], r["T"], r["N"], r["at_reset"]) == (8, 0, 5, 1, True)
    assert torch.equal(r["obs_after"][2, 0], episodes[1][1][0])                # the second episode's first state
    assert torch.equal(r["next_obs"][2, 0], episodes[0][1][3])                 # the first episode's last state
    assert torch.equal(r["obs_after"][3:5, 0], episodes[1][1][1:]) and torch.equal(r["next_obs"][3:5, 0], episodes[1][1][1:])
    assert torch.equal(r["obs0"][0], episodes[0][1][0])
    assert r["done"][:5, 0].tolist() == [0, 0, 1, 0, 1] and torch.equal(r["reward"][:5, 0], torch.tensor([-0.1, -0.2, -0.3, -0.1, -0.2]))


@pytest.mark.parametrize("population", [False, True])
def test_sample_refuses_a_missing_rollout_and_unfit_out_tensors(unindexed, population):
    import re
    B, N, D, Tc = 4, 2, 6, 5
    gen = torch.Generator().manual_seed(6)
    if population:
        st, lead = unindexed.PopulationTrajectoryStore(3, device="cpu", capacity_steps=8), (3,)
    else:
        st, lead = unindexed.TrajectoryStore(device="cpu", capacity_steps=8), ()
    name = type(st).__name__
    with pytest.raises(RuntimeError, match=re.escape(name + ".sample: no rollout stored")):
        st.sample(B)
    if population:
        st.rollout_buffers(Tc, N, D)
        for k, t in _rollout(gen, lead, Tc, N, D).items():
            st._staging[k].copy_(t)
        st.add_rollouts(torch.rand(3, N, D, generator=gen))
    else:
        st.add_rollout(torch.rand(N, D, generator=gen), _rollout(gen, lead, Tc, N, D))
    assert st.chunk["T"] == Tc
    unfit = dict(states=torch.zeros(lead + (B, 2 * D))[..., ::2],              # the right shape, not contiguous
                 dones=torch.zeros(lead + (B,)),                               # the wrong dtype
                 rewards=torch.zeros(lead + (B, 1)))                           # the wrong shape
    assert tuple(unfit["states"].shape) == lead + (B, D) and not unfit["states"].is_contiguous()
    for key, tensor in unfit.items():
        out = dict(states=torch.zeros(lead + (B, D)), actions=torch.zeros(lead + (B, 3)), next_states=torch.zeros(lead + (B, D)),
                   rewards=torch.zeros(lead + (B,)), dones=torch.zeros(lead + (B,), dtype=torch.uint8))
        out[key] = tensor
        with pytest.raises(ValueError, match=re.escape(f"{name}.sample: out[{key!r}] must be a contiguous")):
            st.sample(B, out=out)
    assert st._draw == 0 and st._bound is None                                 # a refused call draws nothing and binds nothing


def test_population_store_refuses_unsupported_construction():
    from armenv.replay import PopulationTrajectoryStore
    for kw in (dict(members=0), dict(members=65), dict(members=2, capacity_steps=None)):
        with pytest.raises(ValueError):
            PopulationTrajectoryStore(**dict(dict(members=2, device="cpu", capacity_steps=8), **kw))
    st = PopulationTrajectoryStore(2, device="cpu", capacity_steps=8)
    assert st.sizes() == [0, 0] and not st.ready(1)
    with pytest.raises(RuntimeError):
        st.sample(4)
    with pytest.raises(RuntimeError):
        st.add_rollouts(torch.zeros(2, 1, 6))
    st.rollout_buffers(9, 1, 6)
    with pytest.raises(ValueError):
        st.add_rollouts(torch.zeros(2, 1, 6))            # a chunk longer than the ring


def test_train_pop_knows_both_stores():
    from armenv.train_pop import STORES, train_reach_population
    assert STORES == ("population", "members")
    with pytest.raises(ValueError):
        train_reach_population(members=1, iterations=0, store="shared")
