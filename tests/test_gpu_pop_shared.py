"""The shared population sampler (armenv_her_pop_sample_shared; PopulationTrajectoryStore.sample(share_ratio=...); armenv.train_pop's
share_ratio) on cuda:0, every comparison BIT FOR BIT (floats as int32).  Its oracles are the kernels it generalises:

  share_ratio = 0   armenv_her_pop_sample on the same arrays (picks: the member in front of that call's four);
  share_ratio = 1   armenv_her_sample with seed + p and the same draw on the MERGED ring -- the members' rings permuted to
                    [cap][P N][...], obs0 [P N][D], indexed by armenv_count_episodes / armenv_write_episodes: the single index lists
                    the episodes env-major and column m N + n is member m's column n, so its episode number is the shared pick's
                    episode + E_0 + ... + E_(m-1);
  in between        row by row the one or the other, told apart by the host model's u4 (tests/pop_shared_cases.py).

The rings are tests/test_gpu_pop_store.py's (seeded numpy data, episodes of 1 to 12 steps, every member its own values) in a full
window that wraps (ring_base 31 of 40) and starts mid-episode.  Only the loop tests create environments."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pop_shared_cases as S
from test_gpu_checkpoint import _abc, _tensors_equal, recorder  # noqa: F401  (recorder: a fixture)
from test_gpu_pop_store import BATCH, DEV, RINGS, _guarded, _guards_intact, _store

pytestmark = pytest.mark.gpu
KEYS = BATCH + ("picks",)
INERT = torch.tensor(S.INERT, dtype=torch.int32)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(x, y):
    return torch.equal(_bits(x), _bits(y))


def _new_out(lead, B, D, width):
    """stale data to overwrite"""
    return dict(states=torch.full(lead + (B, D), 3.0, device=DEV), actions=torch.full(lead + (B, 3), 3.0, device=DEV),
                next_states=torch.full(lead + (B, D), 3.0, device=DEV), rewards=torch.full(lead + (B,), 3.0, device=DEV),
                dones=torch.full(lead + (B,), 3, dtype=torch.uint8, device=DEV),
                picks=torch.full(lead + (B, width), 3, dtype=torch.int32, device=DEV))


def _pop_args(st, B, out, draw, use_her=True, picks=None):
    """an ArmEnvHerPopArgs over the store's ring, filled here by hand"""
    from armenv import _lib as L
    r = st._ring
    pa = L.ArmEnvHerPopArgs()
    pa.members, pa.episodes_stride = st.members, r["episodes"].shape[1]
    a = pa.one
    a.T, a.N, a.ring_base, a.ring_cap, a.obs_dim, a.use_her = r["T"], r["N"], r["base"], r["cap"], r["D"], int(use_her)
    a.obs0_dev, a.obs_after_dev, a.next_obs_dev = r["obs0"].data_ptr(), r["obs_after"].data_ptr(), r["next_obs"].data_ptr()
    a.action_dev, a.reward_dev, a.done_dev = r["action"].data_ptr(), r["reward"].data_ptr(), r["done"].data_ptr()
    a.episodes_dev, a.num_episodes_dev = r["episodes"].data_ptr(), r["num_episodes"].data_ptr()
    a.batch, a.seed, a.draw, a.her_ratio, a.dis_threshold = B, st.seed, draw, S.HER_RATIO, 0.1
    a.picks_dev = None if picks is None else picks.data_ptr()
    a.states_dev, a.actions_dev, a.next_states_dev = out["states"].data_ptr(), out["actions"].data_ptr(), out["next_states"].data_ptr()
    a.rewards_dev, a.dones_dev, a.picks_out_dev = out["rewards"].data_ptr(), out["dones"].data_ptr(), out["picks"].data_ptr()
    return pa


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def shared_call(st, B, ratio, draw, use_her=True, picks=None, out=None):
    """armenv_her_pop_sample_shared through ctypes; the batch and its picks [P][B][5]"""
    from armenv import _lib as L
    out = _new_out((st.members,), B, st._ring["D"], 5) if out is None else out
    if picks is not None:
        picks = torch.as_tensor(picks).to(device=DEV, dtype=torch.int32).contiguous()
        assert tuple(picks.shape) == (st.members, B, 5)
    sa = L.ArmEnvHerPopSharedArgs(_pop_args(st, B, out, draw, use_her, picks), ratio)
    L.check(L.load().armenv_her_pop_sample_shared(0, C.byref(sa), _stream()))
    torch.cuda.synchronize(DEV)
    return out


def own_call(st, B, draw, use_her=True, picks=None):
    """armenv_her_pop_sample through ctypes; its picks [P][B][4] widened to the shared form (the member in front, INERT where inert)"""
    from armenv import _lib as L
    out = _new_out((st.members,), B, st._ring["D"], 4)
    if picks is not None:
        picks = torch.as_tensor(picks).to(device=DEV, dtype=torch.int32).contiguous()
    pa = _pop_args(st, B, out, draw, use_her, picks)
    L.check(L.load().armenv_her_pop_sample(0, C.byref(pa), _stream()))
    torch.cuda.synchronize(DEV)
    p4 = out["picks"]
    member = torch.arange(st.members, dtype=torch.int32, device=DEV)[:, None, None].expand(-1, B, 1)
    wide = torch.cat([member, p4], -1)
    wide[p4[..., 0] < 0] = INERT.to(DEV)
    return dict(out, picks=wide)


def merged_call(st, B, draw, use_her=True):
    """The single sampler on the merged ring for every member's seed: the batch [P][B][...], its picks told apart by member again.
    None if there is no episode at all (the single sampler's batch is then inert, with picks of its own form)."""
    from armenv.replay import TrajectoryStore
    r, P = st._ring, st.members
    merged = dict(cap=r["cap"], base=r["base"], T=r["T"], N=P * r["N"], D=r["D"], at_reset=r["at_reset"],
                  obs0=r["obs0"].reshape(P * r["N"], r["D"]).contiguous())
    for k in RINGS:
        t = r[k].movedim(0, 1)                                            # [cap][P][N][...]
        merged[k] = t.reshape((r["cap"], P * r["N"]) + tuple(t.shape[3:])).contiguous()
    indexer = TrajectoryStore(device=DEV, seed=st.seed)
    indexer._ring = merged
    indexer._index()                                                      # armenv_count_episodes / armenv_write_episodes
    sizes = st.sizes()
    assert indexer.size() == sum(sizes)
    if sum(sizes) == 0:
        return None
    before = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), dtype=torch.int32, device=DEV)
    ends = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=DEV)
    rows = []
    for p in range(P):
        single = TrajectoryStore(device=DEV, seed=st.seed + p)
        single.chunk = indexer.chunk
        single._draw = draw
        ref = single.sample(B, use_her=use_her, her_ratio=S.HER_RATIO, return_picks=True)
        m = torch.bucketize(ref["picks"][:, 0].contiguous(), ends, right=True).to(torch.int32)
        ref["picks"] = torch.cat([m[:, None], (ref["picks"][:, 0] - before[m.long()])[:, None], ref["picks"][:, 1:]], -1)
        rows.append(ref)
    torch.cuda.synchronize(DEV)
    return {k: torch.stack([row[k] for row in rows]) for k in KEYS}


def _cpu(batch):
    return None if batch is None else {k: batch[k].cpu() for k in KEYS}


@functools.lru_cache(maxsize=None)
def case(P, N, B, D, empty=()):
    """Everything the contracts compare, computed once per case and kept on the CPU: for both draws the population sampler (own), the
    merged single sampler (merged) and the shared sampler at 0, 0.5, 1 and the two edge ratios; the members' sizes."""
    st, _ = _store(P, N, D, S.T, S.BASE, S.AT_RESET, empty=empty, cap=S.CAP)
    assert st.seed == S.SEED and st._ring["base"] != 0
    runs = []
    for draw in S.DRAWS:
        run = dict(own=_cpu(own_call(st, B, draw)), merged=_cpu(merged_call(st, B, draw)))
        for ratio in (0.0, 0.5, 1.0) + S.EDGE_RATIOS:
            run[ratio] = _cpu(shared_call(st, B, ratio, draw))
        runs.append(run)
    return dict(sizes=st.sizes(), runs=runs)


def assert_batches_equal(got, want, what, rows=None):
    """`rows`: a bool [P][B] mask of the rows to compare; all of them by default"""
    for k in KEYS:
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        if rows is not None:
            a, b = a[rows], b[rows]
        assert torch.equal(a, b), (what, k)


CASES = [(P, N, B, D) for P in (1, 2, 5) for N in (1, 3) for B in (1, 257) for D in (6, 9)]


# ------------------------------------------------------------------------------------------------ S1: ratio 0

@pytest.mark.parametrize("P,N,B,D", CASES)
def test_ratio_0_writes_the_bytes_of_todays_population_sampler(P, N, B, D):
    c = case(P, N, B, D)
    assert min(c["sizes"]) >= 2                                           # the shared inputs' precondition
    for draw, run in zip(S.DRAWS, c["runs"]):
        assert_batches_equal(run[0.0], run["own"], draw)
        assert (run[0.0]["picks"][..., 0] == torch.arange(P, dtype=torch.int32)[:, None]).all()
    assert B == 1 or not _same(c["runs"][0][0.0]["picks"], c["runs"][1][0.0]["picks"])            # the draw counter moved


# ------------------------------------------------------------------------------------------------ S2: ratio 1

@pytest.mark.parametrize("P,N,B,D", CASES)
def test_ratio_1_is_the_single_sampler_on_the_merged_ring(P, N, B, D):
    c = case(P, N, B, D)
    for draw, run in zip(S.DRAWS, c["runs"]):
        assert_batches_equal(run[1.0], run["merged"], draw)
        pk = run[1.0]["picks"]
        assert (0 <= pk[..., 0]).all() and (pk[..., 0] < P).all() and (pk[..., 1] < torch.tensor(c["sizes"])[pk[..., 0].long()]).all()
    if P == 5 and B == 257:                                               # the condition test_pop_shared_host.py shows for this seed
        assert set(c["runs"][0][1.0]["picks"][..., 0].ravel().tolist()) == set(range(P))
        assert not _same(c["runs"][0][1.0]["states"], c["runs"][0][0.0]["states"])


# ------------------------------------------------------------------------------------------------ S3: in between

@pytest.mark.parametrize("P,N,B,D", CASES)
def test_every_row_is_the_shared_or_the_own_row_by_the_models_u4(P, N, B, D):
    c = case(P, N, B, D)
    for draw, run in zip(S.DRAWS, c["runs"]):
        for ratio in (0.5,) + S.EDGE_RATIOS:
            shared = torch.from_numpy(S.shared_mask(S.SEED, draw, P, B, ratio))
            assert_batches_equal(run[ratio], run[1.0], (draw, ratio, "shared"), rows=shared)
            assert_batches_equal(run[ratio], run[0.0], (draw, ratio, "own"), rows=~shared)
        if B == 257:
            half = S.shared_mask(S.SEED, draw, P, B, 0.5).mean()
            assert 0.2 <= half <= 0.8
            lists = S.gpu_store_lists(P, N, D)
            assert np.array_equal(run[0.5]["picks"].numpy(), S.model_picks(S.SEED, draw, B, lists, S.HER_RATIO, 1, 0.5))


# ------------------------------------------------------------------------------------------------ S4: empty members

@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("empty", [(0,), (1,), (2,)])
def test_an_empty_member_is_never_a_source_and_draws_from_the_others(empty, D):
    P, B, e = 3, 257, empty[0]
    c = case(P, 3, B, D, empty)
    assert [s == 0 for s in c["sizes"]] == [p == e for p in range(P)]
    for draw, run in zip(S.DRAWS, c["runs"]):
        one, zero = run[1.0], run[0.0]
        assert_batches_equal(one, run["merged"], draw)
        assert not (one["picks"][..., 0] == e).any() and (one["picks"][e][:, 0] >= 0).all()      # its own rows are real transitions
        assert set(one["picks"][..., 0].ravel().tolist()) == set(range(P)) - {e}
        assert_batches_equal(zero, run["own"], draw)
        assert (zero["picks"][e] == INERT).all() and (zero["dones"][e] == 1).all()
        assert all(float(zero[k][e].abs().max()) == 0.0 for k in ("states", "next_states", "actions", "rewards"))
        shared = torch.from_numpy(S.shared_mask(S.SEED, draw, P, B, 0.5))
        assert_batches_equal(run[0.5], one, (draw, "shared"), rows=shared)
        assert_batches_equal(run[0.5], zero, (draw, "own"), rows=~shared)
        assert (run[0.5]["picks"][e][~shared[e]] == INERT).all() and 0 < int(shared[e].sum()) < B


@pytest.mark.parametrize("D", [6, 9])
def test_with_all_members_empty_every_row_is_inert(D):
    P, B = 3, 257
    c = case(P, 3, B, D, (0, 1, 2))
    assert c["sizes"] == [0, 0, 0] and c["runs"][0]["merged"] is None
    for run in c["runs"]:
        for ratio in (0.0, 0.5, 1.0):
            got = run[ratio]
            assert (got["picks"] == INERT).all() and (got["dones"] == 1).all()
            assert all(float(got[k].abs().max()) == 0.0 for k in ("states", "next_states", "actions", "rewards"))


# ------------------------------------------------------------------------------------------------ S5: teacher-forced picks

@pytest.mark.parametrize("D", [6, 9])
def test_picks_fed_back_in_reproduce_the_batch_and_may_name_another_member(D):
    P, B, N = 3, 257, 3
    st, _ = _store(P, N, D, S.T, S.BASE, S.AT_RESET, cap=S.CAP)
    drawn = shared_call(st, B, 0.5, 1)
    again = shared_call(st, B, 0.0, 5, picks=drawn["picks"])              # nothing is drawn: another ratio and draw, the same batch
    assert_batches_equal(again, drawn, "fed back")
    # every member reads its neighbour's ring: the rows are the population sampler's for the neighbour, given the same picks
    own = own_call(st, B, 0)
    theirs = own["picks"].roll(-1, 0).contiguous()                        # member p gets member p + 1's picks, which name p + 1
    assert (theirs[..., 0] == ((torch.arange(P, device=DEV) + 1) % P)[:, None]).all()
    got = shared_call(st, B, 1.0, 3, picks=theirs)
    for k in KEYS:
        assert _same(got[k], own[k].roll(-1, 0)), k
    assert not _same(got["states"], own["states"])
    # a pick that names no member, or none of its episodes, gives the inert row
    bad = drawn["picks"].clone()
    bad[0, 0] = INERT.to(DEV)
    bad[1, 0, 0] = P
    bad[2, 0, 1] = st.sizes()[int(bad[2, 0, 0])]
    got = shared_call(st, B, 0.5, 1, picks=bad)
    assert (got["picks"][:, 0].cpu() == INERT).all() and (got["dones"][:, 0] == 1).all() and float(got["states"][:, 0].abs().max()) == 0.0
    for k in KEYS:
        assert _same(got[k][:, 1:], drawn[k][:, 1:]), k


# ------------------------------------------------------------------------------------------------ S6: canaries

def test_nothing_is_written_outside_the_arrays():
    """canaries around the rings, obs0, the index (counts, offsets, episodes, num_episodes), every output and the picks in and out;
    the rows of `episodes` beyond a member's count keep their filling"""
    P, B, N, D = 3, 257, 3, 6
    guards = []
    st, _ = _store(P, N, D, S.T, S.BASE, S.AT_RESET, cap=S.CAP)
    plain = {k: _cpu(shared_call(st, B, k, 0)) for k in (0.5, 1.0)}
    r = st._ring
    for k, t in list(r.items()):
        if torch.is_tensor(t):
            r[k] = _guarded(t, guards)
    r["episodes"].fill_(-77)
    st._index()
    assert torch.is_tensor(r["num_episodes"]) and len(guards) == 10
    sizes = st.sizes()
    out = {k: _guarded(t, guards) for k, t in _new_out((P,), B, D, 5).items()}
    for ratio in (0.5, 1.0):
        got = shared_call(st, B, ratio, 0, out=out)
        assert_batches_equal(got, plain[ratio], ratio)
        fed = _guarded(got["picks"].clone(), guards)
        assert_batches_equal(shared_call(st, B, 0.0, 9, picks=fed, out=out), plain[ratio], (ratio, "fed back"))
    assert len(guards) == 10 + 6 + 2 and _guards_intact(guards)
    for p in range(P):
        assert bool((r["episodes"][p, sizes[p]:] == -77).all()) and bool((r["episodes"][p, : sizes[p]] != -77).all())


# ------------------------------------------------------------------------------------------------ S7: determinism

def test_the_same_call_gives_the_same_bytes_again_and_on_another_stream():
    P, B = 3, 257
    st, _ = _store(P, 3, 9, S.T, S.BASE, S.AT_RESET, cap=S.CAP)
    runs = [_cpu(shared_call(st, B, 0.5, 4)) for _ in range(2)]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        runs.append(_cpu(shared_call(st, B, 0.5, 4)))
    side.synchronize()
    for other in runs[1:]:
        assert_batches_equal(other, runs[0], "again")


# ------------------------------------------------------------------------------------------------ S8: the store

@pytest.mark.parametrize("D", [6, 9])
def test_the_store_hands_the_entry_point_its_arguments(D):
    """PopulationTrajectoryStore.sample(share_ratio=...) against the entry point called by hand, on the kept argument struct too;
    share_ratio = 0.0 against the call without the argument (picks [P][B][4])"""
    P, B = 3, 257
    st, _ = _store(P, 3, D, S.T, S.BASE, S.AT_RESET, cap=S.CAP)
    for ratio in (0.5, 1.0):
        got = None
        for draw in (0, 1):
            st._draw = draw
            got = st.sample(B, use_her=True, her_ratio=S.HER_RATIO, return_picks=True, share_ratio=ratio, out=got)
            assert st._draw == draw + 1 and tuple(got["picks"].shape) == (P, B, 5)
            assert_batches_equal(got, shared_call(st, B, ratio, draw), (ratio, draw))
        fed = st.sample(B, picks=got["picks"], return_picks=True, share_ratio=ratio)
        assert_batches_equal(fed, got, (ratio, "fed back"))
    st._draw = 0
    with_zero = st.sample(B, use_her=True, her_ratio=S.HER_RATIO, return_picks=True, share_ratio=0.0)
    st._draw = 0
    without = st.sample(B, use_her=True, her_ratio=S.HER_RATIO, return_picks=True)
    assert tuple(with_zero["picks"].shape) == (P, B, 4)
    assert_batches_equal(with_zero, without, "0.0")
    assert _same(torch.cat([torch.arange(P, dtype=torch.int32, device=DEV)[:, None, None].expand(-1, B, 1), without["picks"]], -1),
                 shared_call(st, B, 0.0, 0)["picks"])


# ------------------------------------------------------------------------------------------------ S9: the loop

def _pop_run(recorder, **kw):  # noqa: F811
    from armenv.train_pop import train_reach_population
    from test_gpu_checkpoint import SHAPES
    return recorder.run(train_reach_population, **dict(SHAPES, members=3, seed=1, **kw))


def _same_run(x, y):
    return _tensors_equal(x["tensors"], y["tensors"]) and x["counters"] == y["counters"] and x["history"] == y["history"]


@pytest.mark.parametrize("algo", ["td3", "datd3"])
def test_the_loop_with_ratio_0_is_the_loop_without_the_argument(recorder, algo):  # noqa: F811
    a, b = _pop_run(recorder, algo=algo), _pop_run(recorder, algo=algo, share_ratio=0.0)
    assert a["counters"]["total_it"] > 0 and _same_run(a, b)
    assert a["stores"][0]["draw"] == b["stores"][0]["draw"] > 0


@pytest.mark.parametrize("algo", ["td3", "datd3"])
def test_the_loop_with_shared_replay_repeats_resumes_and_differs(recorder, tmp_path, algo):  # noqa: F811
    """share_ratio = 0.5: the uninterrupted run, the run that writes checkpoints and the run resumed from iteration 3 agree in every
    tensor and record (test_gpu_checkpoint's comparison); the run ends elsewhere than with 0.0; a resume with 0.25 is refused"""
    from armenv.checkpoint import load_run
    from armenv.train_pop import train_reach_population
    a, b, _, path = _abc(recorder, tmp_path, train_reach_population, members=3, algo=algo, seed=1, share_ratio=0.5)
    assert _same_run(a, b) and load_run(path)["config"]["share_ratio"] == 0.5
    zero = _pop_run(recorder, algo=algo)
    assert zero["counters"] == a["counters"] and zero["stores"][0]["draw"] == a["stores"][0]["draw"]
    assert not _tensors_equal(zero["tensors"], a["tensors"])
    from test_gpu_checkpoint import SHAPES
    for other in (0.25, 0.0):
        with pytest.raises(ValueError, match="share_ratio"):
            train_reach_population(resume=path, log=lambda line: None, **dict(SHAPES, members=3, algo=algo, seed=1, share_ratio=other))
