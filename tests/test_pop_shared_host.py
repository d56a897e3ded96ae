"""CPU tests of the shared population sampler's host side (armenv_her_pop_sample_shared, ArmEnvHerPopSharedArgs, include/armenv.h;
PopulationTrajectoryStore.sample(share_ratio=...); armenv.train_pop's share_ratio): the ctypes struct agrees with the header, every
bad argument is refused before any HIP call, the two kernels are in the built code object without scratch or LDS, the Python layers
refuse what they must before any device call, and the numpy model of the draw rule (tests/pop_shared_cases.py), which the GPU tests
lean on, agrees with the concatenation model and shows that the GPU tests' seeds meet their conditions."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import pop_shared_cases as S
from learner_host import all_kernels, ctypes_layout, header_layout, refused
from test_pop_store_host import SAMPLE_REFUSALS, _args


def _shared(ratio=0.5, **kw):
    """arguments that pass every check: test_pop_store_host's made-up population arguments (never dereferenced) and a share_ratio.
    NOT to be passed unmodified -- a valid set would be enqueued."""
    from armenv import _lib as L
    return L.ArmEnvHerPopSharedArgs(_args(**kw), ratio)


# ------------------------------------------------------------------------------------------------ H1: ABI layout

def test_struct_layout_matches_the_header():
    from armenv import _lib as L
    members = ctypes_layout(L.ArmEnvHerPopSharedArgs)
    assert [m for m, _ in members][-3:] == ["pop.members", "pop.episodes_stride", "share_ratio"]
    sizes, offsets = header_layout(L.ArmEnvHerPopSharedArgs, extra=("sizeof(ArmEnvHerPopArgs)", "sizeof(double)"))
    assert sizes == [C.sizeof(L.ArmEnvHerPopSharedArgs), C.sizeof(L.ArmEnvHerPopArgs), 8]
    assert offsets == [o for _, o in members], members
    assert L.ArmEnvHerPopSharedArgs.share_ratio.offset == C.sizeof(L.ArmEnvHerPopArgs) == C.sizeof(L.ArmEnvHerPopSharedArgs) - 8


def test_the_symbol_resolves_with_its_prototype_and_the_abi_version_did_not_move():
    from armenv import _lib as L
    lib = L.load()
    assert lib.armenv_abi_version() == 9 and L.ABI_VERSION == 9
    restype, argtypes = L.SYMBOLS["armenv_her_pop_sample_shared"]
    assert restype is C.c_int and argtypes == [C.c_int32, C.POINTER(L.ArmEnvHerPopSharedArgs), C.c_void_p]
    fn = lib.armenv_her_pop_sample_shared
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes


# ------------------------------------------------------------------------------------------------ H2: refusals

def test_null_args_are_refused():
    assert "args" in refused("armenv_her_pop_sample_shared", 0, None, None)


@pytest.mark.parametrize("ratio", [-0.1, 1.1, float("nan"), float("inf"), float("-inf")])
def test_a_share_ratio_outside_the_unit_interval_is_refused_before_any_device_call(ratio):
    assert "share_ratio" in refused("armenv_her_pop_sample_shared", 0, C.byref(_shared(ratio)), None)


@pytest.mark.parametrize("field,mutate", SAMPLE_REFUSALS)
def test_everything_the_population_sampler_refuses_is_refused(field, mutate):
    sa = _shared()
    mutate(sa.pop)
    assert field in refused("armenv_her_pop_sample_shared", 0, C.byref(sa), None)


@pytest.mark.parametrize("ratio", [0.0, 0.5, 1.0])
def test_an_empty_batch_is_ok_without_a_launch(ratio):
    """batch == 0 returns ARMENV_OK on made-up pointers and an absent device; the bounds of share_ratio and of members are accepted"""
    from armenv import _lib as L
    for members in (1, 64):
        assert L.load().armenv_her_pop_sample_shared(0, C.byref(_shared(ratio, P=members, B=0)), None) == 0
    sa = _shared(ratio)
    sa.pop.one.obs_dim = 7                        # the ratio passed: the call is refused for the next broken field
    assert "obs_dim" in refused("armenv_her_pop_sample_shared", 0, C.byref(sa), None)


# ------------------------------------------------------------------------------------------------ H3: kernels present

def test_the_shared_kernels_are_in_the_code_object_without_scratch_or_lds():
    kernels = {dm.replace("void ", "").split("(")[0].replace("armenv::", ""): (md, ins) for _, dm, md, ins in all_kernels()
               if "her_sample" in dm}
    want = ("her_sample_pop_shared_kernel<6>", "her_sample_pop_shared_kernel<9>")
    assert set(want) <= set(kernels), sorted(kernels)
    for k in want:
        md, ins = kernels[k]
        assert md["scratch"] == 0 and md["lds"] == 0 and md["spill_vgpr"] == 0 and len(ins) > 0, (k, md)
        mnems = {i.mnem for i in ins}
        assert not any("atomic" in m or m.startswith(("ds_", "scratch_")) for m in mnems), (k, sorted(mnems))


# ------------------------------------------------------------------------------------------------ H4: the Python layers refuse

@pytest.fixture
def host_store(monkeypatch):
    """a PopulationTrajectoryStore on the cpu device that holds one rollout (the index launches are left out)"""
    from armenv import replay
    monkeypatch.setattr(replay.PopulationTrajectoryStore, "_index", lambda self: None)
    st = replay.PopulationTrajectoryStore(3, device="cpu", capacity_steps=8)
    st.rollout_buffers(5, 2, 6)
    st.add_rollouts(torch.zeros(3, 2, 6))
    return st


@pytest.mark.parametrize("ratio", [-0.1, 1.1, float("nan"), float("inf")])
def test_sample_refuses_a_bad_share_ratio_before_any_device_call(host_store, ratio):
    with pytest.raises(ValueError, match=re.escape("PopulationTrajectoryStore.sample: share_ratio must be in [0, 1]")):
        host_store.sample(4, share_ratio=ratio)
    assert host_store._draw == 0 and host_store._bound is None            # a refused call draws nothing and binds nothing


def test_the_single_store_did_not_gain_the_argument():
    import inspect

    from armenv.replay import PopulationTrajectoryStore, TrajectoryStore
    assert "share_ratio" not in inspect.signature(TrajectoryStore.sample).parameters
    assert inspect.signature(PopulationTrajectoryStore.sample).parameters["share_ratio"].default == 0.0


def test_share_ratio_joins_the_key_of_the_kept_struct_and_picks_the_entry_point(host_store, monkeypatch):
    """the launches replaced by recorders: 0.0 goes to armenv_her_pop_sample with the ArmEnvHerPopArgs, any other value to the shared
    entry point with the ratio in the struct; a repeated call keeps its struct, another ratio builds a new one; _draw advances"""
    from armenv import _lib as L
    calls = []
    monkeypatch.setattr(host_store, "_stream", lambda: None)
    monkeypatch.setattr(host_store, "_launch", lambda dev, args, stream: calls.append(("own", args)) or 0)
    monkeypatch.setattr(host_store, "_launch_shared", lambda dev, args, stream: calls.append(("shared", args)) or 0)
    out = host_store.sample(4, share_ratio=0.0)
    host_store.sample(4, out=out)
    host_store.sample(4, out=out, share_ratio=0.5, return_picks=True)
    host_store.sample(4, out=out, share_ratio=0.5, return_picks=True)
    host_store.sample(4, out=out, share_ratio=1.0)
    assert [c[0] for c in calls] == ["own", "own", "shared", "shared", "shared"] and host_store._draw == 5
    assert calls[0][1] is calls[1][1] and isinstance(calls[0][1], L.ArmEnvHerPopArgs)
    assert calls[2][1] is calls[3][1] and calls[3][1] is not calls[4][1] and isinstance(calls[2][1], L.ArmEnvHerPopSharedArgs)
    assert (calls[2][1].share_ratio, calls[4][1].share_ratio) == (0.5, 1.0) and calls[4][1].pop.one.draw == 4
    assert tuple(out["picks"].shape) == (3, 4, 5) and calls[3][1].pop.one.picks_out_dev == out["picks"].data_ptr()
    assert calls[4][1].pop.members == 3 and calls[4][1].pop.one.states_dev == out["states"].data_ptr()


def test_train_pop_refuses_share_ratio_before_anything_is_created():
    from armenv.train_pop import train_reach_population
    for kw in (dict(share_ratio=-0.1), dict(share_ratio=1.1), dict(share_ratio=float("nan")), dict(share_ratio=0.5, store="members")):
        with pytest.raises(ValueError, match="share_ratio"):
            train_reach_population(members=2, iterations=0, **kw)


# ------------------------------------------------------------------------------------------------ H5: the model of the draw rule

def _random_lists(rng, P, empty):
    """P episode lists (env, t_start, length) with 1..7 episodes of 1..12 steps each, those of `empty` without any"""
    return [np.zeros((0, 3), np.int32) if p in empty else
            np.stack([rng.integers(0, 3, E), rng.integers(0, 20, E), rng.integers(1, 13, E)], -1).astype(np.int32)
            for p, E in enumerate(rng.integers(1, 8, P))]


@pytest.mark.parametrize("P,empty", [(1, ()), (2, ()), (5, ()), (3, (0,)), (3, (1,)), (3, (2,)), (5, (0, 2, 4)), (4, (1, 2))])
def test_the_model_is_the_concatenation_model_at_1_and_todays_sampler_at_0(P, empty):
    rng = np.random.default_rng([20261021, P, len(empty)])
    lists = _random_lists(rng, P, empty)
    for seed, draw, B, use_her in ((7, 0, 257, 1), (2 ** 64 - 1, 2 ** 32 + 1, 64, 1), (5, 1, 64, 0)):
        one = S.model_picks(seed, draw, B, lists, 0.8, use_her, 1.0)
        assert np.array_equal(one, S.concatenation_picks(seed, draw, B, lists, 0.8, use_her))
        assert not set(one[..., 0].ravel().tolist()) & set(empty)
        zero = S.model_picks(seed, draw, B, lists, 0.8, use_her, 0.0)
        assert np.array_equal(zero, S.own_picks(seed, draw, B, lists, 0.8, use_her))
        for ratio in (0.5,) + S.EDGE_RATIOS:
            mask = S.shared_mask(seed, draw, P, B, ratio)
            assert np.array_equal(S.model_picks(seed, draw, B, lists, 0.8, use_her, ratio), np.where(mask[..., None], one, zero))


def test_the_model_gives_inert_rows_where_the_pool_is_empty():
    lists = [np.zeros((0, 3), np.int32)] * 3
    assert S.concatenation_picks(7, 0, 64, lists, 0.8, 1) is None
    for ratio in (0.0, 0.5, 1.0):
        assert (S.model_picks(7, 0, 64, lists, 0.8, 1, ratio) == np.array(S.INERT)).all()
    lists[1] = np.array([[0, 0, 4]], np.int32)
    half = S.model_picks(7, 0, 257, lists, 0.8, 1, 0.5)
    mask = S.shared_mask(7, 0, 3, 257, 0.5)
    assert (half[mask][:, :2] == (1, 0)).all() and (half[1][:, :2] == (1, 0)).all()
    assert (half[0][~mask[0]] == np.array(S.INERT)).all() and (half[2][~mask[2]] == np.array(S.INERT)).all()


def test_u4_is_a_block_of_its_own():
    """u4 differs from u0..u3 of the same row, moves with seed, draw and row, and reads the low 32 bits of the draw"""
    u, u4 = S.philox_uniforms(7, 0, 257), S.u4_uniforms(7, 0, 257)
    assert u4.shape == (257,) and (0.0 <= u4).all() and (u4 < 1.0).all() and len(np.unique(u4)) == 257
    assert all(not np.array_equal(u4, u[k]) for k in range(4))
    assert not np.array_equal(u4, S.u4_uniforms(8, 0, 257)) and not np.array_equal(u4, S.u4_uniforms(7, 1, 257))
    assert np.array_equal(S.u4_uniforms(7, 1, 257), S.u4_uniforms(7, 2 ** 32 + 1, 257))
    assert np.array_equal(S.u4_uniforms(7, 0, 64), u4[:64])


@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("N", [1, 3])
def test_the_gpu_tests_seeds_meet_their_conditions(N, D):
    """On the GPU tests' store at P = 5, B = 257 and their seed and draws: at share_ratio 1 every member that has episodes occurs as
    a source and none that has not; at 0.5 at least 20 % of every draw's rows fall on either side of u4.  (A seed that fails is
    replaced HERE.)"""
    P, B = 5, 257
    for empty in ((), (0,), (2,), (4,)):
        lists = S.gpu_store_lists(P, N, D, empty)
        assert all((len(lists[p]) == 0) == (p in empty) for p in range(P)) and min(len(e) for p, e in enumerate(lists) if p not in empty) >= 2
        for draw in S.DRAWS:
            sources = set(S.model_picks(S.SEED, draw, B, lists, S.HER_RATIO, 1, 1.0)[..., 0].ravel().tolist())
            assert sources == set(range(P)) - set(empty), (empty, draw, sources)
    for P in (1, 2, 3, 5):
        for draw in S.DRAWS:
            share = S.shared_mask(S.SEED, draw, P, B, 0.5).mean()
            assert 0.2 <= share <= 0.8, (P, draw, share)
            lo, hi = (S.shared_mask(S.SEED, draw, P, B, r) for r in S.EDGE_RATIOS)
            assert not lo.any() and hi.all()          # u4 == 0 and u4 == 1 - 2^-53 do not occur in these rows
