"""CPU tests of population-based training's host side: armenv_pop_exploit and ArmEnvPopExploitArgs (include/armenv.h) -- the ctypes
struct agrees with the header, every bad plan is refused before any HIP call, pop_exploit_kernel is in the built code object without
scratch or LDS -- and armenv.pbt.PBTSchedule: truncation selection, the perturbation, the draw order, and the refusals of the schedule
and of train_reach_population(pbt=...).  No test here passes a plan that would launch: that would copy between made-up pointers."""
import ctypes as C
import math
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT
from learner_host import ctypes_layout, header_layout, learner_kernels, refused  # noqa: F401

FIELDS = ("device", "members", "tensors", "reserved", "src", "base", "elems")
TD3_ROW = dict(actor_lr=1e-3, critic_lr=1e-3, tau=0.005, gamma=0.98, policy_noise=0.2, noise_clip=0.5, expl_sigma=0.686)
TD3_NAMES = ("actor_lr", "critic_lr", "tau", "policy_noise", "noise_clip", "expl_sigma")      # sweepable minus gamma, plus expl_sigma


def test_struct_layout_matches_the_header_the_symbol_resolves_and_the_abi_version_did_not_move():
    from armenv import _lib as L
    A = L.ArmEnvPopExploitArgs
    assert tuple(n for n, _ in A._fields_) == FIELDS
    checks = ["_Static_assert(__builtin_types_compatible_p(__typeof__(&armenv_pop_exploit), "
              "int (*)(const ArmEnvPopExploitArgs *, void *)), \"armenv_pop_exploit\");"]
    sizes, offsets = header_layout(A, extra=("ARMENV_EXPLOIT_MAX_TENSORS",), checks=checks, std="gnu11", werror=True)
    assert sizes[0] == C.sizeof(A) == 40 and sizes[1] == L.EXPLOIT_MAX_TENSORS == 128
    assert [n for n, _ in ctypes_layout(A)] == list(FIELDS) and offsets == [getattr(A, n).offset for n in FIELDS]
    lib = L.load()
    assert lib.armenv_pop_exploit is not None
    assert L.SYMBOLS["armenv_pop_exploit"] == (C.c_int, [C.POINTER(A), C.c_void_p])
    assert lib.armenv_abi_version() == 9 and L.ABI_VERSION == 9


def _args(src=(0, 0, 2), elems=(768, 3, 1), device=0):
    """(args, keep-alive): made-up (never dereferenced) device pointers; the default plan WOULD launch -- break it first"""
    from armenv import _lib as L
    a = L.ArmEnvPopExploitArgs()
    a.device, a.members, a.tensors = device, len(src), len(elems)
    s = (C.c_int32 * max(1, len(src)))(*src)
    b = (C.c_void_p * max(1, len(elems)))(*[0x10000000 + 0x1000000 * t for t in range(len(elems))])
    e = (C.c_int64 * max(1, len(elems)))(*elems)
    a.src, a.base, a.elems = s, b, e
    return a, (s, b, e)


def _call(a):
    from armenv import _lib as L
    lib = L.load()
    rc = lib.armenv_pop_exploit(C.byref(a) if a is not None else None, None)
    return rc, lib.armenv_last_error().decode()


def _refused(a):
    return refused("armenv_pop_exploit", C.byref(a) if a is not None else None, None)


def test_null_arguments_are_refused():
    from armenv import _lib as L
    assert "args" in _refused(None)
    for field in ("src", "base", "elems"):
        a, keep = _args()
        setattr(a, field, C.cast(None, dict(L.ArmEnvPopExploitArgs._fields_)[field]))
        assert field + " is NULL" in _refused(a), field


def test_device_member_and_tensor_counts_are_refused():
    a, keep = _args(device=-1)
    assert "device" in _refused(a)
    for members in (0, 65, -1):
        a, keep = _args()
        a.members = members
        assert "members" in _refused(a)
    for tensors in (0, 129, -1):
        a, keep = _args()
        a.tensors = tensors
        assert "tensors" in _refused(a)


def test_a_null_base_and_an_empty_tensor_are_refused_and_named():
    for t in (0, 2):
        a, keep = _args()
        keep[1][t] = None
        assert "base[%d]" % t in _refused(a)
        for bad in (0, -5):
            a, keep = _args()
            keep[2][t] = bad
            assert "elems[%d]" % t in _refused(a)


def test_a_source_outside_the_population_is_refused_and_named():
    for p, bad in ((0, -1), (2, 3), (1, 64), (2, -2 ** 31)):
        a, keep = _args(src=[0, 1, 2])
        keep[0][p] = bad
        assert "src[%d]" % p in _refused(a)


@pytest.mark.parametrize("src,where", [([1, 2, 2], 0), ([1, 0], 0), ([0, 2, 3, 3], 1), ([0, 1, 2, 4, 3], 3)])
def test_a_source_that_is_itself_replaced_is_refused(src, where):
    a, keep = _args(src=src)
    msg = _refused(a)
    assert "src[%d]" % where in msg and "itself replaced" in msg, msg


def test_a_bad_plan_is_refused_whole_even_when_its_first_members_are_fine():
    a, keep = _args(src=[0, 0, 2, 2, 4, 4, 6, 5])           # member 7 copies member 5, which copies member 4
    assert "src[7]" in _refused(a)


def test_an_identity_plan_returns_ok_without_a_device():
    for P in (1, 3, 64):
        a, keep = _args(src=list(range(P)), device=1000)     # no such device: it is never asked for
        rc, msg = _call(a)
        assert rc == 0, (rc, msg)


def test_the_exploit_kernel_is_in_the_code_object_without_scratch_lds_or_spills(learner_kernels):
    """test_td3_fused_host.py holds all of learner_host.learner_kernels, this one included, to no scratch, no spills and no atomics; here:
    it is there, uses no LDS, and copies 16 bytes wide."""
    assert "pop_exploit_kernel" in learner_kernels, sorted(learner_kernels)
    md, ins = learner_kernels["pop_exploit_kernel"]
    assert md["scratch"] == 0 and md["lds"] == 0 and md["spill_vgpr"] == 0, md
    mnems = [i.mnem for i in ins]
    assert "global_load_dwordx4" in mnems and "global_store_dwordx4" in mnems, sorted(set(mnems))
    assert "global_load_dword" in mnems and "global_store_dword" in mnems            # the tails and the unaligned tensors


def _schedule(seed=0, allowed=TD3_NAMES + ("gamma",), **kw):
    from armenv.pbt import PBTSchedule
    return PBTSchedule(**dict(dict(every=1, seed=seed), **kw)).bind(allowed)


def test_plan_a_hand_checked_population_of_eight():
    """Ranks: 1 (0.9), 5 (0.7), 7 (0.6), 2, 3, 6, 0 (0.1), 4 (0.0); n = int(8 * 0.25) = 2: the top is [1, 5], the bottom {0, 4}.
    Member 0 draws first, then member 4, each one randrange(2)."""
    fitness = [0.1, 0.9, 0.5, 0.3, 0.0, 0.7, 0.2, 0.6]
    for seed in range(6):
        rng = random.Random(seed)
        k0, k4 = rng.randrange(2), rng.randrange(2)
        want = list(range(8))
        want[0], want[4] = [1, 5][k0], [1, 5][k4]
        assert _schedule(seed).plan(fitness) == want, seed
    seen = {tuple(_schedule(seed).plan(fitness)) for seed in range(40)}
    assert len(seen) == 4                                   # both sources are taken by both members


def test_plan_breaks_ties_by_the_lower_index():
    # ranks 2, 3 (0.9), then the four 0.5s by index, then 6, 7: the top is [2, 3] and the bottom {6, 7}
    fitness = [0.5, 0.5, 0.9, 0.9, 0.5, 0.5, 0.1, 0.1]
    for seed in range(8):
        src = _schedule(seed).plan(fitness)
        assert src[:6] == [0, 1, 2, 3, 4, 5] and set(src[6:]) <= {2, 3}, src
    # all tied: the rank is the index, n = 1, the top is [0] and the bottom [3] -- whose source is not strictly better
    assert _schedule().plan([0.5, 0.5, 0.5, 0.5]) == [0, 1, 2, 3]
    # the bottom is the tied members with the HIGHER indices: 3 of (1, 2, 3) at 0.2; the top the lower index of the tied best
    for seed in range(8):
        assert _schedule(seed).plan([0.8, 0.2, 0.2, 0.2, 0.8]) == [0, 1, 2, 0, 4], seed


def test_plan_leaves_a_level_population_alone():
    for P in (2, 5, 16, 64):
        for level in (0.0, 0.37, 1.0):
            assert _schedule().plan([level] * P) == list(range(P))


def test_plan_ranks_nan_last():
    nan = float("nan")
    for seed in range(8):
        assert _schedule(seed).plan([0.0, nan, 0.5, 0.0]) == [0, 2, 2, 3], seed      # NaN is below the zeros
        assert _schedule(seed).plan([nan, 0.25, nan, nan]) == [0, 1, 2, 1], seed     # ... and among NaNs the higher index is lower
    assert _schedule().plan([nan, nan, nan]) == [0, 1, 2]
    assert _schedule().plan([0.3, -math.inf]) == [0, 0]


def test_plan_small_populations():
    assert _schedule().plan([0.4]) == [0] and _schedule().plan([]) == []
    assert _schedule().plan([0.1, 0.2]) == [1, 1] and _schedule().plan([0.2, 0.1]) == [0, 0]
    assert _schedule(fraction=0.5).plan([0.1, 0.2]) == [1, 1]
    assert _schedule().plan([0.3, 0.1, 0.2]) == [0, 0, 2]                           # n = max(1, int(0.75)) = 1
    assert _schedule(fraction=0.5).plan([0.1, 0.3, 0.2]) == [1, 1, 2]               # n = int(1.5) = 1


def test_no_plan_has_a_source_that_is_itself_replaced():
    from armenv.fused_pop_base import check_plan
    rng = random.Random(7)
    sched = _schedule(3)
    replaced = 0
    for _ in range(1000):
        P = rng.randrange(1, 65)
        sched.fraction = rng.choice([0.1, 0.25, 1 / 3, 0.5])
        fitness = [rng.choice([0.0, 0.25, 0.5, 1.0, float("nan")]) if rng.random() < 0.5 else rng.random() for _ in range(P)]
        src = sched.plan(fitness)
        assert len(src) == P and all(src[src[p]] == src[p] for p in range(P)), (fitness, src)
        assert check_plan("test", src, P) == src
        n = max(1, int(P * sched.fraction)) if P >= 2 else 0
        assert sum(s != p for p, s in enumerate(src)) <= n
        replaced += sum(s != p for p, s in enumerate(src))
    assert replaced > 1000


def test_explore_multiplies_by_the_documented_draws_and_clips_the_unit_range():
    for seed in range(5):
        sched = _schedule(seed, names=TD3_NAMES, perturb=(0.5, 3.0))
        rng = random.Random(seed)
        row = dict(TD3_ROW, tau=0.4)
        for _ in range(3):
            want = dict(row)
            for name in TD3_NAMES:
                want[name] = row[name] * (0.5 if rng.random() < 0.5 else 3.0)
            want["tau"] = min(want["tau"], 1.0)
            got = sched.explore(row)
            assert got == want and got["gamma"] == row["gamma"] and got is not row
            row = got
    names = ("tau", "gamma", "q_weight", "actor_lr")
    ones = _schedule(allowed=names, names=names, perturb=(2.0, 4.0)).explore(
        dict(tau=0.9, gamma=0.98, q_weight=0.3, actor_lr=0.9))
    assert ones["tau"] == 1.0 and ones["gamma"] == 1.0 and ones["q_weight"] in (0.6, 1.0) and ones["actor_lr"] in (1.8, 3.6)


def test_a_step_draws_the_plan_first_then_the_replaced_members_ascending_then_the_names_in_order():
    fitness = [0.1, 0.9, 0.5, 0.3, 0.0, 0.7, 0.2, 0.6]
    rows = [dict(TD3_ROW, actor_lr=1e-3 * (p + 1)) for p in range(8)]
    for seed in range(4):
        rng = random.Random(seed)
        src = list(range(8))
        src[0] = [1, 5][rng.randrange(2)]
        src[4] = [1, 5][rng.randrange(2)]
        want = {}
        for p in (0, 4):
            want[p] = dict(rows[src[p]])
            for name in TD3_NAMES:
                want[p][name] = rows[src[p]][name] * (0.8 if rng.random() < 0.5 else 1.2)
        kept = [dict(r) for r in rows]
        assert _schedule(seed, names=TD3_NAMES).step(fitness, rows) == (src, want)
        assert rows == kept


def test_two_schedules_with_one_seed_give_identical_sequences():
    a, b, c = _schedule(5), _schedule(5), _schedule(6)
    rng = random.Random(1)
    rows = [dict(TD3_ROW) for _ in range(16)]
    out = {0: [], 1: [], 2: []}
    for _ in range(50):
        fitness = [rng.random() for _ in range(16)]
        for k, s in enumerate((a, b, c)):
            out[k].append(s.step(fitness, rows))
    assert out[0] == out[1] and out[0] != out[2]


def test_names_default_to_what_a_member_may_own_without_gamma():
    from armenv.pbt import PBTSchedule
    from armenv.train_pop import sweepable_names
    assert PBTSchedule(3).bind(sweepable_names("td3")).names == TD3_NAMES
    assert PBTSchedule(3).bind(sweepable_names("daddpg")).names == ("actor_lr", "critic_lr", "tau", "expl_sigma")
    assert PBTSchedule(3).bind(sweepable_names("darc")).names == TD3_NAMES[:-1] + ("q_weight", "regularization_weight", "expl_sigma")
    assert PBTSchedule(3, names=("gamma", "tau")).bind(sweepable_names("datd3")).names == ("gamma", "tau")
    s = PBTSchedule(4)
    assert [s.due(i) for i in range(1, 9)] == [False, False, False, True] * 2
    with pytest.raises(ValueError):
        PBTSchedule(3).explore(dict(TD3_ROW))               # not bound: no names yet


@pytest.mark.parametrize("kw", [dict(every=0), dict(every=-2), dict(every=1.5), dict(every=2, fraction=0.6), dict(every=2, fraction=0.0),
                                dict(every=2, fraction=float("nan")), dict(every=2, perturb=(0.0, 1.2)), dict(every=2, perturb=(0.8, -1.2)),
                                dict(every=2, perturb=(0.8, float("inf"))), dict(every=2, perturb=(float("nan"), 1.2)),
                                dict(every=2, perturb=(0.8,)), dict(every=2, names=("learning_rate",)), dict(every=2, names=("policy_freq",))])
def test_the_schedule_refuses_bad_arguments(kw):
    from armenv.pbt import PBTSchedule
    with pytest.raises(ValueError):
        PBTSchedule(**kw)


def test_train_pop_refuses_a_bad_schedule_before_any_device_is_touched():
    """iterations=0 on a machine without a device: what is refused here was refused before the population, an environment or a store
    was created (the rule of the existing algo="ddpg" refusal)."""
    from armenv.pbt import PBTSchedule
    from armenv.train_pop import train_reach_population
    for kw in (dict(members=1, pbt=dict(every=2)), dict(members=1, pbt=PBTSchedule(2)), dict(members=2, pbt=dict(every=0)),
               dict(members=2, pbt=dict(every=2, fraction=0.6)), dict(members=2, pbt=dict(every=2, names=("learning_rate",))),
               dict(members=2, algo="daddpg", pbt=dict(every=2, names=("policy_noise",))),
               dict(members=2, algo="datd3", pbt=PBTSchedule(2, names=("q_weight",)))):
        with pytest.raises(ValueError):
            train_reach_population(iterations=0, **kw)


def test_the_command_line_refuses_a_bad_schedule():
    cmd = [sys.executable, "-m", "armenv.train_pop", "--iterations", "0"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "drl-on-robot-arm_amd")] + sys.path))
    for extra in (["--members", "1", "--pbt-every", "2"], ["--members", "2", "--pbt-every", "0"],
                  ["--members", "2", "--pbt-every", "2", "--pbt-fraction", "0.6"],
                  ["--members", "2", "--pbt-every", "2", "--pbt-perturb", "0,1.2"]):
        r = subprocess.run(cmd + extra, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "pbt" in r.stderr, (extra, r.returncode, r.stderr[-300:])


def test_exploit_checks_the_plan_on_the_host_and_an_identity_plan_moves_nothing():
    import torch
    from armenv.fused_td3_pop import FusedTD3Population
    pop = FusedTD3Population(3, 6, 3, 0.7, device="cpu", critic_lr=[1e-3, 2e-3, 3e-3])
    before = [t.clone() for p in range(3) for t in pop._member_state(p)]
    for bad in ([1, 2, 2], [0, 1], [0, 1, 2, 2], [0, 1, 3], [0, -1, 2], [0, 1.5, 2], 2, ["a", 1, 2]):
        with pytest.raises(ValueError):
            pop.exploit(bad)
    assert pop.exploit([0, 1, 2]) == [] and pop.exploit((0, 1, 2), hyper=False) == []
    assert all(torch.equal(x, y) for x, y in zip(before, [t for p in range(3) for t in pop._member_state(p)]))
    assert [pop.hyper(p)["critic_lr"] for p in range(3)] == [1e-3, 2e-3, 3e-3]
    with pytest.raises(RuntimeError):                       # the copy is a HIP kernel: there is no host fallback
        pop.exploit([0, 0, 2])
    assert [pop.hyper(p)["critic_lr"] for p in range(3)] == [1e-3, 2e-3, 3e-3]
