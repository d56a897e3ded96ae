"""The kinematics kernels (csrc/armenv_kin.h: sincos_all, fk, quat_from_frame, acos_branchfree, orientation_error, dls_update,
rotate_small) against the 40-digit reference of tests/kin_ref.py, through the C ABI: armenv_fk, one update of armenv_ik, one step of the
step and rollout kernels, and 511 steps of the carried (cos q, sin q) pair.

Reference values and bounds come from tests/golden/kin_ref_cases.npz alone (tests/test_kin_ref.py regenerates it on the CPU and shows
that the bounds hold for an emulation of the kernels' arithmetic and fail for planted defects).  EVERY element of EVERY case must be
inside its derived bound: nothing is excluded, nothing is compared by median.  Batch sizes 1, 63, 64, 65 and 261.
"""
import math

import numpy as np
import pytest

import kin_fixture as KF
import kin_ref_gpu as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def envs():
    from armenv import envs
    return envs


@pytest.fixture(scope="module")
def T():
    return KF.load()


def _report(what, fam, ratios, T, use=None):
    w = KF.worst_by_family(T, fam, ratios, use)
    print(what, "largest err / bound by family:", {k: float("%.3g" % v) for k, v in w.items()})


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", KF.CHAIN_PATHS)
def test_fk_every_case_inside_its_bound(envs, T, path, prec):
    fam = T[f"fk.{path}.family"]
    seen = np.zeros(len(fam), dtype=bool)
    first = {}
    for idx, pos, quat in G.run_fk(envs, T, path, prec):
        rp, rq, use = KF.fk_ratios(T, path, prec, pos, quat, idx)
        _report(f"fk {path} f{prec} n={len(idx)} pos", fam[idx], rp, T, use)
        _report(f"fk {path} f{prec} n={len(idx)} quat", fam[idx], rq, T, use)
        assert (rp[use] <= 1.0).all(), (len(idx), idx[use][~(rp[use] <= 1.0)], rp[use].max())
        assert (rq[use] <= 1.0).all(), (len(idx), idx[use][~(rq[use] <= 1.0)], rq[use].max())
        for k, i in enumerate(idx):                     # a case's bits do not depend on the batch it is in
            ref = first.setdefault(int(i), (pos[k], quat[k]))
            assert np.array_equal(ref[0], pos[k], equal_nan=True) and np.array_equal(ref[1], quat[k], equal_nan=True), (len(idx), i)
        seen[idx] = True
    assert seen.all()


def _ik_params(T):
    return [(str(n), int(p)) for n in T["ik_groups"] if not str(n).startswith("step") for p in T[f"ik.{n}.precs"]]


@pytest.mark.parametrize("name,prec", _ik_params(KF.load()))
def test_ik_one_update_every_case_inside_its_bound(envs, T, name, prec):
    fam, want = T[f"ik.{name}.family"], T[f"ik.{name}.{prec}.count"]
    runs, (q_rep, it_rep) = G.run_ik(envs, T, name, prec)
    seen = np.zeros(len(fam), dtype=bool)
    mixed = {}
    for idx, qo, it in runs:
        r, _ = KF.ik_ratios(T, name, prec, qo, idx=idx)
        _report(f"ik {name} f{prec} n={len(idx)}", fam[idx], r, T)
        assert np.array_equal(it, want[idx]), (len(idx), idx[it != want[idx]])
        assert (r <= 1.0).all(), (len(idx), idx[r > 1.0], r.max())
        for k, i in enumerate(idx):
            mixed[int(i)] = qo[k]
        seen[idx] = True
    assert seen.all()
    # every case alone in its wave: the straight-line side of the wave-uniform dispatch where the mixed batches took the select side
    r, _ = KF.ik_ratios(T, name, prec, q_rep[:, 0])
    _report(f"ik {name} f{prec} alone in its wave", fam, r, T)
    assert (r <= 1.0).all(), (np.flatnonzero(r > 1.0), r.max())
    assert np.array_equal(it_rep, np.repeat(want[:, None], 64, 1))
    assert np.array_equal(q_rep.view(np.uint64), np.repeat(q_rep[:, :1], 64, 1).view(np.uint64))      # the 64 lanes agree
    same = np.array([np.array_equal(q_rep[i, 0].view(np.uint64), mixed[i].view(np.uint64)) for i in range(len(fam))])
    assert same.all(), np.flatnonzero(~same)                                                         # and with the mixed batches


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name", ["step", "step_big"])
def test_step_and_rollout_kernels_one_update(envs, T, name, prec):
    """The select forms without a peel (step kernel) and the peeled trip (rollout): q and the carried pair inside their bounds -- the
    pair against cos and sin of the REFERENCE's updated q -- and the two kernels equal bit for bit.  step: the default max_dtheta, the
    pair advanced by rotate_small; step_big: max_dtheta = 1 > 0.7854, the pair recomputed by sincos_all inside the trip."""
    fam = T[f"ik.{name}.family"]
    seen = np.zeros(len(fam), dtype=bool)
    for idx in G.batches(len(fam)):
        out = G.run_step(envs, T, name, prec, idx)
        for kern, (q, trig) in out.items():
            r, rt = KF.ik_ratios(T, name, prec, q, trig, idx)
            _report(f"{name}: {kern} kernel f{prec} n={len(idx)} q", fam[idx], r, T)
            _report(f"{name}: {kern} kernel f{prec} n={len(idx)} pair", fam[idx], rt, T)
            assert (r <= 1.0).all(), (kern, len(idx), idx[r > 1.0], r.max())
            assert (rt <= 1.0).all(), (kern, len(idx), idx[rt > 1.0], rt.max())
        assert np.array_equal(out["step"][0].view(np.uint64), out["rollout"][0].view(np.uint64))
        assert np.array_equal(out["step"][1].view(np.uint64), out["rollout"][1].view(np.uint64))
        seen[idx] = True
    assert seen.all()


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("task", ["reach", "push", "pick"])
def test_carried_pair_drift_over_511_steps(envs, task, prec):
    """How far the incrementally advanced (cos q, sin q) may be from cos and sin of the env's own q after 511 steps in which no env is
    reset and nothing re-derives the pair: kin_ref_gpu.drift_bound, from the number of updates actually applied and the largest |q|
    the run passed through.  c^2 + s^2 - 1 = 2 (c dc + s ds) to first order, |c| + |s| <= sqrt 2: 2 sqrt 2 times the same bound."""
    d = G.run_drift(envs, task, prec)
    print(f"drift {task} f{prec}: updates {d['updates'].min()}..{d['updates'].max()}, limit steps {d['limit_steps']}, max |q| on the way "
          f"{d['q_abs_max']:.3g}, pair err {d['pair_err'].max():.3g}, norm err {d['norm_err'].max():.3g}, "
          f"bound {d['bound'].min():.3g}..{d['bound'].max():.3g}")
    assert (d["step"] == G.DRIFT_STEPS).all() and d["dones"] == 0 and d["episodes"] == 0        # 511 steps behind every pair
    assert d["replay_equal"]
    assert d["updates"].min() >= G.DRIFT_STEPS
    assert (d["pair_err"] <= d["bound"]).all(), (d["pair_err"] / d["bound"]).max()
    assert (d["norm_err"] <= 2 * math.sqrt(2) * d["bound"] * (1 + d["bound"])).all(), (d["norm_err"] / d["bound"]).max()
