"""The wave-uniform orientation dispatch of the IK trip (armenv_kin.h ARMENV_UNIFORM_ORIENT) gives a lane the same bits whichever
side its wave takes.

quat_from_frame and acos_branchfree compute the common candidates straight-line (quaternion case y or x; the outer acos form) and
run their select forms only in a wave with a lane outside them.  Which side runs depends on the OTHER lanes of the wave, so the
check is one pose solved in two companies, through armenv_ik (ik_move carries the dispatch):

  batch A   64 different poses in one wave: the lanes disagree on the quaternion case and on the acos form -> the select forms run;
  batch B_j pose j in every lane: the wave agrees by construction -> the straight-line side runs wherever pose j is in the common
            candidates, the select forms (now with every lane in ONE case) wherever it is not.

q_out and the update count of lane j of A must equal lane 0 of B_j bit for bit, for every j, and all lanes of B_j must be equal.
The same again on a 96-env handle: a ragged second wave (32 live lanes) holds poses 0..31 a second time.

Draws (seed 7): 63 joint vectors uniform over the URDF limits and, as pose 0, a settled pose (the oracle's IK from the reset pose,
called eight times as the env's steps would: its orientation equals the target's to rounding, the degenerate-axis start that no
uniform draw produces); targets 1-5 cm from each pose's flange.  Coverage of the start frames, computed with the CPU oracle and
asserted below: quaternion cases w / z / y / x on 21 / 12 / 14 / 17 poses, |w| of the error quaternion below 0.5 (inner acos form) on 41
and above on 23, degenerate axis on 1.  The later trips of each call move through further cases."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 7


def _quat_case(R):
    m00, m11, m22 = R[0, 0], R[1, 1], R[2, 2]
    if m00 + m11 + m22 > 0:
        return 0
    if (m11 < m22) if m00 < m11 else (m00 < m22):
        return 1
    return 2 if m00 < m11 else 3


@pytest.fixture(scope="module")
def draws(O, kuka):
    rng = np.random.default_rng(SEED)
    cfg = O.default_config()
    lim = np.array(O.KUKA["limit"])
    q = rng.uniform(-lim, lim, (64, 7))
    q_conv = np.array(cfg.q_init[:])[None]
    for _ in range(8):                                     # repeated calls, as the env's steps make them: the orientation settles
        q_conv, _ = O.ik(kuka, cfg, q_conv, np.array([0.45, 0.1, 0.3]))
    q[0] = q_conv[0]
    p, quat = O.fk(kuka, q)
    u = rng.normal(size=(64, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tgt = p + rng.uniform(0.01, 0.05, (64, 1)) * u
    # what the start frames cover (module docstring)
    cases = np.array([_quat_case(O.fk_full(kuka, q[i])[1]) for i in range(64)])
    tq = np.array(cfg.target_quat[:])
    dw = tq[3] * quat[:, 3] + quat[:, :3] @ tq[:3]
    degenerate = (1.0 - dw * dw) < 10 * np.finfo(np.float64).eps
    cover = dict(cases=np.bincount(cases, minlength=4).tolist(), inner=int((np.abs(dw) < 0.5).sum()), degenerate=int(degenerate.sum()))
    return q, tgt, cover


def test_draws_cover_every_case(draws):
    _, _, cover = draws
    print("coverage of the start frames:", cover)
    assert min(cover["cases"]) >= 1, cover
    assert 1 <= cover["inner"] <= 63, cover
    assert cover["degenerate"] >= 1, cover


@pytest.mark.parametrize("n", [64, 96])
@pytest.mark.parametrize("precision", [64, 32])
def test_lane_bits_do_not_depend_on_the_wave(draws, precision, n):
    from armenv import envs
    q, tgt, _ = draws
    idx = np.arange(n) % 64
    e = envs.BatchedReachEnv(n, device=DEV, precision=precision)
    qa, ia = e.ik(torch.from_numpy(q[idx]), torch.from_numpy(tgt[idx]))
    qa, ia = qa.cpu().numpy(), ia.cpu().numpy()
    assert np.isfinite(qa).all()
    assert len(set(ia.tolist())) > 1                       # the lanes of A leave the loop at different trips
    qb_all, ib_all = [], []
    for j in range(64):
        qb, ib = e.ik(torch.from_numpy(np.repeat(q[j:j + 1], n, 0)), torch.from_numpy(np.repeat(tgt[j:j + 1], n, 0)))
        qb_all.append(qb); ib_all.append(ib)
    qb_all, ib_all = torch.stack(qb_all).cpu().numpy(), torch.stack(ib_all).cpu().numpy()
    e.close()
    for j in range(64):
        qb, ib = qb_all[j], ib_all[j]
        assert np.array_equal(qb.view(np.uint64), np.repeat(qb[:1], n, 0).view(np.uint64)) and (ib == ib[0]).all(), j
        for k in range(j, n, 64):
            assert np.array_equal(qa[k].view(np.uint64), qb[0].view(np.uint64)), (j, k, np.abs(qa[k] - qb[0]).max())
            assert ia[k] == ib[0], (j, k, ia[k], ib[0])
