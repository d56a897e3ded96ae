"""The GPU side of the kinematics reference tests: runs the engine on the cases of tests/golden/kin_ref_cases.npz and returns err / bound
per case.  Shared by tests/test_gpu_kin_ref.py (which asserts) and tests/tools/kin_margins.py (which records the largest ratios)."""
import numpy as np
import torch

import kin_fixture as KF

DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 256 + 5)         # a lone lane, ragged waves on either side of one wave, several waves and a ragged one


def _np(t):
    return t.detach().cpu().numpy()


def batches(n_cases):
    """Index arrays into the case list, one per batch size: the first cases for the small sizes, the whole list tiled for the largest
    (every case is in it at least once)."""
    assert n_cases <= SIZES[-1]
    return [np.arange(s) % n_cases for s in SIZES]


def run_fk(envs, T, path, prec):
    """[(idx, pos, quat)] of armenv_fk over the batch sizes."""
    q = T[f"fk.{path}.q"]
    e = envs.BatchedReachEnv(8, device=DEV, precision=prec, **KF.chain_kwargs(path))
    assert ("generic" in e.kernel_name) == ("generic" in path), e.kernel_name
    out = []
    for idx in batches(len(q)):
        pos, quat = e.fk(torch.from_numpy(q[idx]))
        out.append((idx, _np(pos), _np(quat)))
    e.close()
    return out


def run_ik(envs, T, name, prec):
    """armenv_ik with one update per call.  Returns ([(idx, q_out, count)] over the batch sizes, (q_out, count) [n_cases, 64, ...] of every
    case alone in its wave: the case in all 64 lanes, one wave per case, one launch)."""
    q, tgt = T[f"ik.{name}.q"], T[f"ik.{name}.tgt"]
    e = envs.BatchedReachEnv(8, device=DEV, **KF.group_kwargs(T, name, prec))
    out = []
    for idx in batches(len(q)):
        qo, it = e.ik(torch.from_numpy(q[idx]), torch.from_numpy(tgt[idx]))
        out.append((idx, _np(qo), _np(it)))
    rep = np.repeat(np.arange(len(q)), 64)
    qo, it = e.ik(torch.from_numpy(q[rep]), torch.from_numpy(tgt[rep]))
    e.close()
    return out, (_np(qo).reshape(len(q), 64, 7), _np(it).reshape(len(q), 64))


def run_step(envs, T, name, prec, n_idx):
    """The cases idx of a step group (`step`, `step_big`) through the step kernel and through a one-step rollout: set_state(q) without trig, one step
    with the case's action, get_state.  Returns dict(step=(q, trig), rollout=(q, trig))."""
    q, act = T[f"ik.{name}.q"][n_idx], T[f"ik.{name}.tgt"][n_idx].astype(np.float32)
    n = len(n_idx)
    kw = KF.group_kwargs(T, name, prec)
    # no step ends an episode, no target is clipped
    e = envs.BatchedReachEnv(n, device=DEV, auto_reset=False, reach_dis=1e-9, max_steps=10 ** 6, dv=KF.STEP_DV,
                             box_lo=KF.STEP_BOX[0], box_hi=KF.STEP_BOX[1], **kw)
    e.reset()
    a = torch.from_numpy(act).to(DEV).contiguous()
    out = {}
    e.set_state(q=torch.from_numpy(q))
    _, _, done, _ = e.step(a)
    assert not bool(done.any())
    st = e.get_state()
    out["step"] = (_np(st["q"]), _np(st["trig"]))
    e.set_state(q=torch.from_numpy(q))
    r = e.rollout(1, a[None].contiguous())
    assert not bool(r["done"].any())
    st = e.get_state()
    out["rollout"] = (_np(st["q"]), _np(st["trig"]))
    e.close()
    return out


DRIFT_STEPS = 511        # the pair is re-derived from q when an env's step counter reaches a multiple of 512


def run_drift(envs, task, prec, n=64 + 5, seed=3):
    """511 steps of seeded actions in ONE rollout on a bookkeeping handle (fence_counters = 1: per-step update counts) built so that no
    env is ever reset -- a reset installs a freshly derived pair: max_steps 1300 and success distances of 1e-9, as
    test_trig_rederivation_at_step_512 has them.  A twin handle then replays the same steps one launch at a time and reads q after
    each, for the largest |q| the run passed through (the two runs are the same bits: checked).  Returns dict: pair_err [n] = max
    |carried - (cos q, sin q)| against float64 libm of the handle's own final q, norm_err [n] = max |c^2 + s^2 - 1|, bound [n],
    updates [n], step [n], dones, episodes (finished, from the counters), limit_steps, q_abs_max, replay_equal."""
    cls = dict(reach=envs.BatchedReachEnv, push=envs.BatchedPushEnv, pick=envs.BatchedPickEnv)[task]
    kw = dict(device=DEV, precision=prec, seed=seed, fence_counters=1, max_steps=1300)
    kw.update(dict(reach_dis=1e-9) if task == "reach" else dict(push_success_dis=1e-9))
    g = torch.Generator().manual_seed(seed)
    sig = 0.686 if task == "reach" else 0.392
    a = torch.clamp(torch.randn((DRIFT_STEPS, n, 3), generator=g) * sig, -0.7, 0.7).to(DEV).contiguous()
    e = cls(n, **kw)
    e.reset()
    r = e.rollout(DRIFT_STEPS, a, want_ik_updates=True)
    st = e.get_state()
    cnt = e.counters()
    q, trig, step = _np(st["q"]), _np(st["trig"]), _np(st["step"])
    upd = _np(r["ik_updates"]).astype(np.int64)
    dones = int(_np(r["done"]).sum())
    max_dtheta, max_iters = float(e.cfg.ik_max_dtheta), int(e.cfg.ik_max_iters)
    e.close()
    t = cls(n, **kw)
    t.reset()
    q_max = np.abs(_np(t.get_state()["q"])).max()
    for k in range(DRIFT_STEPS):
        t.step(a[k])
        q_max = max(q_max, float(t.get_state()["q"].abs().max()))
    st2 = t.get_state()
    same = bool(np.array_equal(_np(st2["q"]).view(np.uint64), q.view(np.uint64)) and
                np.array_equal(_np(st2["trig"]).view(np.uint64), trig.view(np.uint64)))
    t.close()
    return dict(pair_err=np.abs(trig - np.concatenate([np.cos(q), np.sin(q)], axis=1)).max(1),
                norm_err=np.abs(trig[:, :7] ** 2 + trig[:, 7:] ** 2 - 1.0).max(1),
                bound=drift_bound(upd.sum(0), prec, q_max + max_iters * max_dtheta),
                updates=upd.sum(0), step=step, dones=dones, episodes=int(cnt["episodes"]), limit_steps=int(cnt["limit_steps"]),
                q_abs_max=float(q_max), replay_equal=same)


def drift_bound(updates, prec, Q):
    """What N updates may put between the carried pair and (cos, sin) of the carried q.  Per update: rotate_small, (2 E_sc + 3) u (the
    fdlibm kernels of the step and one fused 2x2 rotation; rotations keep the norm of the error already there), and u Q for the
    rounding of q += dtheta, which the pair does not see.  Once: E_sc u for the pair a reset derives, and 2^-52 for the host's libm.
    Q bounds |q| at every update: the largest |q| at the end of any step of the run, plus the at most max_iters updates of at most
    max_dtheta each that a step's IK call passes through."""
    u = KF.U[prec]
    return np.asarray(updates, dtype=np.float64) * ((2 * KF.E_SC + 3) * u + u * Q) + KF.E_SC * u + 2.0 ** -52
