"""What the CPU and the GPU tests of the kinematics reference share: loading tests/golden/kin_ref_cases.npz, building the engine handle of
a chain path / an IK group, and err / bound of an engine's outputs against the fixture's float64 hi + lo pairs.  No mpmath, no oracle:
the GPU tests need this module and the fixture only (the reference itself is tests/kin_ref.py, the cases tests/kin_cases.py)."""
import math

import numpy as np

from conftest import golden_npz

CHAIN_PATHS = ("kuka_builtin", "kuka_generic", "diana_builtin", "diana_generic_base")
DIANA_BASE = ((0.1, -0.2, 0.3), (0.0, 0.0, math.pi))       # test_fk_generic_chain_with_base_transform
STEP_DV = 0.02
STEP_BOX = ([-4.0, -4.0, -4.0], [4.0, 4.0, 4.0])            # holds every target of the step group (the arm reaches 1.3 m)
U = {64: 2.0 ** -53, 32: 2.0 ** -24}
E_SC = 4.0                                                  # sincos / fdlibm kernel error in units of u (kin_ref docstring)


def load():
    return dict(golden_npz("kin_ref_cases.npz"))


def chain_kwargs(path):
    """Constructor arguments of the engine handle for a chain path."""
    from armenv.urdf import builtin_chain
    robot = path.split("_")[0]
    if path.endswith("base"):
        return dict(chain=builtin_chain(robot).with_base(xyz=DIANA_BASE[0], rpy=DIANA_BASE[1]))
    return dict(robot=robot, fk_path=1 if "generic" in path else 0)


def group_cfg(T, name):
    c = T[f"ik.{name}.cfg"]
    return dict(lam=float(c[0]), max_dtheta=float(c[1]), residual=float(c[2]), exit_mode=int(c[3]), angle_f32=int(c[4]),
                tip=[float(v) for v in c[5:8]], tq=[float(v) for v in c[8:12]], dv=float(c[12]))


def group_kwargs(T, name, prec):
    """Constructor arguments of the handle that runs an IK group: one update per call."""
    c = group_cfg(T, name)
    kw = dict(chain_kwargs(str(T[f"ik.{name}.path"])), precision=prec, ik_max_iters=1, ik_exit_mode=c["exit_mode"],
              ik_angle_f32=c["angle_f32"], ik_max_dtheta=c["max_dtheta"], ik_lambda=c["lam"], ik_residual=c["residual"],
              target_quat=c["tq"])
    if any(c["tip"]):
        kw["ik_tip_offset"] = c["tip"]
    return kw


def err_against(x, hi, lo):
    """|x - (hi + lo)| in float64: x - hi is exact for values this close."""
    return np.abs((np.asarray(x, dtype=np.float64) - hi) - lo)


def _ratio(err, E):
    """err / E, with 0 / 0 = 0 (a case whose reference is the input itself: exact or wrong)."""
    return np.where(E > 0, err / np.where(E > 0, E, 1.0), np.where(err == 0, 0.0, np.inf))


def fk_ratios(T, path, prec, pos, quat, idx=None):
    """(err / bound of positions [n], of quaternions [n] up to sign, use [n]) of the cases idx (default: all, in order).  use is False
    on the cases the engine is not specified for (kin_cases.F32_UNSPECIFIED): their ratios mean nothing and callers leave them out."""
    pre = f"fk.{path}.{prec}."
    g = (lambda k: T[pre + k]) if idx is None else (lambda k: T[pre + k][idx])
    ep = err_against(pos, g("pos_hi"), g("pos_lo")).max(1) / g("E_p")
    eq = np.minimum(err_against(quat, g("quat_hi"), g("quat_lo")).max(1),
                    err_against(-np.asarray(quat), g("quat_hi"), g("quat_lo")).max(1)) / g("E_q")
    return ep, eq, g("use") != 0


def ik_ratios(T, name, prec, q_out, trig=None, idx=None):
    """err / bound per case: of q_out (the worst element) and, with trig [n,14], of the carried (cos, sin) pair."""
    pre = f"ik.{name}.{prec}."
    g = (lambda k: T[pre + k]) if idx is None else (lambda k: T[pre + k][idx])
    r = _ratio(err_against(q_out, g("q_out_hi"), g("q_out_lo")), g("E_q_out")).max(1)
    if trig is None:
        return r, None
    return r, _ratio(err_against(trig, g("trig_hi"), g("trig_lo")).max(1), g("E_trig"))


def worst_by_family(T, fam_idx, ratios, use=None):
    """{family: largest ratio} over the cases in use"""
    fams = [str(s) for s in T["families"]]
    out = {}
    for f, r in zip(np.asarray(fam_idx)[use] if use is not None else fam_idx, np.asarray(ratios)[use] if use is not None else ratios):
        out[fams[f]] = max(out.get(fams[f], 0.0), float(r))
    return out
