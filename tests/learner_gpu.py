"""What the GPU tests of the single fused learners share (test infrastructure): random batches on cuda:0, a learner's tensors by name
and the gradient rule of tests/test_gpu_*_fused.py; and the bookkeeping of the float64 comparisons of tests/learner_ref64_gpu.py:
|got - ref| <= C[kind] 2^-24 M_ref + allowance_ref per element, the largest measured ratios on the side."""
import copy
import json
import os

import torch

import learner_ref64 as R

DEV = "cuda:0"


def to_numpy(t):
    return t.detach().cpu().numpy()


def batch(gen, B, D=6):
    return dict(states=torch.rand(B, D, device=DEV, generator=gen), actions=torch.rand(B, 3, device=DEV, generator=gen) * 1.4 - 0.7,
                next_states=torch.rand(B, D, device=DEV, generator=gen), rewards=torch.rand(B, device=DEV, generator=gen) - 0.5,
                dones=(torch.rand(B, device=DEV, generator=gen) < 0.1).to(torch.uint8))


def state(f, nets, learning):
    """every tensor a fused update may write, by name: the `nets` of learner f and both moments of those that learn"""
    out = {}
    for name in nets:
        for k, v in getattr(f, name).state_dict().items():
            out[f"{name}.{k}"] = v.clone()
    for name in learning:
        for mv in ("_m", "_v"):
            for i, t in enumerate(getattr(f, name + mv)):
                out[f"{name}{mv}.{i}"] = t.clone()
    return out


def f64_net(net):
    return copy.deepcopy(net).double().requires_grad_(True)


def assert_grads(pairs, where):
    """Every tensor within 5e-2 of its own norm (Frobenius) and of its largest |g|; returns whether every tensor is also within 1e-4
    of its largest |g| (+ 1e-7) element by element -- the rule.  The exceptions are relu boundaries: a pre-activation within rounding
    of zero is active in one learner and not in the other.  In the critic's second layer that moves one row's delta: one row of the
    fc2 weight gradient and, through W2, a rank-one difference over the whole fc1 weight gradient (measured on update 20 of the 40
    of TD3's test_fused_gradients_equal_torch_from_identical_state: fc2 weight 1.1e-5 against a largest |g| of 4.3e-4, fc1 weight
    8.2e-7 against 2.8e-4; every tensor of the 20 updates before it within 1e-4)."""
    tight = True
    for k, (gt, gf) in enumerate(pairs):
        gmax, d = float(gt.abs().max()), gt - gf
        err, rel = float(d.abs().max()), float(d.norm() / max(float(gt.norm()), 1e-30))
        assert err <= 5e-2 * gmax + 1e-7 and rel <= 5e-2, (where, k, tuple(gt.shape), err, gmax, rel)
        tight = tight and err <= 1e-4 * gmax + 1e-7
    return tight


def f64(xs):
    return [t.detach().to(torch.float64) for t in (xs.parameters() if hasattr(xs, "parameters") else xs)]


class Bounds:
    """the constants C per kind of quantity, the cap on the share of ambiguous relu units, and `ratios`: (kind, case) -> largest
    |got - ref| - allowance, in units of 2^-24 M"""

    def __init__(self, C, amb_max):
        self.C, self.amb_max, self.ratios = C, amb_max, {}

    def check(self, kind, case, got, ref, mag, allow=None, record=True):
        """number of elements beyond C[kind] 2^-24 mag + allow; `record`: keep the largest ratio for the calibration log"""
        n, ratio = R.bad_elements(got, ref, mag, torch.zeros_like(mag) if allow is None else allow, self.C[kind])
        if record:
            self.ratios[(kind, case)] = max(self.ratios.get((kind, case), 0.0), ratio)
        return n

    def grad_failures(self, case, got, out, with_actor=True, record=True):
        """quantities whose kernel gradient / loss lies beyond the bound around the reference `out` (beta1 = 0: m is the gradient)"""
        bad = []
        lt = lambda x: torch.tensor([x], dtype=torch.float64)
        if self.check("loss", case, lt(got["loss"]), lt(out["loss"]), lt(out["loss_mag"]), record=record):
            bad.append("loss")
        for side in ("critic",) + (("actor",) if with_actor else ()):
            for k, g in enumerate(got[side + "_m"]):
                name = side + "_grad"
                if self.check(name, case, g, out[name][k], out[name + "_mag"][k], out[name + "_allow"][k], record):
                    bad.append("%s_grad%d" % (side, k))
        return bad

    def adam_failures(self, case, got, out, with_actor=True, sides=("critic", "actor"), record=True):
        """Adam-stepped parameters, moments and (with the actor step) soft-updated targets beyond C_adam 2^-24 of their magnitudes"""
        bad = []
        for side in sides:
            if side == "actor" and not with_actor:
                continue
            for name in [side, side + "_m", side + "_v"] + (["target_" + side] if with_actor else []):
                for k, t in enumerate(got[name]):
                    if self.check("adam", case, t, out[name][k], out[name + "_mag"][k], record=record):
                        bad.append("%s%d" % (name, k))
        return bad

    def ambiguity_is_rare(self, out):
        assert out["ambiguous"] <= self.amb_max * out["units"], (out["ambiguous"], out["units"])
        key = ("ambiguous_fraction", "max")
        self.ratios[key] = max(self.ratios.get(key, 0.0), out["ambiguous"] / out["units"])

    def write(self, path):
        """the largest measured ratio per kind and case as JSON (calibration of C); nothing when `path` is empty"""
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump({"%s|%s" % k: v for k, v in sorted(self.ratios.items())}, fh, indent=1)
