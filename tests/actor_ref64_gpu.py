"""The device side of tests/test_gpu_actor_ref64.py and tests/tools/actor_margins.py (test infrastructure): install the nets of a
case of tests/actor_cases.py on a handle, run the forward kernels, and return err / bound against tests/actor_ref64.py."""
import numpy as np
import torch

import actor_ref64 as R

DEV = "cuda:0"
KINDS = ("actor", "actor_f16x3")


def tsd(net):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in net.items()}


def handle(D, n=64, **kw):
    from armenv import envs
    return (envs.BatchedReachEnv if D == 6 else envs.BatchedPushEnv)(n, device=DEV, **kw)


def np_(t):
    return t.detach().cpu().numpy()


def install_single(e, kind, net, bound, **kw):
    e.set_policy(kind, action_bound=bound, actor_state_dict=tsd(net), **kw)


def install_four(e, agent, nets, bound, **kw):
    a1, a2, c1, c2 = (tsd(n) for n in nets)
    if agent == "daddpg":
        assert nets[3] is nets[2]
        e.set_policy_daddpg(a1, a2, c1, action_bound=bound, **kw)
    else:
        (e.set_policy_darc if agent == "darc" else e.set_policy_datd3)(a1, a2, c1, c2, action_bound=bound, **kw)


def single_forward(e, kind, net, x, bound):
    install_single(e, kind, net, bound)
    return np_(e.actor_forward(torch.from_numpy(x).to(DEV)))


def four_forward(e, agent, nets, x, bound):
    install_four(e, agent, nets, bound)
    a, q1, q2, pk = (np_(t) for t in e.datd3_forward(torch.from_numpy(x).to(DEV), want_q=True))
    return dict(action=a, q1=q1, q2=q2, picked=pk)


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite"""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float((np.abs(got - ref) / bound).max(initial=0.0))


def four_ok(got, b):
    """(ratios, passed) of a datd3_forward result against bound_take_action's b"""
    finite = all(np.all(np.isfinite(got[k])) for k in ("action", "q1", "q2"))
    r = R.take_action_ratios(got, b)
    return r, bool(finite and r["picks_agree"] and max(r["q1"], r["q2"], r["action"]) <= 1.0)
