"""The fused policy forwards on cuda:0 -- the exact-f32 actor, the f16x3 actor and the four-net take_action pass behind
armenv_datd3_forward (DATD3, DARC, DADDPG) -- against the float64 restatement of tests/actor_ref64.py, element by element within the
error bounds DERIVED there (no tolerance in this file is a constant), over the cases of tests/actor_cases.py: every layer scale from
2^-8 to 2^4 and the compensated combinations of a trained net, observation scales 1e-3 .. 30, zero and dominated rows, magnitudes
mixed inside one MFMA tile, values planted at the edges of the f16 split, the largest activation just under 65504, and nets whose lo
parts are coherent (on which tests/test_actor_ref64.py shows that a dropped pass, a flushed subnormal lo part, an unsplit bias or a
lo table read from the wrong net leaves the bound).  Each test records max(err / bound) as a property."""
import numpy as np
import pytest
import torch

import actor_cases as K
import actor_ref64 as R
import actor_ref64_gpu as G

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 255, 256, 257, 1024 + 192)


@pytest.fixture(scope="module")
def handles():
    """one 64-env handle per observation width, shared by the forward tests (a forward reads the installed policy only)"""
    h = {D: G.handle(D) for D in (6, 9)}
    yield h
    for e in h.values():
        e.close()


@pytest.mark.parametrize("cid", [c["id"] for c in K.SINGLE])
def test_single_net_forwards_within_the_derived_bounds(handles, record_property, cid):
    """both actor kernels on every single-net case (the DDPG agent's actor is one of them): finite, |gpu - ref64| <= bound on every
    output, and the two kernels within the sum of their bounds of each other"""
    s = K.single(cid)
    e = handles[K.by_id(cid)["D"]]
    a32 = G.single_forward(e, "actor", s["net"], s["x"], s["bound"])
    a16 = G.single_forward(e, "actor_f16x3", s["net"], s["x"], s["bound"])
    r32, r16 = G.ratio(a32, s["ref"]["out"], s["b32"]["out"]), G.ratio(a16, s["ref"]["out"], s["b16"]["out"])
    rx = G.ratio(a32, a16.astype(np.float64), s["b32"]["out"] + s["b16"]["out"])
    record_property("ratio_f32", r32); record_property("ratio_f16x3", r16); record_property("ratio_f32_vs_f16x3", rx)
    print("%s: err / bound f32 %.3g, f16x3 %.3g, f32 vs f16x3 %.3g" % (cid, r32, r16, rx))
    assert a32.shape == a16.shape == (K.N, 3) and np.all(np.isfinite(a32)) and np.all(np.isfinite(a16))
    assert r32 <= 1.0 and r16 <= 1.0 and rx <= 1.0, (r32, r16, rx)


@pytest.mark.parametrize("cid", [c["id"] for c in K.FOUR])
def test_take_action_within_the_derived_bounds(handles, record_property, cid):
    """datd3_forward(want_q=True) on every four-net case: q1 and q2 raw within their bounds on every row; on clear rows the
    reference's pick and the picked actor's action within that actor's bound; identical actors: q1 == q2 bitwise, actor 1 picked"""
    f, c = K.four(cid), K.by_id(cid)
    got = G.four_forward(handles[c["D"]], c["agent"], f["nets"], f["x"], f["bound"])
    r, ok = G.four_ok(got, f["b"])
    for k in ("q1", "q2", "action"):
        record_property("ratio_" + k, r[k])
    print("%s: err / bound q1 %.3g, q2 %.3g, action %.3g" % (cid, r["q1"], r["q2"], r["action"]))
    assert ok, r
    if c["kind"] == "identical-actors":
        assert np.array_equal(got["q1"], got["q2"]) and not got["picked"].any()
        a1 = f["b"]["ref"]["a1"]
        assert G.ratio(got["action"], a1, f["b"]["a1"]) <= 1.0
    else:
        clear = R.clear_rows(f["b"])
        assert 0 < got["picked"][clear].sum() < clear.sum()                 # both picks occur


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("D", [6, 9])
def test_actor_batch_sizes_and_the_last_workgroup(handles, record_property, kind, D):
    """the mixed-scale net on the first n rows of one batch, n around the wave and workgroup sizes: the kernels clamp the row index
    in the last workgroup, and a wrong clamp shows as row n - 1's value in a live row (every row's reference differs)"""
    net, x = K.mixed_single(D, max(BATCHES))
    b = (R.bound_f16x3 if kind == "actor_f16x3" else R.bound_f32)(net, x, K.BOUND, full=True)
    e = handles[D]
    G.install_single(e, kind, net, K.BOUND)
    worst = 0.0
    for n in BATCHES:
        a = G.np_(e.actor_forward(torch.from_numpy(x[:n]).to(G.DEV)))
        assert a.shape == (n, 3)
        worst = max(worst, G.ratio(a, b["ref"]["out"][:n], b["out"][:n]))
    record_property("ratio", worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("D", [6, 9])
def test_take_action_batch_sizes_and_the_last_workgroup(handles, record_property, D, shared):
    f = K.mixed_four(D, max(BATCHES), shared)
    e = handles[D]
    G.install_four(e, "daddpg" if shared else "datd3", f["nets"], f["bound"])
    worst = 0.0
    for n in BATCHES:
        a, q1, q2, pk = (G.np_(t) for t in e.datd3_forward(torch.from_numpy(f["x"][:n]).to(G.DEV), want_q=True))
        assert a.shape == (n, 3) and q1.shape == q2.shape == pk.shape == (n,)
        r, ok = G.four_ok(dict(action=a, q1=q1, q2=q2, picked=pk), R.head(f["b"], n))
        assert ok, (n, r)
        worst = max(worst, r["q1"], r["q2"], r["action"])
    record_property("ratio", worst)


@pytest.mark.parametrize("n", [64, 320])
@pytest.mark.parametrize("policy", ["actor", "actor_f16x3", "datd3", "daddpg"])
@pytest.mark.parametrize("D", [6, 9])
def test_fused_rollout_actions_within_the_derived_bounds(record_property, D, policy, n):
    """the mixed-scale nets as the fused policy with noise_sigma = 0 (the action is then clip(a, +-action_bound), which moves no
    reference value and is 1-Lipschitz): the actions of rollout(1) from reset()'s observation within the same bound of the float64
    forward of that observation.  320 envs: a ragged workgroup with one live wave (actor_forward_wg_f16x3_impl<IN, false>)."""
    e = G.handle(D, n, seed=5)
    kw = dict(noise_sigma=0.0, noise_clip=K.BOUND)
    try:
        if policy in G.KINDS:
            net, _ = K.mixed_single(D, max(BATCHES))
            G.install_single(e, policy, net, K.BOUND, **kw)
        else:
            nets = K.mixed_four(D, max(BATCHES), policy == "daddpg")["nets"]
            G.install_four(e, policy, nets, K.BOUND, **kw)
        obs = G.np_(e.reset()).copy()
        acts = G.np_(e.rollout(1, None, want_actions=True)["actions"])[0]
    finally:
        e.close()
    assert acts.shape == (n, 3) and np.all(np.isfinite(acts))
    if policy in G.KINDS:
        b = (R.bound_f16x3 if policy == "actor_f16x3" else R.bound_f32)(net, obs, K.BOUND, full=True)
        worst = G.ratio(acts, b["ref"]["out"], b["out"])
    else:
        b = R.bound_take_action(nets, obs, K.BOUND)         # clear rows: the picked actor's action; ambiguous rows: either actor's
        clear, pk = R.clear_rows(b), b["ref"]["picked"] == 1
        r1 = (np.abs(acts - b["ref"]["a1"]) / b["a1"]).max(1)
        r2 = (np.abs(acts - b["ref"]["a2"]) / b["a2"]).max(1)
        worst = float(np.where(clear, np.where(pk, r2, r1), np.minimum(r1, r2)).max())
    record_property("ratio", worst)
    assert worst <= 1.0, worst
