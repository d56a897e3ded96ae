"""The rollouts' exploration noise on cuda:0 (csrc/armenv_env.h policy_noise) against the float64 reference of tests/noise_ref.py,
element by element within the bound DERIVED there (no tolerance in this file is a constant), on the cases of tests/noise_cases.py.

Observing the draw: the `random` policy with noise_sigma = 1 and noise_clip = 8 -- above the largest possible |z| = 6.66 -- makes
rollout(..., want_actions=True) return the three normals themselves (z * 1 is exact, the clip moves nothing).  No action may equal
+-8: fminf(fmaxf(NaN, -clip), clip) is -clip, which is how a NaN from the noise would show.

  - the planted edge keys (u = 1, the steps next to it, the deep tail, the quadrant boundaries and ties), one tuple per env and launch;
  - random blocks at the key boundaries (seed and global id past 2^32, a seed past 2^63, episode counters that wrap) through every
    compiled context that calls policy_noise: lockstep rollout, lane-asynchronous rollout (count and straggler rule), two waves per SIMD,
    half-filled waves, the step kernel -- all of which must also agree bit for bit;
  - the fused policies with all-zero nets (mu = 0 exactly), and a real net with sigma = 0.5 for the fmaf that joins the two halves;
  - keying: reset draws against the oracle across a wrapping episode counter, two shards against one handle across 2^32.

Each test records max(err / bound); ARMENV_NOISE_MARGINS=<path> writes them as JSON (profiles/policy_noise_margins.json)."""
import json
import os

import numpy as np
import pytest
import torch

import actor_cases as K
import actor_ref64 as R
import actor_ref64_gpu as G
import noise_cases as NC
import noise_ref as NR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMA, CLIP = 1.0, 8.0
MAX_STEPS = 10          # random blocks: every env is reset in place twice within the 32 steps
FULL = dict(rollout_waves_per_simd=1, rollout_lanes_per_wave=64)
SCHEDULES = (
    ("lockstep", dict(FULL, rollout_ready_lanes=0, rollout_straggler_trips=0)),
    ("count33", dict(FULL, rollout_ready_lanes=33, rollout_straggler_trips=0)),
    ("straggler33", dict(FULL, rollout_ready_lanes=33, rollout_straggler_trips=3)),
    ("two_waves", dict(rollout_ready_lanes=0, rollout_straggler_trips=0, rollout_waves_per_simd=2, rollout_lanes_per_wave=64)),
    ("half_waves", dict(rollout_ready_lanes=0, rollout_straggler_trips=0, rollout_waves_per_simd=1, rollout_lanes_per_wave=32)),
)
BOUNDARY_BLOCKS = ("seed-past-2^63", "counter-wraps")
MARGINS = {}


@pytest.fixture(scope="module")
def envs():
    from armenv import envs
    return envs


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    path = os.environ.get("ARMENV_NOISE_MARGINS")
    if path and MARGINS:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        out = dict(what="max |policy_noise on the GPU - float64| / derived bound (tests/noise_ref.py) per test and call site of "
                        "tests/test_gpu_noise_ref.py; every figure must be at most 1",
                   bound_relative_size="6.5 .. 8.2 times 2^-24", largest=max(MARGINS.values()), margins=MARGINS)
        with open(path, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _u32(a):
    """u32 bits as the int32 tensor set_state takes"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy())


def _env_class(envs, task):
    return dict(reach=envs.BatchedReachEnv, push=envs.BatchedPushEnv, pick=envs.BatchedPickEnv)[task]


def _handle(envs, task, n, b, **kw):
    """a handle at the keying of block b whose random policy returns the draw itself, reset, at episode counter b["counter"]"""
    e = _env_class(envs, task)(n, device=DEV, seed=b["seed"], env_id_offset=b["offset"], auto_reset=True, **kw)
    e.set_policy("random", action_bound=0.7, noise_sigma=SIGMA, noise_clip=CLIP)
    e.reset()
    e.set_state(episode=_u32(np.full(n, b["counter"], dtype=np.uint32)))
    return e


def _check_draws(acts, ref, bnd):
    """the actions ARE the draws: finite, none at the clip (a NaN's image), within the bound; returns max err / bound"""
    assert acts.dtype == np.float32 and acts.shape == ref.shape
    assert np.all(np.isfinite(acts)) and np.abs(acts).max() < CLIP
    return NR.ratio(acts, ref, bnd)


def _note(record_property, name, r):
    record_property("ratio", r)
    MARGINS[name] = max(MARGINS.get(name, 0.0), r)
    print("%s: err / bound %.3f" % (name, r))


# ------------------------------------------------------------------ planted edge keys

@pytest.mark.parametrize("schedule", ["lockstep", "count33"])
def test_planted_edge_keys_within_the_bound(envs, record_property, schedule):
    """every tuple of tests/golden/noise_edge_keys.npz planted through set_state(episode = index + 1, step =) on its env, one launch of
    rollout(1) per group of tuples, by the lockstep and by the lane-asynchronous kernel: every output of every env (planted or not)
    within the bound, and the u = 1 draws exactly +-0"""
    k = NC.edge_keys()
    e = _env_class(envs, "reach")(NC.EDGE_ENVS, device=DEV, seed=k["seed"], env_id_offset=k["offset"], max_steps=2 * NC.EDGE_STEPS,
                                  **dict(SCHEDULES)[schedule])
    e.set_policy("random", action_bound=0.7, noise_sigma=SIGMA, noise_clip=CLIP)
    e.reset()
    ids = np.uint64(k["offset"]) + np.arange(NC.EDGE_ENVS, dtype=np.uint64)
    worst, seen = 0.0, 0
    try:
        for counter, step, rows in NC.edge_launches(k):
            e.set_state(episode=_u32(counter), step=torch.from_numpy(step))
            acts = _np(e.rollout(1, None, want_actions=True)["actions"])[0]
            w = NR.words(k["seed"], ids, (counter.astype(np.int64) - 1) & 0xFFFFFFFF, step)
            member = NC.classify(w)
            for i in np.nonzero(rows >= 0)[0]:
                assert member[i, k["cls"][rows[i]]]                                     # the launch planted what the fixture says
                name = NC.CLASSES[k["cls"][rows[i]]]
                if name == "a:rad-one":
                    assert acts[i, 0] == 0 and acts[i, 1] == 0, (name, acts[i])
                elif name == "b:rad-one":
                    assert acts[i, 2] == 0, (name, acts[i])
                seen += 1
            r = _check_draws(acts, NR.reference(w), NR.bound(w))
            assert r <= 1.0, (r, np.argwhere(np.abs(acts - NR.reference(w)) > NR.bound(w)))
            worst = max(worst, r)
    finally:
        e.close()
    assert seen == len({(a, b, c) for a, b, c in zip(k["env"], k["episode"], k["step"])})
    _note(record_property, "edge-keys/" + schedule, worst)


# ------------------------------------------------------------------ random blocks through every call site

def _run_block(envs, task, n, b, schedule, precision, by_step=False):
    e = _handle(envs, task, n, b, precision=precision, max_steps=MAX_STEPS, **schedule)
    try:
        if by_step:
            rows = []
            for _ in range(NC.BLOCK_STEPS):
                o, r, d, s = e.step(None)
                rows.append((_np(o), _np(r), _np(d)))
            out = dict(obs=np.stack([x[0] for x in rows]), reward=np.stack([x[1] for x in rows]), done=np.stack([x[2] for x in rows]))
        else:
            o = e.rollout(NC.BLOCK_STEPS, None, want_actions=True)
            out = {kk: _np(o[kk]) for kk in ("obs", "reward", "done", "actions")}
        st = e.get_state()
        out["state"] = {kk: _np(v) for kk, v in st.items()}
    finally:
        e.close()
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _block_test(envs, record_property, task, precision, n, blocks, schedules, tag):
    worst = 0.0
    for bid in blocks:
        b = NC.block(bid)
        base = None
        for name, over in schedules:
            out = _run_block(envs, task, n, b, over, precision)
            ref, bnd = NC.block_reference(b, n=n, done=out["done"])
            r = _check_draws(out["actions"], ref, bnd)
            assert r <= 1.0, (bid, name, r)
            worst = max(worst, r)
            MARGINS["%s/%s" % (tag, name)] = max(MARGINS.get("%s/%s" % (tag, name), 0.0), r)
            resets = out["done"].sum(0)
            assert resets.min() >= 2, (bid, name, resets.min())              # the counter moved twice on every env
            if base is None:
                base = out
            else:
                for kk in ("actions", "obs", "reward", "done"):
                    assert _same_bits(out[kk], base[kk]), (bid, name, kk)
                for kk in base["state"]:
                    assert _same_bits(out["state"][kk], base["state"][kk]), (bid, name, kk)
        # the step kernel returns no actions: its outputs and state are the rollout's, bit for bit, so its draws were
        out = _run_block(envs, task, n, b, schedules[0][1], precision, by_step=True)
        for kk in ("obs", "reward", "done"):
            assert _same_bits(out[kk], base[kk]), (bid, "step", kk)
        for kk in base["state"]:
            assert _same_bits(out["state"][kk], base["state"][kk]), (bid, "step", kk)
    record_property("ratio", worst)
    print("%s: err / bound %.3f" % (tag, worst))


@pytest.mark.parametrize("n", [64, 64 + 32 + 7])
@pytest.mark.parametrize("precision", [64, 32])
def test_reach_random_blocks_every_call_site(envs, record_property, precision, n):
    """reach, both precisions, a full and a ragged batch: every keying at n = 64 on f64 (the two boundary keyings elsewhere) through
    the five rollout builds and the step kernel"""
    blocks = [b["id"] for b in NC.BLOCKS] if (precision, n) == (64, 64) else BOUNDARY_BLOCKS
    _block_test(envs, record_property, "reach", precision, n, blocks, SCHEDULES, "reach-f%d-n%d" % (precision, n))


@pytest.mark.parametrize("n", [64, 64 + 32 + 7])
@pytest.mark.parametrize("task", ["push", "pick"])
def test_cube_tasks_random_blocks_default_schedule(envs, record_property, task, n):
    """push and pick on f64 with the schedule their defaults choose (lane-asynchronous, half-filled waves where they apply), and the
    step kernel"""
    _block_test(envs, record_property, task, 64, n, BOUNDARY_BLOCKS, (("default", {}),), "%s-f64-n%d" % (task, n))


# ------------------------------------------------------------------ fused policies

def _zero_net(in_dim, rows):
    z = lambda *s: np.zeros(s, dtype=np.float32)
    return {"fc1.weight": z(256, in_dim), "fc1.bias": z(256), "fc2.weight": z(256, 256), "fc2.bias": z(256),
            "fc3.weight": z(rows, 256), "fc3.bias": z(rows)}


def _install(e, policy, actor, critic, **kw):
    if policy in G.KINDS:
        G.install_single(e, policy, actor, K.BOUND, **kw)
    else:
        G.install_four(e, policy, (actor, actor, critic, critic), K.BOUND, **kw)


@pytest.mark.parametrize("n", [64, 320])
@pytest.mark.parametrize("policy", ["actor", "actor_f16x3", "datd3", "daddpg"])
@pytest.mark.parametrize("D", [6, 9])
def test_fused_policies_with_zero_nets_return_the_draw(record_property, D, policy, n):
    """all-zero nets: mu = bound * tanh(0) = 0 exactly, so fmaf(z, 1, 0) is the draw -- the fused-actor rollouts' own call of
    policy_noise (no carried frame, MFMA phases between the steps), at the wrapping-counter keying, full and ragged workgroups"""
    b = NC.block("counter-wraps")
    e = G.handle(D, n, seed=b["seed"], env_id_offset=b["offset"], max_steps=MAX_STEPS)
    try:
        _install(e, policy, _zero_net(D, 3), _zero_net(D + 3, 1), noise_sigma=SIGMA, noise_clip=CLIP)
        e.reset()
        e.set_state(episode=_u32(np.full(n, b["counter"], dtype=np.uint32)))
        out = e.rollout(NC.BLOCK_STEPS, None, want_actions=True)
        acts, done = _np(out["actions"]), _np(out["done"])
    finally:
        e.close()
    ref, bnd = NC.block_reference(b, n=n, done=done)
    r = _check_draws(acts, ref, bnd)
    assert done.sum(0).min() >= 2
    _note(record_property, "fused-zero-nets/%s-D%d-n%d" % (policy, D, n), r)
    assert r <= 1.0, r


@pytest.mark.parametrize("policy", G.KINDS)
def test_fused_actor_plus_noise_within_the_joined_bound(record_property, policy):
    """the mixed-scale net of tests/actor_cases.py with noise_sigma = 0.5: a = clip(fmaf(z, 0.5, mu), +-0.7) within
    actor bound + 0.5 * noise bound + one f32 rounding of clip(mu_ref + 0.5 z_ref) (the clip is 1-Lipschitz and moves no reference
    value by more than it moves the kernel's)"""
    D, n, sigma = 6, 320, 0.5
    b = NC.block("seed-high-word")
    net, _ = K.mixed_single(D, 1024 + 192)
    e = G.handle(D, n, seed=b["seed"], env_id_offset=b["offset"])
    try:
        G.install_single(e, policy, net, K.BOUND, noise_sigma=sigma, noise_clip=K.BOUND)
        obs = _np(e.reset())
        acts = _np(e.rollout(1, None, want_actions=True)["actions"])[0]
    finally:
        e.close()
    ab = (R.bound_f16x3 if policy == "actor_f16x3" else R.bound_f32)(net, obs, K.BOUND, full=True)
    w = NR.words(b["seed"], np.uint64(b["offset"]) + np.arange(n, dtype=np.uint64), 0, 0)       # the first episode's first step
    zr, zb = NR.reference(w), NR.bound(w)
    v = ab["ref"]["out"] + sigma * zr
    bnd = ab["out"] + sigma * zb
    bnd = bnd + NR.EPS * (np.abs(v) + bnd)
    ref = np.clip(v, -np.float64(np.float32(K.BOUND)), np.float64(np.float32(K.BOUND)))
    assert np.all(np.isfinite(acts)) and np.abs(acts).max() <= np.float32(K.BOUND)
    inside = np.abs(v) < K.BOUND
    assert 0.3 < inside.mean() < 1.0                                        # both sides of the clip occur
    r = NR.ratio(acts, ref, bnd)
    _note(record_property, "fused-mixed-net-sigma0.5/" + policy, r)
    assert r <= 1.0, r


# ------------------------------------------------------------------ keying

@pytest.mark.parametrize("task", ["reach", "push", "pick"])
def test_reset_draws_match_the_oracle_across_a_wrapping_counter(envs, O, kuka, task):
    """goals (reach) and placements (push, pick) at seed >= 2^63 and global ids across 2^32: reset() at episode counter 0xFFFFFFFE, then
    the in-place resets of a rollout at counters 0xFFFFFFFF, 0 and 1 -- each equal to the oracle's draw for that counter, bit for bit"""
    n, b = 64, NC.block("counter-wraps")
    reset = dict(reach=O.reach_reset, push=O.push_reset, pick=O.pick_reset)[task]
    State = dict(reach=O.ReachState, push=O.PushState, pick=O.PickState)[task]
    cfg = O.default_config(task)

    def oracle(counter):
        st = State(n)
        st.episode[:] = counter
        obs = reset(kuka, cfg, st, seed=b["seed"], env_id0=b["offset"])
        assert np.all(st.episode == np.uint32((counter + 1) & 0xFFFFFFFF))
        return obs[:, 3:].copy()

    e = _env_class(envs, task)(n, device=DEV, seed=b["seed"], env_id_offset=b["offset"], max_steps=3)
    try:
        e.set_policy("random")
        e.reset()
        e.set_state(episode=_u32(np.full(n, 0xFFFFFFFE, dtype=np.uint32)))
        first = _np(e.reset())
        assert _same_bits(first[:, 3:], oracle(0xFFFFFFFE))
        out = e.rollout(16, None)
        obs, done = _np(out["obs"]), _np(out["done"])
        final = _np(e.get_state()["episode"]).view(np.uint32)
    finally:
        e.close()
    want = {}
    counter = np.full(n, 0xFFFFFFFF, dtype=np.int64)
    compared = 0
    for t in range(obs.shape[0]):
        for i in np.nonzero(done[t])[0]:
            c = int(counter[i])
            if c not in want:
                want[c] = oracle(c)
            assert _same_bits(obs[t, i, 3:], want[c][i]), (t, i, hex(c))
            counter[i] = (counter[i] + 1) & 0xFFFFFFFF
            compared += 1
    assert done.sum(0).min() >= 3 and compared >= 3 * n and {0xFFFFFFFF, 0, 1} <= set(want)    # every env went through the wrap
    assert np.array_equal(final.astype(np.int64), counter)


def test_two_shards_across_2_pow_32_reproduce_one_handle(envs):
    """two 32-env handles at offsets 2^32 - 32 and 2^32 against the 64-env handle at 2^32 - 32, 32 steps of the random policy:
    outputs, actions and state bit for bit (a shard that dropped the id's high word, or added its offset in 32 bits, would not)"""
    b = NC.block("ids-across-2^32")
    kw = dict(precision=64, max_steps=MAX_STEPS, **dict(SCHEDULES)["lockstep"])

    def run(n, offset):
        e = _handle(envs, "reach", n, dict(b, offset=offset), **kw)
        try:
            o = e.rollout(NC.BLOCK_STEPS, None, want_actions=True)
            out = {kk: _np(o[kk]) for kk in ("obs", "reward", "done", "success", "actions")}
            state = {kk: _np(v) for kk, v in e.get_state().items()}
        finally:
            e.close()
        return out, state

    whole, ws = run(64, b["offset"])
    lo, ls = run(32, b["offset"])
    hi, hs = run(32, b["offset"] + 32)
    assert b["offset"] + 32 == 2 ** 32
    for kk in whole:
        assert _same_bits(np.concatenate([lo[kk], hi[kk]], 1), whole[kk]), kk
    for kk in ws:
        assert _same_bits(np.concatenate([ls[kk], hs[kk]], 0), ws[kk]), kk
    assert not _same_bits(lo["actions"], hi["actions"])
