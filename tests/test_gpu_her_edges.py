"""The episode index and the HER sampler on cuda:0 against the case table of tests/her_cases.py: index_episodes_kernel and
her_sample_kernel through TrajectoryStore, their _pop forms through PopulationTrajectoryStore.  The rings are filled directly
(_allocate, copy, base / T / at_reset, _index), every expectation comes from the CPU (oracle.her on the linear window; the picks of the
draw block from the host's Philox), and EVERY element of every output is compared bit for bit -- floats as int32.  The outputs are
pre-filled with a sentinel and end in a guard region that must come back untouched."""
import numpy as np
import pytest
import torch

import her_cases as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                   # rows behind every output
SENTINEL = {torch.float32: 0x5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5}
TAILS = dict(states=None, actions=(3,), next_states=None, rewards=(), dones=(), picks=(4,))
DTYPES = dict(states=torch.float32, actions=torch.float32, next_states=torch.float32, rewards=torch.float32, dones=torch.uint8,
              picks=torch.int32)


@pytest.fixture(scope="module")
def table():
    return H.build()


def _store(members, cap, seed=0):
    from armenv.replay import PopulationTrajectoryStore, TrajectoryStore
    if members is None:
        return TrajectoryStore(device=DEV, seed=seed, capacity_steps=cap)
    return PopulationTrajectoryStore(members, device=DEV, seed=seed, capacity_steps=cap)


def _fill(st, rings, base, T, at_reset):
    """copies host rings into the store's (allocated) ring, sets the window and indexes it; rings: key -> array with the lead in front"""
    r = st._ring
    for k, v in rings.items():
        r[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    r["base"], r["T"], r["at_reset"] = int(base), int(T), bool(at_reset)
    st._started = True
    r["episodes"].fill_(-7)
    st._index()


def _filled(S, members=None, seed=0):
    """a store holding the table store S -- a population: S in every member, or member p holding S[p] of a list of stores of one
    geometry -- indexed, every member's index checked against the oracle"""
    each = list(S) if isinstance(S, (list, tuple)) else [S] * (members or 1)
    S = each[0]
    assert len(each) == (members or 1) and all(tuple(M[k] for k in H.GEOMETRY) == tuple(S[k] for k in H.GEOMETRY) for M in each)
    st = _store(members, S["cap"], seed)
    st._allocate(S["N"], S["D"])
    _fill(st, {k: each[0][k] if members is None else np.stack([M[k] for M in each]) for k in ("obs0",) + H.RINGS},
          S["base"], S["T"], S["at_reset"])
    got = st._ring["episodes"].cpu().numpy().reshape((members or 1, -1, 3))
    sizes = [st.size()] if members is None else st.sizes()
    for p, M in enumerate(each):
        eps = H.episodes_of(M)
        assert sizes[p] == len(eps), (M["name"], p)
        assert np.array_equal(got[p, :len(eps)], eps) and (got[p, len(eps):] == -7).all(), (M["name"], p)
    return st


def _outputs(lead, B, D):
    """(out dict for sample(out=...), the whole buffers): every output is the front of a sentinel-filled buffer with GUARD rows behind"""
    rows = int(np.prod(lead, dtype=np.int64)) * B
    out, whole = {}, {}
    for k, tail in TAILS.items():
        tail = (D,) if tail is None else tail
        dt = DTYPES[k]
        raw = torch.full((rows + GUARD,) + tail, SENTINEL[dt], dtype=torch.uint8 if dt == torch.uint8 else torch.int32, device=DEV)
        whole[k] = raw
        out[k] = raw.view(dt)[:rows].view(tuple(lead) + (B,) + tail)
    return out, whole


def _mismatches(whole, want, label):
    """rows of the outputs that differ from `want` (key -> array, lead flattened) in any bit, and the guard check"""
    bad = set()
    for k, raw in whole.items():
        got = raw.cpu().numpy()
        w = H.bits(want[k]).reshape((-1,) + got.shape[1:])
        rows = len(w)
        assert rows + GUARD == len(got), (label, k)
        assert (got[rows:] == (SENTINEL[DTYPES[k]] & (0xFF if got.dtype == np.uint8 else 0xFFFFFFFF))).all(), (label, k, "guard written")
        bad |= set(np.flatnonzero((got[:rows] != w).reshape(rows, -1).any(axis=1)).tolist())
    return sorted(bad)


def _run_picks(st, S, picks_by_member, label):
    """samples the store with forced picks ([P or 1][B][4]) and returns the rows that differ from oracle.her, as
    (label, member, row); S: the table store the store holds, or the list of its members' stores"""
    each = list(S) if isinstance(S, (list, tuple)) else [S] * len(picks_by_member)
    S = each[0]
    members = getattr(st, "members", None)
    lead = () if members is None else (members,)
    P, B = len(picks_by_member), picks_by_member.shape[1]
    out, whole = _outputs(lead, B, S["D"])
    pk = picks_by_member if members is not None else picks_by_member[0]
    got = st.sample(B, use_her=True, dis_threshold=S["thr"], her_ratio=0.8, picks=pk, return_picks=True, out=out)
    assert got is out
    torch.cuda.synchronize()
    exp = [H.expected(each[p], picks_by_member[p]) for p in range(P)]
    want = {k: np.concatenate([e[k] for e in exp]) for k in H.BATCH}
    want["picks"] = picks_by_member.reshape(-1, 4)                      # picks_out must equal picks_in
    return [(label, r // B, r % B) for r in _mismatches(whole, want, label)]


def _rotations(S, P=3):
    """the same picks in P different orders, and each row's family"""
    B = len(S["picks"])
    order = [np.roll(np.arange(B), -p * (B // P)) for p in range(P)]
    return np.stack([S["picks"][o] for o in order]), [S["family"][o] for o in order]


def _block(table, block, D=None):
    return [S for S in table["stores"] if S["block"] == block and D in (None, S["D"])]


# ------------------------------------------------------------------------------------------------ index

def test_index_block_single_and_population():
    from oracle import her
    stores = {}
    for cap, T, N, base, at_reset in H.index_cases():
        phys, window = H.index_done(cap, T, N, base)
        if (cap, N) not in stores:
            stores[cap, N] = _store(None, cap), _store(3, cap)
            for st in stores[cap, N]:
                st._allocate(N, 6)
        single, pop = stores[cap, N]
        # the population's member p holds the columns rotated by 5 p: three different indexes of one geometry
        shift = [0, 5 % N, 10 % N]
        for st, members in ((single, [phys]), (pop, [np.roll(phys, -s, axis=1) for s in shift])):
            _fill(st, dict(done=members[0] if st is single else np.stack(members)), base, T, at_reset)
            r = st._ring
            counts = r["counts"].cpu().numpy().reshape(len(members), N)
            eps_got = r["episodes"].cpu().numpy().reshape(len(members), cap * N, 3)
            num = r["num_episodes"].cpu().numpy().reshape(-1)
            for p, s in enumerate(shift[:len(members)]):
                eps = her.index_episodes(np.roll(window, -s, axis=1), starts_at_reset=bool(at_reset))
                label = (cap, T, N, base, at_reset, "pop" if st is pop else "single", p)
                assert num[p] == len(eps), label
                assert np.array_equal(counts[p], np.bincount(eps[:, 0], minlength=N)), label
                assert np.array_equal(eps_got[p, :len(eps)], eps), label
                assert (eps_got[p, len(eps):] == -7).all(), label               # rows from E on are not written


# ------------------------------------------------------------------------------------------------ forced picks

@pytest.mark.parametrize("D", [6, 9])
def test_addressing_block_every_pick_of_every_window(table, D):
    bad = []
    for S in _block(table, "addressing", D):
        bad += _run_picks(_filled(S), S, S["picks"][None], S["name"])
        # the population: three members of this geometry, member p with the env columns rotated by p -- its own index, picks and values
        members = [H.rolled(S, p) for p in range(3)]
        assert not np.array_equal(members[1]["picks"], S["picks"])
        bad += _run_picks(_filled(members, members=3), members, np.stack([M["picks"] for M in members]), S["name"] + ".pop")
    assert not bad, bad[:20]


def test_threshold_block_every_case(table):
    bad = []
    for S in _block(table, "threshold"):
        for label, p, b in _run_picks(_filled(S), S, S["picks"][None], S["name"]):
            bad.append((label, b, str(S["family"][b])))
        picks, family = _rotations(S)
        for label, p, b in _run_picks(_filled(S, members=3), S, picks, S["name"] + ".pop"):
            bad.append((label, p, b, str(family[p][b])))
    print("cases that differ:", sorted({(b[0], b[-1]) for b in bad}))
    assert not bad, (len(bad), bad[:40])


@pytest.mark.parametrize("B", [255, 256, 257])
def test_guard_regions_around_the_block_size(table, B):
    for S in (_block(table, "addressing", 6)[3], _block(table, "addressing", 9)[-1]):
        assert 0 < len(S["picks"]) < 255
        picks = np.resize(S["picks"], (B, 4))                                                     # the picks, repeated up to B
        assert not _run_picks(_filled(S), S, picks[None], S["name"])
        assert not _run_picks(_filled(S, members=3), S, np.stack([picks, picks[::-1], np.roll(picks, 1, axis=0)]), S["name"] + ".pop")


# ------------------------------------------------------------------------------------------------ own draws

def test_draw_block_picks_are_the_hosts_philox_and_values_follow(table):
    bad = []
    for S in _block(table, "draw"):
        single = _filled(S)
        for d in S["draws"]:
            P, B = d["members"], d["B"]
            if P == 1:
                st, lead = single, ()
            else:
                st, lead = _filled(S, members=P, seed=d["seed"]), (P,)
            st.seed, st._bound, st._draw = d["seed"], None, d["draw"]
            out, whole = _outputs(lead, B, S["D"])
            st.sample(B, use_her=bool(d["use_her"]), dis_threshold=S["thr"], her_ratio=d["her_ratio"], return_picks=True, out=out)
            torch.cuda.synchronize()
            assert st._draw == d["draw"] + 1
            exp = [H.expected(S, d["picks"][p]) for p in range(P)]
            want = {k: np.concatenate([e[k] for e in exp]) for k in H.BATCH}
            want["picks"] = d["picks"].reshape(-1, 4)
            label = (S["name"], B, d["seed"], d["draw"], d["her_ratio"], d["use_her"], P)
            bad += [(label, r) for r in _mismatches(whole, want, label)]
    assert not bad, bad[:20]
