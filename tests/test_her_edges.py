"""The trajectory store's edge cases on the CPU (tests/her_cases.py): the table's own conditions, oracle.her against the reference's
recorded word on them (tests/golden/her_edges_*.npz, G17), and the sensitivity of the table -- a numpy restatement of
her_sample_one agrees with oracle.her on every case, and each planted defect is caught by at least one."""
import numpy as np
import pytest

import her_cases as H
from conftest import golden_npz
from oracle import her


@pytest.fixture(scope="module")
def table():
    return H.build()


@pytest.fixture(scope="module", params=["reach", "push"])
def fixture(request):
    return H.load_fixture(golden_npz(f"her_edges_{request.param}.npz"))


def test_the_table_holds_its_conditions_fresh_and_loaded(table, fixture):
    H.check(table, whole=True)
    H.check(fixture)
    D = fixture["stores"][0]["D"]
    fresh = {S["name"]: S for S in H.fixture_stores(table, D)}
    assert list(fresh) == [S["name"] for S in fixture["stores"]] and len(fresh) == 4
    for S in fixture["stores"]:                                     # the fixture holds the table's inputs, bit for bit
        F = fresh[S["name"]]
        assert all(S[k] == F[k] for k in H.GEOMETRY) and S["thr"] == F["thr"]
        for k in ("obs0",) + H.RINGS + ("picks",):
            assert np.array_equal(H.bits(S[k]), H.bits(F[k])), (S["name"], k)
        assert S["family"].tolist() == F["family"].tolist()


def test_the_index_block_expectations_are_the_patterns_own_episodes():
    """oracle.her.index_episodes on the 32 patterns: pattern n with bits b has popcount(b) complete episodes after a reset and one
    fewer without (none for 0), and their lengths are the gaps between set bits"""
    for cap, T, N, base, at_reset in H.index_cases():
        _, window = H.index_done(cap, T, N, base)
        eps = her.index_episodes(window, starts_at_reset=bool(at_reset))
        for n in range(N):
            ones = [t for t in range(T) if (n % 32) >> t & 1]
            mine = eps[eps[:, 0] == n]
            starts = ([0] if at_reset else []) + [t + 1 for t in ones]
            want = [(s, e - s + 1) for s, e in zip(starts, ones if at_reset else ones[1:])]
            assert [tuple(r[1:]) for r in mine.tolist()] == want, (cap, T, N, base, at_reset, n)


def test_oracle_her_equals_the_reference_on_every_edge_case(fixture):
    """states, next states, actions and dones exactly; rewards as np.float32 of the reference's Python floats, by their bits"""
    for S in fixture["stores"]:
        got, ref = H.expected(S), S["ref"]
        assert len(S["picks"]) == len(ref["dones"]) > 0
        for k in ("states", "next_states"):
            assert ref[k].dtype == np.float64 and np.array_equal(got[k].astype(np.float64), ref[k]), (S["name"], k)
        assert np.array_equal(H.bits(got["actions"]), H.bits(ref["actions"])), S["name"]
        assert np.array_equal(got["dones"], ref["dones"]), S["name"]
        assert np.array_equal(H.bits(got["rewards"]), H.bits(ref["rewards"].astype(np.float32))), S["name"]
        planted = S["family"] != "aux"
        if S["block"] == "threshold":                                # the planted picks alone already split both ways, or all one way
            far = ref["dones"][planted & (S["picks"][:, 2] == 1)] == 0
            assert np.array_equal(ref["rewards"][planted][far], np.full(far.sum(), -0.1)) and len(far) >= 24


def _draw_batches(S, defect=None):
    """(label, expected, emulated) of every draw of a draw store: picks from the uniforms, values from the picks"""
    eps = H.episodes_of(S)
    for d in S["draws"]:
        for p in range(d["members"]):
            u = H.philox_uniforms((d["seed"] + p) & H.M64, d["draw"], d["B"])
            pk = H.picks_from_uniforms(u, eps, d["her_ratio"], d["use_her"], defect=defect)
            yield (S["name"], d["B"], d["seed"], d["draw"], d["her_ratio"], d["use_her"], p), d["picks"][p], pk


def _disagreements(table, defect):
    """every case on which her_sample_one with `defect` differs from the expectation, in table order: [(store, row, family, key)]
    with the first differing key of that row"""
    out = []
    for S in table["stores"]:
        if S["block"] == "draw":
            if defect not in (None, "sg_upper"):
                continue
            for label, want, got in _draw_batches(S, defect):
                out.extend((label, int(b), "draw", "picks") for b in np.flatnonzero((want != got).any(axis=1)))
                if defect is None:
                    e, w = H.emu_sample(S, want), H.expected(S, want)
                    out.extend((label, int(b), "draw", "values") for b in range(len(want))
                               if H.first_difference({k: e[k][b:b + 1] for k in H.BATCH}, {k: w[k][b:b + 1] for k in H.BATCH}))
            continue
        e, w = H.emu_sample(S, defect=defect), S["expect"]
        rows = np.flatnonzero(np.any([(H.bits(e[k]) != H.bits(w[k])).reshape(len(S["picks"]), -1).any(axis=1) for k in H.BATCH], axis=0))
        out.extend((S["name"], int(b), str(S["family"][b]), H.first_difference({k: e[k][b:b + 1] for k in H.BATCH},
                                                                                {k: w[k][b:b + 1] for k in H.BATCH})[0]) for b in rows)
    return out


@pytest.fixture(scope="module")
def expectations(table):
    for S in table["stores"]:
        if S["block"] != "draw":
            S["expect"] = H.expected(S)
    return table


def test_the_restated_kernel_agrees_with_the_oracle_on_the_whole_table(expectations):
    assert _disagreements(expectations, None) == []


# defect -> the family (or block) built to catch it: at least one of its cases must
BUILT_FOR = dict(thr_f32=("eq", "between"), ge=("eq", "exact"), f32_at_9=("f32",), sum_order=("order",), fused=("fma",),
                 obs_after_for_next=("all",), obs0_ignored=("all",), no_ring=("all",), row_off_by_one=("all",), sg_upper=("draw",),
                 keep_6_9=("all",), goal_state_only=("all",))


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_every_planted_defect_is_caught(expectations, defect):
    hits = _disagreements(expectations, defect)
    assert hits, defect
    print(defect, "first caught by", hits[0], "--", len(hits), "cases in all")
    assert set(BUILT_FOR[defect]) <= {h[2] for h in hits}, (defect, sorted({h[2] for h in hits}))
    if defect in ("sum_order", "fused", "f32_at_9"):                 # and by that family in both variants it was built in
        fam = BUILT_FOR[defect][0]
        assert {h[0][:6] for h in hits if h[2] == fam} == ({"thr.D6", "thr.D9"} if defect != "f32_at_9" else {"thr.D9"})


def test_the_f32_threshold_flips_exactly_the_cases_on_the_rounding_band(expectations):
    """What rounding dis_threshold to f32 changes, case by case: the relabelled picks whose dis lies on the band between thr and
    (double)(float)thr -- at 0.1 (f32 rounds up) dis in (thr, f32 thr], far in the reference and near with the rounded threshold; at
    0.7 (rounds down) dis in (f32 thr, thr], the other way, which no f32 dis of reach can hit; none at 0.25 and none in the addressing
    block.  All of reach's `eq` cases at 0.1 and of push's `between` cases at 0.1 and 0.7 are among them, and nothing but reward and
    done of those picks moves."""
    flipped = {}
    for S in expectations["stores"]:
        if S["block"] == "draw":
            continue
        got, want = H.emu_sample(S, defect="thr_f32"), S["expect"]
        bad = got["dones"] != want["dones"]
        assert H.first_difference({k: got[k][~bad] for k in H.BATCH}, {k: want[k][~bad] for k in H.BATCH}) is None
        lin, eps, thr = H.linear(S), H.episodes_of(S), S["thr"]
        lo, hi = sorted((thr, float(np.float32(thr))))
        for b in np.flatnonzero(bad):
            ep, st, h, sg = S["picks"][b]
            n, t0, _ = eps[ep]
            dis = H.distance(lin["next_obs"][t0 + st, n, :3], lin["next_obs"][t0 + sg - 1, n, :3], S["D"])
            assert h == 1 and lo < dis <= hi and S["block"] == "threshold", (S["name"], b, dis)
            assert want["dones"][b] == (0 if thr == 0.1 else 1) and got["dones"][b] == 1 - want["dones"][b], (S["name"], b)
            assert H.bits(got["rewards"])[b] == H.bits(np.float32([1.0 if thr == 0.1 else -0.1]))[0]
            flipped.setdefault((S["D"], thr, str(S["family"][b])), []).append(int(b))
        if S["block"] == "threshold":
            fam = "eq" if S["D"] == 6 else "between"
            if (S["D"], thr) in ((6, 0.1), (9, 0.1), (9, 0.7)):
                assert set(np.flatnonzero(S["family"] == fam)) <= set(np.flatnonzero(bad)), S["name"]
            else:
                assert not bad.any(), S["name"]
    print("f32 threshold flips:", {k: len(v) for k, v in sorted(flipped.items())})
    assert {k[:2] for k in flipped} == {(6, 0.1), (9, 0.1), (9, 0.7)}
    assert all(len(flipped[k]) == 8 for k in ((6, 0.1, "eq"), (9, 0.1, "between"), (9, 0.7, "between")))
