"""The cell table of tests/cube_cells.py, checked on the CPU against the oracle: every cell lands in the branch it names, none is
ambiguous under the disagreement the engine is allowed with the oracle, the two sides of every edge differ in an asserted output by more
than the GPU test's tolerance, and every constant a decision compares against is pinned by at least one cell."""
import numpy as np
import pytest

import cube_cells as CC

# branches whose sides are not the two sides of one edge (directions, stand-alone cells)
NOT_EDGES = {"dir8_low", "dir8_low_y", "dir_fric", "m0dir8_mid", "m0dir8_mid_xy", "closed", "first", "still", "m0press", "m0sweep", "held_hi", "tmo_moving", "tmo_held", "pickfall_m0"}


def _evaluate(O, chain, cells, shift=None):
    """(task, variant) -> (cells, oracle result); shift: kwargs of make_cfg"""
    out = {}
    for (task, variant), cs in CC.groups(cells).items():
        cfg = CC.make_cfg(O, task, variant, **(shift or {}))
        out[(task, variant)] = (cs, CC.run_oracle(O, chain, task, cfg, *CC.rows_of(cs, range(len(cs)))))
    return out


def _model(O, chain, x):
    return CC.model_step(x.task, CC.constants(x.task, x.variant), CC.arms(O, chain)[x.task][x.arm], x.aux, x.step)


@pytest.fixture(scope="module")
def table(O, kuka):
    cells = CC.build_cells(O, kuka)
    return cells, _evaluate(O, kuka, cells)


def test_arm_poses_are_well_conditioned(O, kuka):
    for task, d in CC.arms(O, kuka).items():
        cfg = O.default_config(task)
        for nm, a in d.items():
            assert a["iters"] < cfg.ik_max_iters, (task, nm, a["iters"])
            assert a["pose_pivot"] >= cfg.fence_pivot and a["minpiv"] >= cfg.fence_pivot, (task, nm, a["pose_pivot"], a["minpiv"])
    # the travel gate's margins were found, not placed: between m and 10 m
    for side in ("under", "over"):
        a = CC.arms(O, kuka)["push"]["travel_" + side]
        t = np.hypot(*(a["p1"][:2] - a["p0"][:2])) - 1e-3
        assert CC.M64 <= abs(t) <= 10 * CC.M64 and (t < 0) == (side == "under")


def test_table_size_and_names(table):
    cells, _ = table
    names = [(x.task, x.variant, x.name) for x in cells]
    assert len(set(names)) == len(names) and 120 <= len(cells) <= 400, len(cells)
    assert {x.task for x in cells} == {"push", "pick"}
    assert any(x.variant == "m0" and x.task == "push" for x in cells)


def test_each_cell_lands_in_its_branch(O, kuka, table):
    cells, res = table
    A = CC.arms(O, kuka)
    seen = {}
    for (task, variant), (cs, r) in res.items():
        for i, x in enumerate(cs):
            a = A[task][x.arm]
            assert np.array_equal(r["q"][i], a["q1"]), x           # the arm's motion does not depend on the cube
            assert r["iters"][i] == a["iters"] and r["minpiv"][i] >= 1e-2, x
            m = _model(O, kuka, x)
            for k, v in x.want.items():
                assert k in m["trace"] and m["trace"][k] == v, (x, k, v, m["trace"])
            for k, v in m["trace"].items():
                seen.setdefault((task, k), set()).add(v)
            # oracle == model
            na = 9 if task == "push" else 11
            assert np.abs(r["aux"][i][:na] - m["aux"][:na]).max() <= 1e-12, (x, r["aux"][i], m["aux"])
            assert r["done"][i] == m["done"] and r["success"][i] == m["success"] and r["step"][i] == m["step"], (x, m)
            assert abs(r["reward"][i] - m["reward"]) <= 1e-12, (x, r["reward"][i], m["reward"])
            if not m["trace"]["deadband"]:      # well inside the deadband decision unless the cell is about it
                assert x.branch.startswith("dead") or abs(abs(m["test"]) - 1e-5) > 1e-4, (x, m["test"])
            if not x.branch.startswith("succ") and x.branch != "tmo_succ":
                assert abs(m["dt32"] - 0.05) > 1e-2, (x, m["dt32"])
            # closed forms / discrete expectations
            e, aux = x.expect, r["aux"][i]
            for k in ("done", "success"):
                if k in e:
                    assert r[k][i] == e[k], (x, k)
            if "reward" in e:
                assert abs(r["reward"][i] - e["reward"]) <= 1e-12, (x, r["reward"][i], e["reward"])
                if e["reward"] in (100.0, -1.0):
                    assert r["reward"][i] == e["reward"], x
            if "vel" in e:
                assert np.abs(aux[7:9] - e["vel"]).max() <= 1e-12, (x, aux[7:9], e["vel"])
                if e["vel"] == (0.0, 0.0):
                    assert not aux[7:9].any(), x
            if "untouched" in e:
                assert np.array_equal(aux[0:2], x.aux[0:2]), x
            if "xy" in e:
                assert np.abs(aux[0:2] - e["xy"]).max() <= 1e-12, (x, aux[0:2], e["xy"])
            if "z" in e:
                assert abs(aux[2] - e["z"]) <= 1e-12, (x, aux[2], e["z"])
            if "grip" in e:
                assert aux[7] == e["grip"], (x, aux[7])
            if "off" in e:
                assert np.array_equal(aux[8:11], e["off"]), x
    # every decision of the model is taken both ways somewhere in the table
    for (task, k), vals in sorted(seen.items()):
        want = {0, 1, 2, 3} if k == "face" else ({0.0, 1.0, 2.0} if k == "grip_in" else {True, False})
        assert vals == want, (task, k, vals)


@pytest.mark.parametrize("precision", [64, 32])
def test_no_cell_is_ambiguous(O, kuka, precision):
    """Placing the cells from a p1 that is off by the engine's allowed disagreement, along either direction of each axis, changes no
    cell's decisions: the trace of the model at the true p1, done, success and the gripper state.  No cell is exempt."""
    m, f32 = (CC.M64, False) if precision == 64 else (CC.M32, True)
    base = CC.build_cells(O, kuka, m=m, f32_only=f32)
    ref = [_model(O, kuka, x) for x in base]
    if precision == 32:
        assert 60 <= len(base) and all(x.f32 for x in base)
    d = CC.PERTURB[precision]
    bad = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            shift = [0.0, 0.0, 0.0]; shift[ax] = sgn * d
            moved = CC.build_cells(O, kuka, m=m, shift=shift, f32_only=f32)
            assert [x.name for x in moved] == [x.name for x in base]
            for x, r in zip(moved, ref):
                g = _model(O, kuka, x)
                same = g["trace"] == r["trace"] and g["done"] == r["done"] and g["success"] == r["success"]
                if x.task == "pick":
                    same = same and g["aux"][7] == r["aux"][7]
                if not same:
                    bad.append((x, ax, sgn))
    assert not bad, bad


@pytest.mark.parametrize("precision", [64, 32])
def test_edges_are_visible(O, kuka, precision):
    """the sides of every edge differ in an asserted output by more than the GPU test's tolerance for it (or in an exact one)"""
    m, f32 = (CC.M64, False) if precision == 64 else (CC.M32, True)
    cells = CC.build_cells(O, kuka, m=m, f32_only=f32)
    n_edges = 0
    for (task, variant), (cs, r) in _evaluate(O, kuka, cells).items():
        tol = CC.tolerances(precision, CC.constants(task, variant))
        by = {}
        for i, x in enumerate(cs):
            by.setdefault(x.branch, []).append(i)
        for branch, idx in by.items():
            if branch in NOT_EDGES:
                continue
            assert len(idx) >= 2 or precision == 32, (task, variant, branch)      # (an f64-only side leaves the f32 set a single cell)
            for i, j in zip(idx[:-1], idx[1:]):
                assert CC.differs(task, r, r, i, j, tol), (cs[i], cs[j])
                n_edges += 1
    assert n_edges >= (60 if precision == 64 else 25), n_edges


TEETH = [(k, 2 * CC.M64) for k in ("push_cube_half", "push_eef_radius", "push_tool_radius", "push_tool_below", "push_contact_split", "push_rest_z",
                                   "push_success_dis", "pick_trigger_dis", "pick_jaw_half", "pick_gripper_length", "push_drop_contact")] + \
        [("max_steps", 1), ("push_friction", ("rel", 1e-2)), ("push_contact_erp", ("rel", 1e-2))]


@pytest.mark.parametrize("const,by", TEETH, ids=[t[0] for t in TEETH])
def test_every_constant_is_pinned(O, kuka, table, const, by):
    """the oracle with one constant shifted by 2 m (either way) differs from the unshifted one beyond the GPU tolerances in at least one
    cell: a kernel that compared against a slightly wrong constant would fail the GPU test"""
    cells, base = table
    for sgn in (-1, 1):
        shift = {const: ("rel", sgn * by[1]) if isinstance(by, tuple) else sgn * by}
        hit = []
        for (task, variant), (cs, r) in _evaluate(O, kuka, cells, shift).items():
            tol = CC.tolerances(64, CC.constants(task, variant))
            hit += [(cs[i], why) for i in range(len(cs)) for why in [CC.differs(task, base[(task, variant)][1], r, i, i, tol)] if why]
        assert hit, (const, sgn)
