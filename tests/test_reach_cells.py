"""The cell table of tests/reach_cells.py, checked on the CPU: every cell lands in the branch it names under the model's trace, none is
ambiguous under the disagreement the engine is allowed with the oracle, the model and the oracle -- two independent restatements of the
step -- agree before either judges a kernel, every planted defect changes a checked output of a named cell by more than the GPU test's
tolerance, and every constant the table restates is pinned to the oracle's defaults."""
import numpy as np
import pytest

import reach_cells as RC

SEED = 3
ROBOTS = ("kuka", "diana")
EDGE_FAMILIES = ("reach_dis", "precedence", "short_success", "zero", "never")      # cells placed a margin from reach_dis on purpose


@pytest.fixture(scope="module")
def chains(O, kuka, diana):
    return dict(kuka=kuka, diana=diana)


def _margin(precision):
    return RC.M64 if precision == 64 else RC.M32


def _table(O, chains, robot, precision, shift=(0.0, 0.0, 0.0)):
    return RC.build_cells(O, chains[robot], robot, m=_margin(precision), shift=shift, f32=precision == 32)


def _cases(cells):
    """(cell, auto_reset, steps) of every run a reach cell gets; the position in the list is the env's global id"""
    return [(x, ar, n) for x in cells if x.task == "reach" for ar in (False, True) for n in ((1, 2) if x.twostep else (1,))]


def _model(O, chains, robot, cases, defect=None):
    out = []
    for i, (x, ar, n) in enumerate(cases):
        cfg, c = RC.make_cfg(O, x.task, x.variant, robot), RC.constants(O, x.task, x.variant, robot)
        out.append(RC.model_run(O, chains[robot], cfg, c, x, env_id=i, seed=SEED, auto_reset=ar, nsteps=n, defect=defect))
    return out


@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_arm_poses_are_well_conditioned(O, chains, robot, f32):
    n = 0
    for (task, variant), d in RC.arms(O, chains[robot], robot, f32).items():
        cfg = RC.make_cfg(O, task, variant, robot)
        for nm, a in d.items():
            assert a["iters"] < cfg.ik_max_iters, (task, variant, nm, a["iters"])
            assert a["pose_pivot"] >= cfg.fence_pivot and a["minpiv"] >= cfg.fence_pivot, (task, variant, nm, a["pose_pivot"], a["minpiv"])
            assert a["gate"] >= RC.GATE_BAND, (task, variant, nm, a["gate"])
            box_lo, box_hi = np.array(cfg.box_lo[:]), np.array(cfg.box_hi[:])
            assert (a["p0"] >= box_lo - 1e-4).all() and (a["p0"] <= box_hi + 1e-4).all(), (task, variant, nm, a["p0"])      # inside the workspace (sb_on: on a face)
            n += 1
    assert n >= (20 if robot == "diana" else 70), n


def test_small_box_is_as_the_table_records_it(O, kuka):
    """every bound 2 to 4 cm from FK(q_init), no two equal, |lo| != |hi| on every axis"""
    p = O.fk(kuka, O.default_config().q_init[:])[0][0]
    lo, hi = np.array(RC.SMALLBOX["box_lo"]), np.array(RC.SMALLBOX["box_hi"])
    off = np.concatenate([p - lo, hi - p])
    assert (off >= 0.02).all() and (off <= 0.04).all(), off
    assert len(set(np.concatenate([lo, hi]).tolist())) == 6 and len(set(np.round(off, 9).tolist())) == 6
    assert (np.abs(lo) != np.abs(hi)).all()


@pytest.mark.parametrize("precision", [64, 32])
def test_table_size_and_names(O, chains, precision):
    cells = _table(O, chains, "kuka", precision)
    names = [(x.task, x.variant, x.name) for x in cells]
    assert len(set(names)) == len(names) and 100 <= len(cells) <= 200, len(cells)
    assert {(x.task, x.variant) for x in cells} == {(t, v) for t in RC.VARIANTS for v in RC.VARIANTS[t]}
    assert sum(x.zero_action for x in cells if x.task == "reach") >= 15
    assert all(x.ep_return != 0.0 and x.episode >= 2 and np.float32(x.ep_return) == x.ep_return for x in cells)
    d = _table(O, chains, "diana", precision)
    assert {(x.task, x.variant) for x in d} == {("reach", v) for v in RC.OUTCOME_VARIANTS}
    assert [x.name for x in d] == [x.name for x in cells if x.task == "reach" and x.variant in RC.OUTCOME_VARIANTS and not x.branch.startswith("clip")]


@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("precision", [64, 32])
def test_each_cell_lands_in_its_branch(O, chains, robot, precision):
    m = _margin(precision)
    cells = _table(O, chains, robot, precision)
    seen = {}
    for x in cells:
        cfg, c = RC.make_cfg(O, x.task, x.variant, robot), RC.constants(O, x.task, x.variant, robot)
        st = dict(q=x.q, goal=x.goal, step=x.step, episode=x.episode, ep_return=x.ep_return)
        r = RC.model_step(O, chains[robot], cfg, c, x.task, st, x.action)
        tr, e = r["trace"], x.expect
        for k, v in x.want.items():
            assert k in tr and tr[k] == v, (x, k, v, tr)
        for k, v in tr.items():
            seen.setdefault(k, set()).add(v)
        # the clip: every bound is 5 mm or more from the unclipped target, but for the cell that sits on a face
        start = r["p0"].astype(np.float32).astype(np.float64) if x.task == "pick" else r["p0"]
        v = start + x.action.astype(np.float64) * c["dv"]
        gap = np.minimum(np.abs(v - c["box_lo"]), np.abs(v - c["box_hi"]))
        if "on" in e:
            k, bound = e["on"]
            assert abs(v[k] - bound) <= 2e-4 and abs(r["tgt"][k] - v[k]) <= 2e-4 and np.delete(gap, k).min() >= 5e-3, (x, v)
            assert tr["lo%d" % k] == (v[k] < bound)      # the trace says which side the pose took
        else:
            assert gap.min() >= 5e-3, (x, v, gap)
        if "faces" in e:      # a clipped axis ends on its face to within the IK's residual, and 0.35 dv from where no clip would send it
            for k, bound in e["faces"]:
                assert r["tgt"][k] == bound and abs(r["eef"][k] - bound) <= 2e-4, (x, k, r["tgt"], r["eef"])
                assert abs(v[k] - bound) >= 5e-3, (x, v[k], bound)
            assert sum(tr[s] for s in tr if s[:2] in ("lo", "hi")) == len(e["faces"]), (x, tr)
        if "unclipped" in e:
            assert np.array_equal(r["tgt"], v), (x, r["tgt"], v)
        if x.task != "reach":
            continue
        # the outcome: placed cells a margin from reach_dis (the f32 goal moves them by less than 1e-7), every other one 5 margins or more
        dist, rd = r["dist"], c["reach_dis"]
        if x.name == "reach_dis/zero":
            assert dist <= 6e-8 and e["nearest"] == (dist != 0.0), (x, dist)
        elif x.branch.startswith(EDGE_FAMILIES) and x.name not in ("zero/far", "never/far"):
            assert abs(abs(dist - rd) - m) <= 1e-7, (x, dist)
        else:
            assert abs(dist - rd) >= 5 * m, (x, dist)
        for k in ("done", "success"):
            if k in e:
                assert r[k] == e[k], (x, k)
        if "reward" in e:
            assert abs(r["reward"] - e["reward"]) <= 1e-6 and (e["reward"] != 0.0 or r["reward"] == 0.0), (x, r["reward"], e["reward"])
        if "last_len" in e:
            assert r["ended"][1] == e["last_len"], (x, r["ended"])
    # every decision of the model is taken both ways somewhere in the table
    want = {"timeout", "near", "reset"} | ({"%s%d" % (s, k) for s in ("lo", "hi") for k in range(3)} if robot == "kuka" else set())
    for k in want - {"reset"}:
        assert seen.get(k) == {True, False}, (k, seen.get(k))
    # ... and the in-place reset happens exactly under auto-reset on a finished episode
    cases = _cases(cells)
    for (x, ar, n), r in zip(cases, _model(O, chains, robot, cases)):
        for tr in r["traces"]:
            assert tr["reset"] == (ar and (tr["timeout"] or tr["near"])), (x, ar, tr)


@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("precision", [64, 32])
def test_no_cell_is_ambiguous(O, chains, robot, precision):
    """Placing the cells from a p1 that is off by the engine's allowed disagreement, along either direction of each axis, changes no
    cell's decisions: the model's trace of every step, done, success, the step and episode counters.  No cell is exempt."""
    base = _table(O, chains, robot, precision)
    cases = _cases(base)
    ref = _model(O, chains, robot, cases)
    d = RC.PERTURB[precision]
    bad = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            shift = [0.0, 0.0, 0.0]; shift[ax] = sgn * d
            moved = _table(O, chains, robot, precision, shift=shift)
            assert [x.name for x in moved] == [x.name for x in base]
            mc = _cases(moved)
            for (x, ar, n), g, r in zip(mc, _model(O, chains, robot, mc), ref):
                if not (g["traces"] == r["traces"] and all(g[k] == r[k] for k in ("done", "success", "step", "episode", "n_done", "n_success"))):
                    bad.append((x, ar, n, ax, sgn))
    assert not bad, bad


@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("precision", [64, 32])
def test_model_agrees_with_the_oracle(O, chains, robot, precision):
    """flags, counters and goals equal, everything else to 1e-12, on every reach cell with and without auto-reset (two-step cells over
    both steps); for push and pick the arm (q and the flange) on the clip cells"""
    cells = _table(O, chains, robot, precision)
    tight = dict(pos=1e-12, reward=1e-12, nsteps=1)
    n_rows = 0
    for (task, variant), cs in RC.groups(cells).items():
        cfg, c = RC.make_cfg(O, task, variant, robot), RC.constants(O, task, variant, robot)
        if task != "reach":
            rows = RC.rows_of(cs, range(len(cs)))
            for ar in (False, True):
                r = RC.run_oracle(O, chains[robot], task, cfg, rows, auto_reset=ar, seed=SEED)
                for i, x in enumerate(cs):
                    g = RC.model_step(O, chains[robot], cfg, c, task, dict(q=x.q, step=x.step), x.action)
                    assert not r["done"][i] and np.abs(r["q"][i] - g["q"]).max() <= 1e-12 and r["step"][i] == g["step"], (x, ar)
                    assert np.array_equal(r["obs"][i, :3], g["eef"].astype(np.float32)), (x, ar)
                    n_rows += 1
            continue
        for ar in (False, True):
            for nsteps in (1, 2):
                idx = [i for i, x in enumerate(cs) if nsteps == 1 or x.twostep]
                if not idx:
                    continue
                r = RC.run_oracle(O, chains[robot], task, cfg, RC.rows_of(cs, idx), auto_reset=ar, seed=SEED, nsteps=nsteps)
                g = RC.stack([RC.model_run(O, chains[robot], cfg, c, cs[i], env_id=row, seed=SEED, auto_reset=ar, nsteps=nsteps) for row, i in enumerate(idx)])
                r["eef"] = g["eef"]
                bad = RC.compare(g, r, tight, ulp=False)
                assert not bad, (variant, ar, nsteps, [(cs[idx[i]], what, dev) for i, what, dev in bad[:8]])
                n_rows += len(idx)
    assert n_rows >= (100 if robot == "kuka" else 60), n_rows


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("defect", RC.DEFECTS)
def test_planted_defect_is_caught(O, chains, record_property, defect, precision):
    """the model with one defect planted differs from the model in a checked output of at least one cell by more than the GPU test's
    tolerance for it (or in an exact one): a kernel with that defect would fail tests/test_gpu_reach_cells.py at the cells named"""
    cells = _table(O, chains, "kuka", precision)
    cases = _cases(cells)
    ref, got = _model(O, chains, "kuka", cases), _model(O, chains, "kuka", cases, defect)
    caught = {}
    for (x, ar, n), g, r in zip(cases, got, ref):
        tol = RC.tolerances(precision, n) if defect not in RC.CPU_ONLY_DEFECTS else dict(pos=1e-12, reward=1e-12, nsteps=n)
        bad = RC.compare(RC.stack([g]), RC.stack([r]), tol, ulp=defect not in RC.CPU_ONLY_DEFECTS)
        if bad:
            caught.setdefault("%s/%s%s" % (x.variant, x.name, " (auto-reset)" if ar else ""), set()).update(what for _, what, _ in bad)
    if defect.startswith(("no_", "clip_")):      # the clip is the arm's: push and pick show it in q and the flange
        for x in cells:
            if x.task == "reach":
                continue
            cfg, c = RC.make_cfg(O, x.task, x.variant), RC.constants(O, x.task, x.variant)
            st = dict(q=x.q, step=x.step)
            g, r = (RC.model_step(O, chains["kuka"], cfg, c, x.task, st, x.action, defect=d) for d in (defect, None))
            if max(np.abs(g["q"] - r["q"]).max(), np.abs(g["eef"] - r["eef"]).max()) > RC.PERTURB[precision]:
                caught.setdefault("%s %s/%s" % (x.task, x.variant, x.name), set()).add("q")
        for task in RC.VARIANTS:
            assert any(k.startswith(task + " ") or (task == "reach" and not k.startswith(("push ", "pick "))) for k in caught), (defect, task, sorted(caught))
    print("defect %s is caught by %d cells: %s" % (defect, len(caught), "; ".join("%s [%s]" % (k, ", ".join(sorted(v))) for k, v in sorted(caught.items()))))
    record_property("caught_by", sorted(caught))
    assert caught, defect
    if defect in RC.CPU_ONLY_DEFECTS:      # ... and this one by the 1e-12 CPU check only: below the GPU tolerances by construction (reach_cells docstring)
        worst = {}
        for g, r, (x, ar, n) in zip(got, ref, cases):
            assert not RC.compare(RC.stack([g]), RC.stack([r]), RC.tolerances(precision, n), worst=worst), x
        assert worst["reward"] <= 10 * 3 * 2.0 ** -25, worst


def test_constants_are_pinned(O):
    """every constant the table restates is the oracle's default (which tests/test_oracle_golden.py and the parity tests hold to the engine's)"""
    for task in RC.VARIANTS:
        cfg = O.default_config(task)
        assert cfg.reach_dis == RC.CONST["reach_dis"] and cfg.max_steps == RC.CONST["max_steps"] and cfg.dv == RC.CONST["dv"][task]
        assert tuple(cfg.box_lo[:]) == RC.CONST["box_lo"] and tuple(cfg.box_hi[:]) == RC.CONST["box_hi"][task]
        assert tuple(cfg.goal_lo[:]) == RC.CONST["goal_lo"] and tuple(cfg.goal_hi[:]) == RC.CONST["goal_hi"]
        c = RC.constants(O, task, "default")
        for k in ("reach_dis", "max_steps", "dv"):
            assert c[k] == getattr(cfg, k)
        for k in ("box_lo", "box_hi", "goal_lo", "goal_hi", "q_init"):
            assert c[k] == tuple(getattr(cfg, k)[:]), k
    assert (RC.M64, RC.M32) == (1e-5, 1e-3) and RC.PERTURB == {64: 1e-6, 32: 1e-4}
