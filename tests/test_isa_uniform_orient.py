"""The reach rollout kernels with the wave-uniform orientation dispatch in their peeled IK trips (armenv_kin.h
ARMENV_UNIFORM_ORIENT) still meet the structural guards of test_isa_guard.py: no scratch traffic, and one action-prefetch triple whose
three AGPRs nothing touches between issue and settle -- the out-of-line select forms lie inside that window.  No GPU, nothing is
recompiled: the guards are re-run on the built library for exactly these kernels."""
import re

import pytest

import test_isa_guard as G

kernels = G.kernels        # the module-scoped fixture: every kernel of the built libarmenv.so


def _reach_p0(kernels):
    sel = [(sn, md, ins) for sn, _, md, ins in kernels if re.search(r"^reach_rollout_f(64|32)_[a-z]+_p0$", sn)]
    assert len(sel) == 6
    return sel


def test_reach_rollouts_have_no_scratch(kernels):
    for sn, md, ins in _reach_p0(kernels):
        # the guard as test_isa_guard.py states it: no scratch TRAFFIC; a reserved scavenger slot that no instruction touches is tolerated
        assert not [i.text for i in ins if i.mnem.startswith(("scratch_", "buffer_"))], sn
        assert md["scratch"] <= 128 and md["lds"] == 0, (sn, md)


def test_reach_rollouts_have_one_prefetch_triple_left_alone(kernels):
    for sn, md, ins in _reach_p0(kernels):
        triples = G._prefetch_triples(ins)
        assert len(triples) == 1, (sn, triples)
        k0, regs = triples[0]
        settles = [k for k in range(1, len(ins) - 2)
                   if all(ins[k + j].mnem == "v_accvgpr_read_b32" and ins[k + j].ops.split(", ")[1] == regs[j] for j in range(3))
                   and ins[k - 1].mnem == "s_waitcnt" and "vmcnt(0)" in ins[k - 1].ops]
        assert len(settles) == 1, (sn, settles)
        window = G._reachable_before(ins, k0 + 3, settles[0] - 1)
        pat = re.compile(r"\b(%s)\b" % "|".join(regs))
        assert not [ins[k].text for k in sorted(window) if pat.search(ins[k].ops)], sn


def test_headline_register_budget(kernels):
    by = {sn: md for sn, _, md, _ in kernels}
    md = by["reach_rollout_f64_kuka_p0"]
    assert md["vgpr"] <= 512 and md["scratch"] == 0 and md["lds"] == 0, md
    assert by["reach_rollout_f64_kuka_p0_w2"]["vgpr"] <= 256 and by["reach_rollout_f64_kuka_p0_w2"]["agpr"] == 0
