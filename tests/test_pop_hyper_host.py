"""CPU tests of the host side of the per-member hyper-parameters of the population updates (armenv_td3_pop_update_hyper,
armenv_daddpg_pop_update_hyper, armenv_datd3_pop_update_hyper and ArmEnvPopHyper, include/armenv.h): the ctypes struct agrees with the
header, every argument -- each member's values among them -- is validated before any HIP call, the population classes take a scalar or
P values of every sweepable name and pick the entry point accordingly, and the six *_pop_hyper_kernel forms are in the built code
object.  No test here passes a valid set of arguments to an entry point: that would enqueue kernels on made-up pointers."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import isa  # noqa: E402

HEADER_DIR = os.path.join(ROOT, "include")
FIELDS = ("gamma", "tau", "policy_noise", "noise_clip", "actor_lr", "critic_lr", "q_weight", "regularization_weight")
UNIT = ("gamma", "tau", "q_weight")                       # in [0, 1]; the others >= 0
TD3_NETS = ("actor", "q1", "q2", "target_actor", "target_q1", "target_q2", "actor_m", "actor_v", "q1_m", "q1_v", "q2_m", "q2_v")
DADDPG_NETS = ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic",
               "actor1_m", "actor1_v", "actor2_m", "actor2_v", "critic_m", "critic_v")
DATD3_NETS = ("actor1", "actor2", "critic1", "critic2", "target_actor1", "target_actor2", "target_critic1", "target_critic2",
              "actor1_m", "actor1_v", "actor2_m", "actor2_v", "critic1_m", "critic1_v", "critic2_m", "critic2_v")
# kind -> (the C entry points' stem, `darc`, the fields of hyper[p] that the agent reads)
KINDS = dict(td3=("td3", 0, FIELDS[:6]), daddpg=("daddpg", 0, ("gamma", "tau", "actor_lr", "critic_lr")), datd3=("datd3", 0, FIELDS[:6]),
             darc=("datd3", 1, FIELDS))
HYPER_KERNELS = ("adam", "critic_head", "daddpg_critic_head", "datd3_critic_head", "actor_head", "datd3_actor_head")


def test_struct_layout_matches_the_header_and_the_abi_version_did_not_move():
    from armenv import _lib as L
    H = L.ArmEnvPopHyper
    assert tuple(n for n, _ in H._fields_) == FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "armenv.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(ArmEnvPopHyper));']
    lines += ['  printf("%%zu\\n", offsetof(ArmEnvPopHyper, %s));' % n for n in FIELDS]
    # the declarations take what the ctypes prototypes say they take (checked by the compiler; nothing is linked)
    lines += ["  _Static_assert(__builtin_types_compatible_p(__typeof__(&armenv_%s_pop_update_hyper), "
              "int (*)(const %s *, const ArmEnvPopHyper *, void *)), \"%s\");" % (n, s, n)
              for n, s in (("td3", "ArmEnvTd3PopArgs"), ("daddpg", "ArmEnvDaddpgPopArgs"), ("datd3", "ArmEnvDatd3PopArgs"))]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", HEADER_DIR, "-o", exe, src], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert out[0] == C.sizeof(H) == 32
    assert out[1:] == [getattr(H, n).offset for n in FIELDS]
    lib = L.load()
    assert lib.armenv_abi_version() == 8 and L.ABI_VERSION == 8
    for stem, pop in (("td3", L.ArmEnvTd3PopArgs), ("daddpg", L.ArmEnvDaddpgPopArgs), ("datd3", L.ArmEnvDatd3PopArgs)):
        res, args = L.SYMBOLS["armenv_%s_pop_update_hyper" % stem]
        assert res is C.c_int and args == [C.POINTER(pop), C.POINTER(H), C.c_void_p]


def _args(kind, P=3, B=64, D=6):
    """(arguments, hyper) that pass every check but the one a test breaks: made-up (never dereferenced) 16-byte aligned device
    pointers, every hyper[p] equal to `one`'s fields.  NOT to be passed unmodified -- a valid set would be enqueued."""
    from armenv import _lib as L
    stem, darc, _ = KINDS[kind]
    Pop, nets = dict(td3=(L.ArmEnvTd3PopArgs, TD3_NETS), daddpg=(L.ArmEnvDaddpgPopArgs, DADDPG_NETS), datd3=(L.ArmEnvDatd3PopArgs, DATD3_NETS))[stem]
    pa = Pop()
    pa.members = P
    a = pa.one
    a.device, a.state_dim, a.action_dim, a.hidden_dim, a.batch = 0, D, 3, 256, B
    a.action_bound, a.gamma, a.tau = 0.7, 0.98, 0.005
    a.actor_lr, a.critic_lr, a.beta1, a.beta2, a.eps = 1e-3, 1e-3, 0.9, 0.999, 1e-8
    a.critic_step, a.actor_step = 1, 1
    if stem == "td3":
        a.with_actor = 1
    else:
        a.update_actor = 1
    if stem != "daddpg":
        a.policy_noise, a.noise_clip = 0.2, 0.5
    if stem == "datd3":
        a.darc, a.q_weight, a.regularization_weight = darc, 0.2, 0.005
    addr = [0x10000000]

    def ptr():
        addr[0] += 0x1000000
        return addr[0]
    for net in nets:
        for k in ("W1", "b1", "W2", "b2", "W3", "b3"):
            setattr(getattr(a, net), k, ptr())
    for k in ("states_dev", "actions_dev", "next_states_dev", "rewards_dev", "dones_dev", "workspace_dev"):
        setattr(a, k, ptr())
    a.workspace_bytes = getattr(L.load(), "armenv_%s_pop_workspace_bytes" % stem)(D, 256, B, P)
    assert a.workspace_bytes > 0
    hyper = (L.ArmEnvPopHyper * P)()
    for h in hyper:
        for n in FIELDS:
            setattr(h, n, getattr(a, n, 0.0))
    return pa, hyper


def _refused(kind, pa, hyper):
    from armenv import _lib as L
    lib = L.load()
    fn = "armenv_%s_pop_update_hyper" % KINDS[kind][0]
    rc = getattr(lib, fn)(C.byref(pa) if pa is not None else None, hyper, None)
    msg = lib.armenv_last_error().decode()
    assert rc == -1, (rc, msg)                       # ARMENV_EINVAL, not ENODEV: nothing touched the device
    assert msg.startswith(fn), msg
    return msg


@pytest.mark.parametrize("kind", list(KINDS))
def test_null_arguments_and_member_counts_are_refused(kind):
    pa, hyper = _args(kind)
    assert "hyper is NULL" in _refused(kind, pa, None)
    assert "args" in _refused(kind, None, hyper)
    for members in (0, 65, -1):
        pa.members = members
        assert "members" in _refused(kind, pa, hyper)


@pytest.mark.parametrize("kind", list(KINDS))
def test_whatever_the_population_update_refuses_is_refused(kind):
    from armenv import _lib as L
    stem = KINDS[kind][0]
    for field, mutate in (("gamma", lambda a: setattr(a, "gamma", float("nan"))), ("batch", lambda a: setattr(a, "batch", 0)),
                          ("hidden_dim", lambda a: setattr(a, "hidden_dim", 128)), ("states_dev", lambda a: setattr(a, "states_dev", None)),
                          ("critic_step", lambda a: setattr(a, "critic_step", 0)),
                          ("workspace_bytes", lambda a: setattr(a, "workspace_bytes", a.workspace_bytes - 1))):
        pa, hyper = _args(kind)
        mutate(pa.one)
        assert field in _refused(kind, pa, hyper), field
    pa, hyper = _args(kind, P=2)
    pa.one.workspace_bytes = getattr(L.load(), "armenv_%s_workspace_bytes" % stem)(6, 256, 64)      # one member's, for two
    msg = _refused(kind, pa, hyper)
    assert "workspace_bytes" in msg and "armenv_%s_pop_workspace_bytes" % stem in msg, msg


@pytest.mark.parametrize("kind", list(KINDS))
def test_each_members_values_are_checked_and_named(kind):
    """Every field the agent reads, out of range on either side and NaN, in the first and in the last member: refused, the message
    naming hyper[p].field."""
    P = 3
    for field in KINDS[kind][2]:
        for bad in (-0.25, float("nan"), float("inf")) + ((1.5,) if field in UNIT else ()):
            for p in (0, P - 1):
                pa, hyper = _args(kind, P=P)
                setattr(hyper[p], field, bad)
                msg = _refused(kind, pa, hyper)
                assert "hyper[%d].%s" % (p, field) in msg, (field, bad, p, msg)


@pytest.mark.parametrize("kind", list(KINDS))
def test_fields_the_agent_does_not_read_are_ignored(kind):
    """Member 0 holds -1 in every field its agent does not read and the LAST member an out-of-range gamma: the call is refused for
    the last member's gamma -- the checks run member by member, so member 0's unread fields were passed over.  (Nothing but a
    refusal can be observed here without a device.)"""
    P = 3
    unread = [f for f in FIELDS if f not in KINDS[kind][2]]
    assert len(unread) == dict(td3=2, daddpg=4, datd3=2, darc=0)[kind]
    pa, hyper = _args(kind, P=P)
    for f in unread:
        setattr(hyper[0], f, -1.0)
    hyper[P - 1].gamma = 2.0
    assert "hyper[%d].gamma" % (P - 1) in _refused(kind, pa, hyper)


def _classes(kind):
    from armenv.fused_daddpg import FusedDADDPG
    from armenv.fused_daddpg_pop import FusedDADDPGPopulation
    from armenv.fused_datd3 import FusedDARC, FusedDATD3
    from armenv.fused_datd3_pop import FusedDARCPopulation, FusedDATD3Population
    from armenv.fused_td3 import FusedTD3
    from armenv.fused_td3_pop import FusedTD3Population
    return dict(td3=(FusedTD3Population, FusedTD3), daddpg=(FusedDADDPGPopulation, FusedDADDPG), datd3=(FusedDATD3Population, FusedDATD3),
                darc=(FusedDARCPopulation, FusedDARC))[kind]


@pytest.mark.parametrize("kind", list(KINDS))
def test_scalars_keep_the_shared_entry_point_and_sequences_take_the_member_one(kind):
    Pop, _ = _classes(kind)
    stem, _, read = KINDS[kind]
    assert Pop.sweepable() == tuple(n for n in ("actor_lr", "critic_lr", "tau", "gamma", "policy_noise", "noise_clip", "q_weight",
                                                "regularization_weight") if n in read)
    pop = Pop(3, 6, 3, 0.7, device="cpu", actor_lr=5e-4)
    assert pop.uniform() and pop.entry_point == "armenv_%s_pop_update" % stem
    assert pop.actor_lr == 5e-4 and pop.gamma == 0.98 and isinstance(pop.tau, float)       # the scalars they always were
    assert pop.hyper(2)["actor_lr"] == 5e-4 and set(pop.hyper(0)) == set(Pop.sweepable())
    for name in Pop.sweepable():
        values = [0.25, 0.5, 0.75]
        swept = Pop(3, 6, 3, 0.7, device="cpu", **{name: values})
        assert not swept.uniform() and swept.entry_point == "armenv_%s_pop_update_hyper" % stem, name
        assert getattr(swept, name) == tuple(values) and [swept.hyper(p)[name] for p in range(3)] == values
        assert swept._hp(name) == 0.25                      # `one` carries member 0's
    same = Pop(3, 6, 3, 0.7, device="cpu", tau=[0.01, 0.01, 0.01])                # P equal values: still the shared entry point
    assert same.uniform() and same.tau == 0.01 and same.entry_point == "armenv_%s_pop_update" % stem
    same.always_hyper = True
    assert same.entry_point == "armenv_%s_pop_update_hyper" % stem


@pytest.mark.parametrize("kind", list(KINDS))
def test_wrong_lengths_unsweepable_names_and_values_out_of_range_raise(kind):
    Pop, _ = _classes(kind)
    for kw in (dict(actor_lr=[1e-3, 1e-3]), dict(gamma=[0.9] * 4), dict(tau=[]), dict(hidden_dim=[256] * 3),
               dict(gamma=[0.9, 0.9, 1.5]), dict(critic_lr=[1e-3, -1e-3, 1e-3]), dict(tau=[0.0, float("nan"), 0.0])):
        with pytest.raises(ValueError):
            Pop(3, 6, 3, 0.7, device="cpu", **kw)
    if kind != "daddpg":                                    # DADDPG has no policy_freq, and no noise to sweep
        with pytest.raises(ValueError):
            Pop(3, 6, 3, 0.7, device="cpu", policy_freq=[3, 3, 3])
    else:
        with pytest.raises(TypeError):
            Pop(3, 6, 3, 0.7, device="cpu", policy_noise=[0.1, 0.2, 0.3])
    if kind == "datd3":                                     # DARC's two are not DATD3's
        with pytest.raises(ValueError):
            Pop(3, 6, 3, 0.7, device="cpu", q_weight=[0.1, 0.2, 0.3])


@pytest.mark.parametrize("kind", list(KINDS))
def test_hyper_and_set_hyper_round_trip(kind):
    Pop, _ = _classes(kind)
    stem = KINDS[kind][0]
    pop = Pop(3, 6, 3, 0.7, device="cpu")
    before = pop.hyper(1)
    pop.set_hyper(1, gamma=0.5, critic_lr=0.0)
    assert pop.hyper(1) == dict(before, gamma=0.5, critic_lr=0.0) and pop.hyper(0) == before == pop.hyper(2)
    assert pop.gamma == (0.98, 0.5, 0.98) and pop.critic_lr == (1e-3, 0.0, 1e-3) and pop.tau == 0.005
    assert pop.entry_point == "armenv_%s_pop_update_hyper" % stem and pop._args is None      # bound anew at the next train
    got = pop.hyper(1)
    got["gamma"] = 0.0                                      # a copy: writing to it changes nothing
    assert pop.hyper(1)["gamma"] == 0.5
    for bad in (dict(policy_freq=2), dict(hidden_dim=256), dict(expl_sigma=0.1), dict(gamma=1.5), dict(actor_lr=-1.0), dict(tau=float("nan"))):
        with pytest.raises(ValueError):
            pop.set_hyper(0, **bad)
        assert pop.hyper(0) == before
    pop.set_hyper(1, **before)
    assert pop.uniform() and pop.gamma == 0.98 and pop.entry_point == "armenv_%s_pop_update" % stem


@pytest.mark.parametrize("kind", list(KINDS))
def test_export_member_carries_the_members_values_and_load_member_leaves_them(kind):
    Pop, Single = _classes(kind)
    values = dict(actor_lr=[1e-3, 2e-3, 0.0], gamma=[0.9, 0.95, 1.0], tau=[0.0, 0.01, 1.0])
    pop = Pop(3, 6, 3, 0.7, device="cpu", seed=5, **values)
    for p in range(3):
        single = pop.export_member(p)
        assert type(single) is Single
        assert (single.actor_lr, single.gamma, single.tau, single.critic_lr) == (values["actor_lr"][p], values["gamma"][p], values["tau"][p], 1e-3)
        assert all(torch.equal(x, y) for x, y in zip(pop._member_state(p), pop._single_state(single)))
        if kind != "daddpg":
            assert single.seed == 5 + p and single.policy_noise == 0.2
    other = Single(6, 3, 0.7, device="cpu", gamma=0.5)
    pop.load_member(2, other)
    assert pop.hyper(2)["gamma"] == 1.0 and all(torch.equal(x, y) for x, y in zip(pop._member_state(2), pop._single_state(other)))


@pytest.mark.parametrize("kind", list(KINDS))
def test_copy_member_with_and_without_the_hyper_parameters(kind):
    Pop, _ = _classes(kind)
    pop = Pop(3, 6, 3, 0.7, device="cpu", critic_lr=[1e-3, 2e-3, 3e-3])
    with torch.no_grad():
        for name in pop.stacks:                             # moments too: distinct per member
            for t in pop.stacks[name]:
                t.add_(torch.arange(3.0).reshape(3, *[1] * (t.dim() - 1)))
    state = lambda p: [t.clone() for t in pop._member_state(p)]
    m0, m1, m2 = state(0), state(1), state(2)
    assert not any(torch.equal(x, y) for x, y in zip(m0, m2))
    pop.copy_member(0, 2)
    assert all(torch.equal(x, y) for x, y in zip(state(2), m0)) and all(torch.equal(x, y) for x, y in zip(state(0), m0))
    assert all(torch.equal(x, y) for x, y in zip(state(1), m1))
    assert [pop.hyper(p)["critic_lr"] for p in range(3)] == [1e-3, 2e-3, 3e-3]
    pop.copy_member(1, 0, hyper=True)
    assert all(torch.equal(x, y) for x, y in zip(state(0), m1))
    assert [pop.hyper(p)["critic_lr"] for p in range(3)] == [2e-3, 2e-3, 3e-3] and pop.critic_lr == (2e-3, 2e-3, 3e-3)
    assert pop.member(0).actor.fc1.weight.data_ptr() == pop.stacks[pop._NETS[0]][0][0].data_ptr()       # still views into the stacks
    with pytest.raises(IndexError):
        pop.copy_member(0, 3)


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_refused_call_leaves_every_counter_at_zero(kind):
    """A population with members' own values: a batch of 0 rows and (where the agent takes it) a `noise` of the wrong shape raise from
    `train` before total_it or a step number moves, and a member's value out of range is refused where it is given -- by the
    constructor and by set_hyper -- so no `train` is refused for it after its counters moved.  No device is touched."""
    Pop, _ = _classes(kind)
    pop = Pop(2, 6, 3, 0.7, device="cpu", gamma=[0.9, 0.99])
    assert pop.entry_point.endswith("_hyper")

    def batch(B):
        return dict(states=torch.zeros(2, B, 6), actions=torch.zeros(2, B, 3), next_states=torch.zeros(2, B, 6),
                    rewards=torch.zeros(2, B), dones=torch.zeros(2, B, dtype=torch.uint8))

    def counters():
        return {k: v for k, v in vars(pop).items() if k == "total_it" or k.endswith("_step")}
    assert set(counters()) == set(pop._COUNTERS)
    with pytest.raises(ValueError):
        pop.train(batch(0))
    assert all(v == 0 for v in counters().values()), counters()
    if kind != "daddpg":
        bad = torch.zeros(2, 5, 3)
        with pytest.raises(ValueError):
            pop.train(batch(4), noise=bad if kind == "td3" else (bad, bad))
        assert all(v == 0 for v in counters().values()), counters()
    with pytest.raises(ValueError):
        pop.set_hyper(1, gamma=1.5)
    assert pop.hyper(1)["gamma"] == 0.99 and all(v == 0 for v in counters().values())


def test_train_pop_refuses_an_unknown_sweep_name_and_a_wrong_count():
    from armenv.train_pop import sweepable_names, train_reach_population
    assert sweepable_names("td3") == ("actor_lr", "critic_lr", "tau", "gamma", "policy_noise", "noise_clip", "expl_sigma")
    assert sweepable_names("daddpg") == ("actor_lr", "critic_lr", "tau", "gamma", "expl_sigma")
    assert sweepable_names("darc")[-3:] == ("q_weight", "regularization_weight", "expl_sigma")
    for algo, sweep in (("td3", dict(learning_rate=[1e-3, 1e-3])), ("td3", dict(policy_freq=[2, 3])), ("td3", dict(actor_lr=[1e-3])),
                        ("td3", dict(expl_sigma=[0.1, 0.2, 0.3])), ("daddpg", dict(policy_noise=[0.1, 0.2])),
                        ("datd3", dict(q_weight=[0.1, 0.2]))):
        with pytest.raises(ValueError):
            train_reach_population(members=2, iterations=0, algo=algo, sweep=sweep)


def test_the_command_line_refuses_a_bad_sweep():
    cmd = [sys.executable, "-m", "armenv.train_pop", "--members", "2", "--iterations", "0"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "drl-on-robot-arm_amd")] + sys.path))
    for sweep in ("actor_lr=1e-3", "lr=1e-3,1e-3"):
        r = subprocess.run(cmd + ["--sweep", sweep], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "sweep" in r.stderr, (sweep, r.returncode, r.stderr[-300:])


@pytest.fixture(scope="module")
def learner_kernels():
    if not os.path.exists(isa.LIB):
        pytest.skip("libarmenv.so is not built")
    if not os.path.exists(os.path.join(isa.LLVM, "llvm-objdump")):
        pytest.skip("the ROCm LLVM tools (llvm-objdump, llvm-readelf) are not installed")
    rows = [r for r in isa.all_kernels() if "armenv::learner::" in r[1]]
    return {dm.split("armenv::learner::")[1].split("(")[0]: (md, ins) for _, dm, md, ins in rows}


def test_member_hyper_kernels_are_in_the_code_object(learner_kernels):
    """test_td3_fused_host.py holds every armenv::learner:: kernel, these included, to no scratch, no atomics and exact f32; here:
    exactly the six kernels that read a member's scalar have a *_pop_hyper_kernel form, beside their *_pop_kernel form, with no
    scratch, and the heads use no LDS."""
    hyper = {k for k in learner_kernels if k.endswith("_pop_hyper_kernel")}
    assert hyper == {k + "_pop_hyper_kernel" for k in HYPER_KERNELS}, sorted(learner_kernels)
    for k in HYPER_KERNELS:
        assert k + "_pop_kernel" in learner_kernels and k + "_kernel" in learner_kernels
        md, ins = learner_kernels[k + "_pop_hyper_kernel"]
        assert md["scratch"] == 0 and len(ins) > 0, (k, md)
        assert md["lds"] == (learner_kernels["adam_pop_kernel"][0]["lds"] if k == "adam" else 0), (k, md)
