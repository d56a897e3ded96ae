"""CPU tests of the host side of the per-member hyper-parameters of the population updates (armenv_td3_pop_update_hyper,
armenv_daddpg_pop_update_hyper, armenv_datd3_pop_update_hyper and ArmEnvPopHyper, include/armenv.h): the ctypes struct agrees with the
header, every argument -- each member's values among them -- is validated before any HIP call, the population classes take a scalar or
P values of every sweepable name and pick the entry point accordingly, and the six *_pop_hyper_kernel forms are in the built code
object.  No test here passes a valid set of arguments to an entry point: that would enqueue kernels on made-up pointers."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from learner_host import classes, ctypes_layout, fake_pop_args, header_layout, learner_kernels, refused  # noqa: F401

FIELDS = ("gamma", "tau", "policy_noise", "noise_clip", "actor_lr", "critic_lr", "q_weight", "regularization_weight")
UNIT = ("gamma", "tau", "q_weight")                       # in [0, 1]; the others >= 0
# kind -> (the C entry points' stem, `darc`, the fields of hyper[p] that the agent reads)
KINDS = dict(td3=("td3", 0, FIELDS[:6]), daddpg=("daddpg", 0, ("gamma", "tau", "actor_lr", "critic_lr")), datd3=("datd3", 0, FIELDS[:6]),
             darc=("datd3", 1, FIELDS))
HYPER_KERNELS = ("adam", "critic_head", "daddpg_critic_head", "datd3_critic_head", "actor_head", "datd3_actor_head")


def test_struct_layout_matches_the_header_and_the_abi_version_did_not_move():
    from armenv import _lib as L
    H = L.ArmEnvPopHyper
    assert tuple(n for n, _ in H._fields_) == FIELDS
    # the declarations take what the ctypes prototypes say they take (checked by the compiler; nothing is linked)
    checks = ["_Static_assert(__builtin_types_compatible_p(__typeof__(&armenv_%s_pop_update_hyper), "
              "int (*)(const %s *, const ArmEnvPopHyper *, void *)), \"%s\");" % (n, s, n)
              for n, s in (("td3", "ArmEnvTd3PopArgs"), ("daddpg", "ArmEnvDaddpgPopArgs"), ("datd3", "ArmEnvDatd3PopArgs"))]
    sizes, offsets = header_layout(H, checks=checks, std="gnu11", werror=True)
    assert sizes == [C.sizeof(H)] == [32]
    assert [n for n, _ in ctypes_layout(H)] == list(FIELDS) and offsets == [getattr(H, n).offset for n in FIELDS]
    lib = L.load()
    assert lib.armenv_abi_version() == 9 and L.ABI_VERSION == 9
    for stem, pop in (("td3", L.ArmEnvTd3PopArgs), ("daddpg", L.ArmEnvDaddpgPopArgs), ("datd3", L.ArmEnvDatd3PopArgs)):
        res, args = L.SYMBOLS["armenv_%s_pop_update_hyper" % stem]
        assert res is C.c_int and args == [C.POINTER(pop), C.POINTER(H), C.c_void_p]


def _with_hyper(kind, P=3, B=64, D=6):
    """(fake_pop_args, hyper): every hyper[p] equal to `one`'s fields.  NOT to be passed unmodified -- a valid set would be enqueued."""
    from armenv import _lib as L
    pa = fake_pop_args(kind, P, B, D)
    hyper = (L.ArmEnvPopHyper * P)()
    for h in hyper:
        for n in FIELDS:
            setattr(h, n, getattr(pa.one, n, 0.0))
    return pa, hyper


def _refused(kind, pa, hyper):
    return refused("armenv_%s_pop_update_hyper" % KINDS[kind][0], C.byref(pa) if pa is not None else None, hyper, None)


@pytest.mark.parametrize("kind", list(KINDS))
def test_null_arguments_and_member_counts_are_refused(kind):
    pa, hyper = _with_hyper(kind)
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
        pa, hyper = _with_hyper(kind)
        mutate(pa.one)
        assert field in _refused(kind, pa, hyper), field
    pa, hyper = _with_hyper(kind, P=2)
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
                pa, hyper = _with_hyper(kind, P=P)
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
    pa, hyper = _with_hyper(kind, P=P)
    for f in unread:
        setattr(hyper[0], f, -1.0)
    hyper[P - 1].gamma = 2.0
    assert "hyper[%d].gamma" % (P - 1) in _refused(kind, pa, hyper)


@pytest.mark.parametrize("kind", list(KINDS))
def test_scalars_keep_the_shared_entry_point_and_sequences_take_the_member_one(kind):
    Pop, _, _ = classes(kind)
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
    Pop, _, _ = classes(kind)
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
    Pop, _, _ = classes(kind)
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
    Pop, Single, _ = classes(kind)
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
    Pop, _, _ = classes(kind)
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
    Pop, _, _ = classes(kind)
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


def test_member_hyper_kernels_are_in_the_code_object(learner_kernels):
    """test_td3_fused_host.py holds all of learner_host.learner_kernels, these included, to no scratch, no atomics and exact f32; here:
    exactly the six kernels that read a member's scalar have a *_pop_hyper_kernel form, beside their *_pop_kernel form, with no
    scratch, and the heads use no LDS."""
    hyper = {k for k in learner_kernels if k.endswith("_pop_hyper_kernel")}
    assert hyper == {k + "_pop_hyper_kernel" for k in HYPER_KERNELS}, sorted(learner_kernels)
    for k in HYPER_KERNELS:
        assert k + "_pop_kernel" in learner_kernels and k + "_kernel" in learner_kernels
        md, ins = learner_kernels[k + "_pop_hyper_kernel"]
        assert md["scratch"] == 0 and len(ins) > 0, (k, md)
        assert md["lds"] == (learner_kernels["adam_pop_kernel"][0]["lds"] if k == "adam" else 0), (k, md)
