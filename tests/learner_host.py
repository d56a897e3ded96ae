"""What the CPU tests of the fused learners' host side share (test infrastructure; no device is needed): the layout of a ctypes struct
against include/armenv.h, the table of agents, made-up argument structs for the refusal tests, the refusals themselves as data
(tests/learner_abi.py records them into tests/golden/learner_abi.json in this order), the population and single classes of a kind,
and the learner kernels of the built code object."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import pytest

from armenv import _lib as L
from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import isa  # noqa: E402

HEADER_DIR = os.path.join(ROOT, "include")
LAYERS = ("W1", "b1", "W2", "b2", "W3", "b3")
ARRAYS = ("states_dev", "actions_dev", "next_states_dev", "rewards_dev", "dones_dev", "workspace_dev")
TD3_NETS = ("actor", "q1", "q2", "target_actor", "target_q1", "target_q2", "actor_m", "actor_v", "q1_m", "q1_v", "q2_m", "q2_v")
DADDPG_NETS = ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic",
               "actor1_m", "actor1_v", "actor2_m", "actor2_v", "critic_m", "critic_v")
DATD3_NETS = ("actor1", "actor2", "critic1", "critic2", "target_actor1", "target_actor2", "target_critic1", "target_critic2",
              "actor1_m", "actor1_v", "actor2_m", "actor2_v", "critic1_m", "critic1_v", "critic2_m", "critic2_v")

# kind -> the argument structs, the stacks of `one` in struct order, the C entry points' stem and the agent's own scalar fields
_NOISE = dict(policy_noise=0.2, noise_clip=0.5)
AGENTS = dict(
    td3=dict(args=L.ArmEnvTd3Args, pop_args=L.ArmEnvTd3PopArgs, nets=TD3_NETS, stem="td3", scalars=dict(_NOISE, with_actor=1)),
    daddpg=dict(args=L.ArmEnvDaddpgArgs, pop_args=L.ArmEnvDaddpgPopArgs, nets=DADDPG_NETS, stem="daddpg", scalars=dict(update_actor=2)),
    datd3=dict(args=L.ArmEnvDatd3Args, pop_args=L.ArmEnvDatd3PopArgs, nets=DATD3_NETS, stem="datd3",
               scalars=dict(_NOISE, update_actor=2, darc=0, q_weight=0.2, regularization_weight=0.005)))
AGENTS["darc"] = dict(AGENTS["datd3"], scalars=dict(AGENTS["datd3"]["scalars"], darc=1))


def ctypes_layout(struct):
    """[(C member path, offset)] of every scalar member of a ctypes struct, nested structs flattened"""
    out = []
    for name, typ in struct._fields_:
        off = getattr(struct, name).offset
        if isinstance(typ, type) and issubclass(typ, C.Structure):
            out += [(f"{name}.{k}", off + o) for k, o in ctypes_layout(typ)]
        else:
            out.append((name, off))
    return out


def header_layout(struct, extra=(), checks=(), std="c99", werror=False):
    """(sizes, offsets) as the C compiler reads them from include/armenv.h: sizes = [sizeof of the struct that the ctypes `struct` is
    named after, then the C expressions `extra`], offsets = offsetof of every member of ctypes_layout(struct), in its order.  `checks`
    are further statements of the program (static assertions: the compiler is their test)."""
    name = struct.__name__
    exprs = ["sizeof(%s)" % name] + list(extra) + ["offsetof(%s, %s)" % (name, m) for m, _ in ctypes_layout(struct)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "armenv.h"', "int main(void) {"]
    lines += ['  printf("%%ld\\n", (long)(%s));' % e for e in exprs] + ["  " + c for c in checks] + ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=" + std, "-Wall"] + ["-Werror"] * werror + ["-I", HEADER_DIR, "-o", exe, src], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    return out[:1 + len(extra)], out[1 + len(extra):]


def _fill(a, kind, B, D, addr, step, scalars):
    """shape, hyper-parameters and `scalars`, then one made-up 16-byte aligned address per array, `step` apart, in struct order"""
    a.device, a.state_dim, a.action_dim, a.hidden_dim, a.batch = 0, D, 3, 256, B
    a.action_bound, a.gamma, a.tau = 0.7, 0.98, 0.005
    a.actor_lr, a.critic_lr, a.beta1, a.beta2, a.eps = 1e-3, 1e-3, 0.9, 0.999, 1e-8
    a.critic_step, a.actor_step = 1, 1
    for name, value in scalars.items():
        setattr(a, name, value)
    for target, names in [(getattr(a, net), LAYERS) for net in AGENTS[kind]["nets"]] + [(a, ARRAYS)]:
        for k in names:
            addr += step
            setattr(target, k, addr)


def fake_args(kind, B=64, D=6, **scalars):
    """Arguments of armenv_<stem>_update that pass every check but the one a test breaks: made-up (never dereferenced) device pointers
    from 0x11000 on, 0x1000 apart.  NOT to be passed unmodified -- a valid set would be enqueued."""
    row = AGENTS[kind]
    a = row["args"]()
    _fill(a, kind, B, D, 0x10000, 0x1000, dict(row["scalars"], **scalars))
    a.workspace_bytes = getattr(L.load(), "armenv_%s_workspace_bytes" % row["stem"])(D, 256, B)
    assert a.workspace_bytes > 0
    return a


def fake_pop_args(kind, P=3, B=64, D=6, **scalars):
    """fake_args for armenv_<stem>_pop_update[_hyper]: P members, the stacks from 0x11000000 on, 0x1000000 apart (room for every
    member of every array at these sizes); the two-actor agents step actor 1"""
    row = AGENTS[kind]
    pa = row["pop_args"]()
    pa.members = P
    first = dict(update_actor=1) if "update_actor" in row["scalars"] else {}
    _fill(pa.one, kind, B, D, 0x10000000, 0x1000000, {**row["scalars"], **first, **scalars})
    pa.one.workspace_bytes = getattr(L.load(), "armenv_%s_pop_workspace_bytes" % row["stem"])(D, 256, B, P)
    assert pa.one.workspace_bytes > 0
    return pa


# ---- the refusals: (a word of the message, what breaks the arguments) ----

def _set(field, value):
    return lambda a: setattr(a, field, value)


def _net(net, key, value=None):
    return lambda a: setattr(getattr(a, net), key, value)


def _shift(net, key, by):
    """a misaligned pointer"""
    return lambda a: setattr(getattr(a, net), key, getattr(getattr(a, net), key) + by)


def _one(mutate):
    """a mutation of the single arguments, applied to a population's `one`"""
    return lambda pa: mutate(pa.one)


_SHORT_WORKSPACE = ("workspace_bytes", lambda a: setattr(a, "workspace_bytes", a.workspace_bytes - 1))
_TWO_ACTOR_HEAD = [
    ("batch", _set("batch", 0)),
    ("batch", _set("batch", (1 << 20) + 1)),
    ("hidden_dim", _set("hidden_dim", 128)),
    ("state_dim", _set("state_dim", 0)),
    ("state_dim", _set("state_dim", 13)),
    ("action_dim", _set("action_dim", 2)),
    ("update_actor", _set("update_actor", 0)),
    ("update_actor", _set("update_actor", 3)),
]
REFUSALS = dict(
    td3=[
        ("batch", _set("batch", 0)),
        ("hidden_dim", _set("hidden_dim", 128)),
        ("state_dim", _set("state_dim", 0)),
        ("state_dim", _set("state_dim", 13)),
        ("q2", _net("q2", "W2")),
        ("actor_v", _net("actor_v", "b3")),
        ("states_dev", _set("states_dev", None)),
        ("dones_dev", _set("dones_dev", None)),
        ("workspace_dev", _set("workspace_dev", None)),
        _SHORT_WORKSPACE,
        ("action_dim", _set("action_dim", 2)),
        ("gamma", _set("gamma", float("nan"))),
    ],
    daddpg=_TWO_ACTOR_HEAD + [
        ("critic_step", _set("critic_step", 0)),
        ("actor_step", _set("actor_step", 0)),
        ("gamma", _set("gamma", float("nan"))),
        ("tau", _set("tau", 1.5)),
        ("beta1", _set("beta1", 1.0)),
        ("eps", _set("eps", 0.0)),
        ("actor1", _net("actor1", "W1")),
        ("actor2", _net("actor2", "b3")),
        ("critic", _net("critic", "W2")),
        ("target_actor2", _net("target_actor2", "W3")),
        ("target_critic", _shift("target_critic", "b1", 4)),
        ("actor1_m", _net("actor1_m", "b2")),
        ("actor2_v", _shift("actor2_v", "W1", 8)),
        ("critic_v", _net("critic_v", "b3")),
        ("states_dev", _set("states_dev", None)),
        ("dones_dev", _set("dones_dev", None)),
        ("workspace_dev", _set("workspace_dev", None)),
        ("workspace_dev", lambda a: setattr(a, "workspace_dev", a.workspace_dev + 4)),
        _SHORT_WORKSPACE,
    ],
    # recorded, and parametrised, over fake_args("darc")
    datd3=_TWO_ACTOR_HEAD + [
        ("darc", _set("darc", 2)),
        ("darc", _set("darc", -1)),
        ("critic_step", _set("critic_step", 0)),
        ("actor_step", _set("actor_step", 0)),
        ("action_bound", _set("action_bound", 0.0)),
        ("gamma", _set("gamma", float("nan"))),
        ("tau", _set("tau", 1.5)),
        ("policy_noise", _set("policy_noise", -0.1)),
        ("noise_clip", _set("noise_clip", float("inf"))),
        ("actor_lr", _set("actor_lr", -1e-3)),
        ("critic_lr", _set("critic_lr", float("nan"))),
        ("beta1", _set("beta1", 1.0)),
        ("beta2", _set("beta2", -0.1)),
        ("eps", _set("eps", 0.0)),
        ("q_weight", _set("q_weight", 1.5)),
        ("q_weight", _set("q_weight", -0.1)),
        ("regularization_weight", _set("regularization_weight", -0.005)),
        ("regularization_weight", _set("regularization_weight", float("nan"))),
    ] + [(net, _net(net, key)) for net, key in zip(DATD3_NETS, LAYERS * 3)] + [
        ("target_critic2", _shift("target_critic2", "b1", 4)),
        ("critic1_v", _shift("critic1_v", "W1", 8)),
        ("states_dev", _set("states_dev", None)),
        ("actions_dev", _set("actions_dev", None)),
        ("next_states_dev", _set("next_states_dev", None)),
        ("rewards_dev", _set("rewards_dev", None)),
        ("dones_dev", _set("dones_dev", None)),
        ("workspace_dev", _set("workspace_dev", None)),
        ("workspace_dev", lambda a: setattr(a, "workspace_dev", a.workspace_dev + 4)),
        _SHORT_WORKSPACE,
    ])

_TWO_ACTOR_POP = [
    ("members", _set("members", 0)),
    ("members", _set("members", 65)),
    ("members", _set("members", -1)),
    ("update_actor", _one(_set("update_actor", 0))),
    ("update_actor", _one(_set("update_actor", 3))),
    ("target_actor2", _one(_net("target_actor2", "W2"))),
    ("actor2_v", _one(_shift("actor2_v", "b3", 4))),
    ("states_dev", _one(_set("states_dev", None))),
    ("workspace_bytes", _one(_SHORT_WORKSPACE[1])),
    ("gamma", _one(_set("gamma", float("nan")))),
    ("batch", _one(_set("batch", 0))),
    ("hidden_dim", _one(_set("hidden_dim", 128))),
    ("actor_step", _one(_set("actor_step", 0))),
]
POP_REFUSALS = dict(
    td3=[
        ("members", _set("members", 0)),
        ("members", _set("members", 65)),
        ("target_q2", _one(_net("target_q2", "W2"))),
        ("states_dev", _one(_set("states_dev", None))),
        ("workspace_bytes", _one(_SHORT_WORKSPACE[1])),
        ("gamma", _one(_set("gamma", float("nan")))),
        ("batch", _one(_set("batch", 0))),
        ("hidden_dim", _one(_set("hidden_dim", 128))),
    ],
    daddpg=_TWO_ACTOR_POP, datd3=_TWO_ACTOR_POP)
# DATD3's and DARC's own: (a word of the message, `darc` of the arguments, what breaks them)
POP_REFUSALS_DATD3 = [
    ("darc", 0, _one(_set("darc", 2))),
    ("darc", 0, _one(_set("darc", -1))),
    ("q_weight", 1, _one(_set("q_weight", 1.5))),
    ("q_weight", 1, _one(_set("q_weight", -0.1))),
    ("regularization_weight", 1, _one(_set("regularization_weight", -1.0))),
    ("policy_noise", 0, _one(_set("policy_noise", -0.1))),
    ("critic2_m", 1, _one(_net("critic2_m", "W1"))),
]


def refused(fn, *args):
    """the message of a call that must be refused with ARMENV_EINVAL (not ENODEV: nothing touched the device) under its own name"""
    lib = L.load()
    rc, msg = getattr(lib, fn)(*args), lib.armenv_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(fn), msg
    return msg


def classes(kind):
    """(population class, single class, the C entry points' stem)"""
    from armenv.fused_daddpg import FusedDADDPG
    from armenv.fused_daddpg_pop import FusedDADDPGPopulation
    from armenv.fused_datd3 import FusedDARC, FusedDATD3
    from armenv.fused_datd3_pop import FusedDARCPopulation, FusedDATD3Population
    from armenv.fused_td3 import FusedTD3
    from armenv.fused_td3_pop import FusedTD3Population
    pop, single = dict(td3=(FusedTD3Population, FusedTD3), daddpg=(FusedDADDPGPopulation, FusedDADDPG),
                       datd3=(FusedDATD3Population, FusedDATD3), darc=(FusedDARCPopulation, FusedDARC))[kind]
    return pop, single, AGENTS[kind]["stem"]


# ---- the built code object ----

@functools.lru_cache(maxsize=None)
def all_kernels():
    """tools/isa.py's rows of every kernel of the built library, disassembled once per session"""
    if not os.path.exists(isa.LIB):
        pytest.skip("libarmenv.so is not built")
    if not os.path.exists(os.path.join(isa.LLVM, "llvm-objdump")):
        pytest.skip("the ROCm LLVM tools (llvm-objdump, llvm-readelf) are not installed")
    return isa.all_kernels()


@pytest.fixture(scope="module")
def learner_kernels():
    rows = [r for r in all_kernels() if "armenv::learner::" in r[1]]
    return {dm.split("armenv::learner::")[1].split("(")[0]: (md, ins) for _, dm, md, ins in rows}
