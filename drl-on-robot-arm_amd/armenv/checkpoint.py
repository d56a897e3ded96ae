"""Saving what a training run holds.

Agents, in the reference's own files: ``save_agent(agent, filename)`` / ``load_agent(agent, filename)`` -- also ``agent.save(filename)``
/ ``agent.load(filename)`` of every learner (armenv.td3.TD3, armenv.daddpg.DADDPG, armenv.datd3.DATD3 / DARC and their fused
counterparts) and of a population's ``member(p)`` -- write and read what the reference's ``agent.save`` / ``agent.load`` do
(algo/*/*_mlp.py): one ``torch.save(module.state_dict(), filename + suffix)`` per learning net,

    td3             _critic.pt (the twin critic, fc1 ... fc6), _actor.pt
    daddpg          _critic.pt, _actor1.pt, _actor2.pt
    datd3, darc     _critic1.pt, _actor1.pt, _critic2.pt, _actor2.pt

with the keys, shapes and dtype of the reference's modules, tensors on the CPU: the reference reads our files and we read its.

Whole runs, bit for bit: ``save_run(path, state)`` / ``load_run(path)`` keep the nested ``state_dict()``s of a loop's objects (the
fused learner or population, the trajectory stores, the envs, the PBT schedule) and the loop's own variables in ONE file that holds
nothing but tensors, numbers, strings, lists and dicts; armenv.train and armenv.train_pop write and resume from it
(``checkpoint=``, ``resume=``).  Every random stream of a run is stateless -- Philox over (seed, env, episode, step), over (seed,
sample, draw), over (seed, row, update number), and one ``random.Random`` -- and the fused updates are bitwise reproducible, so a
resumed run equals the uninterrupted one in every bit."""
import os

import torch

from ._lib import ABI_VERSION

FORMAT = 1

# what identifies an agent (an attribute it has) -> its saved nets, in the order of the reference's save()
_AGENT_FILES = (("critic1", ("critic1", "actor1", "critic2", "actor2")),       # datd3, darc
                ("actor2", ("critic", "actor1", "actor2")),                    # daddpg
                ("critic", ("critic", "actor")))                               # td3


def agent_nets(agent):
    """the names of the nets that `agent`'s files hold, in the order they are written; file `name` is ``filename + "_<name>.pt"``"""
    for mark, names in _AGENT_FILES:
        if hasattr(agent, mark):
            return names
    raise TypeError("%s is not an agent that save_agent / load_agent know" % type(agent).__name__)


def save_agent(agent, filename):
    """The reference's ``agent.save(filename)``: the ``state_dict()`` of each learning net, on the CPU, one file per net.  Returns
    the list of the files written."""
    paths = []
    for name in agent_nets(agent):
        path = "%s_%s.pt" % (filename, name)
        torch.save({k: v.detach().to("cpu", copy=True) for k, v in getattr(agent, name).state_dict().items()}, path)
        paths.append(path)
    return paths


@torch.no_grad()
def load_agent(agent, filename):
    """The reference's ``agent.load(filename)`` as it is meant: every learning net takes its file's tensors and every target becomes
    a copy of its net; Adam's moments and the counters stay.  Written through the modules' own tensors, so a population's member
    loads into the stacks.  A missing file, a missing or an extra key and a wrong shape raise ValueError naming the file and the
    key -- all files are read and checked before the first tensor is written."""
    loaded = []
    for name in agent_nets(agent):
        path = "%s_%s.pt" % (filename, name)
        if not os.path.isfile(path):
            raise ValueError("load_agent: %s is missing" % path)
        sd = torch.load(path, map_location="cpu", weights_only=True)
        own = getattr(agent, name).state_dict()
        if not isinstance(sd, dict):
            raise ValueError("load_agent: %s holds no state dict" % path)
        for k in own:
            if k not in sd:
                raise ValueError("load_agent: %s has no key %r" % (path, k))
        for k, v in sd.items():
            if k not in own:
                raise ValueError("load_agent: %s has the extra key %r" % (path, k))
            if not torch.is_tensor(v) or tuple(v.shape) != tuple(own[k].shape):
                raise ValueError("load_agent: %s: %r has shape %s, the net's is %s"
                                 % (path, k, tuple(getattr(v, "shape", ())), tuple(own[k].shape)))
        loaded.append((name, sd))
    for name, sd in loaded:
        net, target = getattr(agent, name).state_dict(), getattr(agent, "target_" + name).state_dict()
        for k, v in sd.items():
            net[k].copy_(v)
            target[k].copy_(net[k])


class AgentFiles:
    """``save(filename)`` / ``load(filename)`` of an agent: save_agent / load_agent as methods"""

    def save(self, filename):
        return save_agent(self, filename)

    def load(self, filename):
        load_agent(self, filename)


# ------------------------------------------------------------------------------------------------ state dicts: shared checks

def to_cpu(t):
    """a CPU copy of a tensor that shares nothing with it"""
    return t.detach().to("cpu", copy=True)


def check_field(who, name, got, want):
    if got != want:
        raise ValueError("%s.load_state_dict: %s is %r in the state, %r here" % (who, name, got, want))


def check_tensors(who, name, saved, own):
    """`saved` against the list of tensors `own` it is to be copied into: count, shapes and dtypes, before anything is written"""
    if not isinstance(saved, (list, tuple)) or len(saved) != len(own):
        raise ValueError("%s.load_state_dict: %s holds %s tensors, %d here" % (who, name, len(saved) if hasattr(saved, "__len__") else "no", len(own)))
    for k, (s, t) in enumerate(zip(saved, own)):
        if not torch.is_tensor(s) or tuple(s.shape) != tuple(t.shape) or s.dtype != t.dtype:
            raise ValueError("%s.load_state_dict: %s[%d] is %s %s in the state, %s %s here"
                             % (who, name, k, getattr(s, "dtype", type(s).__name__), tuple(getattr(s, "shape", ())), t.dtype, tuple(t.shape)))


# ------------------------------------------------------------------------------------------------ the file

def save_run(path, state):
    """Writes `state` -- tensors (saved as CPU tensors) and plain numbers, strings, lists and dicts -- with the format number and the
    package's ABI number on top, to ``path + ".tmp"``, and moves it into place with ``os.replace``: a save that fails leaves the
    previous file as it was and no ``.tmp`` behind."""
    tmp = path + ".tmp"
    try:
        torch.save(dict(format=FORMAT, abi=ABI_VERSION, state=state), tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def load_run(path):
    """The `state` that ``save_run`` wrote, tensors on the CPU.  Read with ``weights_only=True``: nothing but tensors and plain
    containers is ever unpickled.  ValueError for a file of an unknown ``format`` or of another ABI."""
    blob = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or blob.get("format") != FORMAT:
        raise ValueError("load_run: %s has format %r; this build reads format %d"
                         % (path, blob.get("format") if isinstance(blob, dict) else None, FORMAT))
    if blob.get("abi") != ABI_VERSION:
        raise ValueError("load_run: %s was written by ABI %r; this build is ABI %d" % (path, blob.get("abi"), ABI_VERSION))
    return blob["state"]


# ------------------------------------------------------------------------------------------------ what the loops share

def check_config(saved, config):
    """A resumed run must be the run that was saved: ValueError naming the first field of `config` (the call's) that the saved one
    does not hold with the same value"""
    for name, value in config.items():
        if name not in saved:
            raise ValueError("resume: the checkpoint's config has no %s" % name)
        if saved[name] != value:
            raise ValueError("resume: %s is %r in the checkpoint, %r in this call" % (name, saved[name], value))
    for name in saved:
        if name not in config:
            raise ValueError("resume: the checkpoint's config has %s, which this call does not know" % name)


def check_loop_arguments(learner, checkpoint, checkpoint_every, resume, save, save_best):
    """the refusals that armenv.train's and armenv.train_pop's loops share, before anything is created"""
    if learner == "torch" and (checkpoint is not None or resume is not None):
        raise ValueError("checkpoint / resume need learner='hip' or 'fused': the torch learner's noise comes from torch's device "
                         "generator and its captured graphs cannot be restored (save= works for it)")
    if isinstance(checkpoint_every, bool) or int(checkpoint_every) != checkpoint_every or checkpoint_every < 0:
        raise ValueError("checkpoint_every = %r must be an integer >= 0" % (checkpoint_every,))
    if checkpoint_every and checkpoint is None:
        raise ValueError("checkpoint_every needs checkpoint, the file to write")
    if save_best and save is None:
        raise ValueError("save_best needs save, the name of the agent's files")


def checkpoint_due(iteration, iterations, checkpoint, checkpoint_every):
    """whether the state is written after iteration `iteration` (counted from 1): every `checkpoint_every`-th and the last one"""
    return checkpoint is not None and (iteration == iterations or (checkpoint_every > 0 and iteration % checkpoint_every == 0))


class BestKeeper:
    """The reference's ``if success_rate >= best: agent.save(...)`` (main.py:151-153) for one agent: ``offer(rate, agent)`` writes
    ``filename + ".best"`` at the first rate it is offered and again whenever a rate reaches the best so far (>=); returns whether
    it wrote.  ``state_dict`` / ``load_state_dict``: the best so far, so a resumed run keeps comparing against it."""

    def __init__(self, filename, write=save_agent):
        self.filename, self.best, self._write = filename, None, write

    def offer(self, rate, agent):
        if self.best is not None and not rate >= self.best:
            return False
        self.best = float(rate)
        self._write(agent, self.filename + ".best")
        return True

    def state_dict(self):
        return dict(best=self.best)

    def load_state_dict(self, sd):
        self.best = sd["best"]


def add_cli_arguments(ap):
    """the five flags of python -m armenv.train and python -m armenv.train_pop"""
    ap.add_argument("--checkpoint", default=None, metavar="FILE", help="write the whole run's state to FILE (after --checkpoint-every "
                    "iterations and after the last one); --resume FILE continues it bit for bit")
    ap.add_argument("--checkpoint-every", type=int, default=0, metavar="N")
    ap.add_argument("--resume", default=None, metavar="FILE", help="continue the run that --checkpoint wrote; every other argument as then")
    ap.add_argument("--save", default=None, metavar="NAME", help="write the trained agent in the reference's files NAME_actor.pt, ... "
                    "(a population: NAME.m<p>_...)")
    ap.add_argument("--save-best", action="store_true", help="also write NAME.best_... whenever a logged success rate reaches its best")


def check_cli_arguments(ap, a, learner):
    """``ap.error`` for what the loops would refuse"""
    try:
        check_loop_arguments(learner, a.checkpoint, a.checkpoint_every, a.resume, a.save, a.save_best)
    except ValueError as e:
        ap.error("--checkpoint / --resume / --save: %s" % e)
    if a.resume is not None and not os.path.isfile(a.resume):
        ap.error("--resume %s: no such file" % a.resume)
