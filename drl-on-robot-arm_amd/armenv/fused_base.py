"""What the fused learners (fused_td3.FusedTD3, fused_daddpg.FusedDADDPG, fused_datd3.FusedDATD3 / FusedDARC) and their populations
share: the ArmEnvMlpRW views of their nets, the stored hyper-parameters, the batch and workspace tensors, the argument struct's common
part and the one call into libarmenv.so."""
import ctypes as C
from functools import cached_property

import torch

from . import _lib as L
from .checkpoint import AgentFiles, check_field, check_tensors, to_cpu


def _mlp(net, heads=("fc1", "fc2", "fc3")):
    m = L.ArmEnvMlpRW()
    for i, name in enumerate(heads):
        layer = getattr(net, name)
        for key, t in (("W%d" % (i + 1), layer.weight), ("b%d" % (i + 1), layer.bias)):
            assert t.is_contiguous() and t.dtype == torch.float32
            setattr(m, key, t.data_ptr())
    return m


def _mlp_of(tensors):
    """ArmEnvMlpRW over six tensors in W1, b1, W2, b2, W3, b3 order"""
    m = L.ArmEnvMlpRW()
    for key, t in zip(("W1", "b1", "W2", "b2", "W3", "b3"), tensors):
        setattr(m, key, t.data_ptr())
    return m


class FusedLearner(AgentFiles):
    """Base of the fused learners and, through fused_pop_base.FusedPopulation, of their populations.  An agent's schedule class (the
    mixin next to its single learner: fused_td3.TD3Schedule, ...) names the C entry points' argument struct ``_Args``, the
    hyper-parameters ``_hyper`` it copies into the struct beside the common ones, the constructor's hyper-parameters ``_HYPER_KW``
    and the host counters ``_COUNTERS``, and holds ``train``; the learner names its entry points (``_fn`` of armenv_<_fn>_update and
    armenv_<_fn>_workspace_bytes) and which exception ``_noise_error`` a wrongly shaped ``noise`` raises, and creates its own nets,
    in its torch learner's order.  What a population overrides of the call path: ``_lead``, the shape in front of every tensor -- ()
    here, (P,) there: the loss's shape, what precedes [B][action_dim] in `noise`, and the workspace query's further argument --,
    ``_batch_axis`` (which axis of the batch is B, ``len(_lead)``) and ``_per_call_struct``.

    ``save`` / ``load``: the agent in the reference's files (armenv.checkpoint).  ``state_dict()`` / ``load_state_dict(sd)``: the
    whole learner -- every net, target and moment tensor, the counters and the noise seed -- as CPU tensors and plain numbers, for a
    run that is to continue bit for bit; a single learner names its learning nets ``_LEARNING``."""

    _fn = _Args = None
    _hyper = _HYPER_KW = _COUNTERS = ()       # _hyper: fields of the C struct; _HYPER_KW: keyword arguments of the constructor
    _takes_seed = False                       # whether the constructor has `seed` (the agent draws target-policy noise)
    _noise_error = ValueError
    _lead, _batch_axis = (), 0
    _LEARNING = ()                            # a single learner's learning nets: each has a target_<name>, <name>_m and <name>_v

    def _check_shapes(self, state_dim, action_dim, hidden_dim):
        if hidden_dim != 256 or action_dim != 3 or not 1 <= state_dim <= 12:
            raise ValueError("%s: the fused update is built for hidden_dim 256, action_dim 3, state_dim 1..12" % type(self).__name__)

    def _configure(self, state_dim, action_dim, action_bound, **hyper):
        """What the constructors of an agent's single learner and of its population share: the shape check, the shapes, the agent's
        hyper-parameters (every name of ``_HYPER_KW``) and Adam's constants as attributes, the counters at 0, nothing bound yet."""
        if set(hyper) != set(self._HYPER_KW):                     # a population's **darc may carry a name its agent does not take
            raise TypeError("%s: hyper-parameters missing: %s; not taken: %s" % (type(self).__name__, sorted(set(self._HYPER_KW) - set(hyper)),
                                                                                 sorted(set(hyper) - set(self._HYPER_KW))))
        self._check_shapes(state_dim, action_dim, hyper["hidden_dim"])
        self.state_dim, self.action_dim, self.action_bound = state_dim, action_dim, action_bound
        for name, value in hyper.items():
            setattr(self, name, value)
        self.betas, self.eps = (0.9, 0.999), 1e-8                 # torch.optim.Adam's defaults, as the torch learners' optimisers
        for name in self._COUNTERS:
            setattr(self, name, 0)
        self._ws = self._args = self._one = None                  # _one: the per-call struct inside _args, set where _args is

    def _static_args(self):
        """the part of the argument struct that does not change between updates: what every update has; a subclass adds its nets"""
        a = self._Args()
        a.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        a.state_dim, a.action_dim, a.hidden_dim = self.state_dim, self.action_dim, self.hidden_dim
        a.action_bound, a.beta1, a.beta2, a.eps = self.action_bound, self.betas[0], self.betas[1], self.eps
        for name in ("gamma", "tau", "actor_lr", "critic_lr") + self._hyper:
            setattr(a, name, self._hp(name))
        return a

    def _hp(self, name):
        """the value of hyper-parameter `name` that the argument struct carries; a population with members' own values: member 0's"""
        return getattr(self, name)

    def batch_buffers(self, batch_size):
        """static input tensors of `batch_size` rows that ``TrajectoryStore.sample(out=...)`` fills in place"""
        B, D, dev = int(batch_size), self.state_dim, self.device
        return dict(states=torch.zeros(B, D, device=dev), actions=torch.zeros(B, self.action_dim, device=dev),
                    next_states=torch.zeros(B, D, device=dev), rewards=torch.zeros(B, device=dev),
                    dones=torch.zeros(B, dtype=torch.uint8, device=dev))

    @cached_property
    def _update_fn(self):
        return getattr(L.load(), "armenv_%s_update" % self._fn)

    @cached_property
    def _workspace_fn(self):
        return getattr(L.load(), "armenv_%s_workspace_bytes" % self._fn)

    def _workspace(self, B):
        """the workspace of an update of B rows (kept, and grown when needed); an unsupported batch size raises ValueError.  The
        schedules call this before they move a counter, so a refused batch leaves the learner as it was."""
        n = self._workspace_fn(self.state_dim, self.hidden_dim, B, *self._lead)
        if n < 0:
            raise ValueError("%s: unsupported batch size %d" % (type(self).__name__, B))
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._ws

    def _inputs(self, batch):
        """(states, actions, rewards, next_states, dones) of a batch dict as the contiguous f32 / uint8 device tensors the update reads"""
        dev = self.device
        f32 = lambda k: batch[k].to(dev, torch.float32).contiguous()
        r = batch["rewards"].to(dev, torch.float32).reshape(-1).contiguous()
        d = batch["dones"].to(dev)
        d = (d if d.dtype == torch.uint8 else (d != 0).to(torch.uint8)).reshape(-1).contiguous()
        return f32("states"), f32("actions"), r, f32("next_states"), d

    def _noise(self, noise, B):
        """`noise` as the [B][action_dim] ([P][B][action_dim]) f32 device tensor the update reads, or None"""
        if noise is not None:
            noise = noise.to(self.device, torch.float32).contiguous()
            if tuple(noise.shape) != self._lead + (B, self.action_dim):
                raise self._noise_error("noise must be %s[B][%d] standard normals" % ("[P]" * len(self._lead), self.action_dim))
        return noise

    @staticmethod
    def _per_call_struct(args):
        """the struct of `args` that holds what changes between updates"""
        return args

    def _bind(self, args):
        """makes `args` the argument struct of the updates to come"""
        self._args, self._one = args, self._per_call_struct(args)
        self._has_noise = hasattr(self._one, "noise_dev")

    def _call(self, ws, s, a, r, s2, d, noise=None, **per_call):
        """One armenv_<_fn>_update over prepared tensors and the workspace `ws` on the current stream, with `per_call` (step numbers,
        which nets, draw) written into the argument struct first; returns the critic loss (no host sync): a 0-dim tensor, [P] from a
        population."""
        if self._args is None:
            self._bind(self._static_args())
        one = self._one
        loss = torch.empty(self._lead, dtype=torch.float32, device=self.device)
        one.batch = s.shape[self._batch_axis]
        for key, value in per_call.items():
            setattr(one, key, value)
        if self._has_noise:
            one.noise_dev = noise.data_ptr() if noise is not None else None
        one.states_dev, one.actions_dev, one.next_states_dev = s.data_ptr(), a.data_ptr(), s2.data_ptr()
        one.rewards_dev, one.dones_dev, one.loss_dev = r.data_ptr(), d.data_ptr(), loss.data_ptr()
        one.workspace_dev, one.workspace_bytes = ws.data_ptr(), ws.numel()
        L.check(self._enqueue(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return loss

    def _enqueue(self, stream):
        """the one call into libarmenv.so over the bound argument struct; returns its code"""
        return self._update_fn(C.byref(self._args), stream)

    @torch.no_grad()
    def _load_from(self, learner, names):
        """Copies parameters, the Adam moments and step counters of the nets `names` (`<name>_opt` of the torch learner) and total_it."""
        for mine, theirs in zip(self._nets(), learner._nets()):
            for p, q in zip(mine.parameters(), theirs.parameters()):
                p.copy_(q)
        for name in names:
            opt = getattr(learner, name + "_opt")
            step = 0
            for p, m, v in zip(getattr(learner, name).parameters(), getattr(self, name + "_m"), getattr(self, name + "_v")):
                st = opt.state.get(p, {})
                if "exp_avg" in st:
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                    step = int(st["step"])
                else:
                    m.zero_()
                    v.zero_()
            setattr(self, name + "_step", step)
        self.total_it = learner.total_it

    # ---- the whole learner's state (armenv.checkpoint)
    def _state_tensors(self):
        """name -> the list of this learner's own tensors under it: the nets' and targets' parameters and the moments"""
        out = {}
        for name in self._LEARNING:
            out[name] = list(getattr(self, name).parameters())
            out["target_" + name] = list(getattr(self, "target_" + name).parameters())
            out[name + "_m"], out[name + "_v"] = getattr(self, name + "_m"), getattr(self, name + "_v")
        return out

    def _state_header(self):
        """the fields that must agree before a state is loaded, in the order they are checked"""
        return dict(kind=type(self).__name__, state_dim=self.state_dim, action_dim=self.action_dim, hidden_dim=self.hidden_dim)

    def state_dict(self):
        """The learner's whole state: CPU copies of every net, target and moment tensor, the counters and the seed (None for an
        agent that draws no noise).  The hyper-parameters are the constructor's and are not part of it."""
        return dict(self._state_header(), seed=getattr(self, "seed", None), counters={n: int(getattr(self, n)) for n in self._COUNTERS},
                    tensors={name: [to_cpu(t) for t in ts] for name, ts in self._state_tensors().items()})

    def _check_state(self, sd):
        who = type(self).__name__
        for name, value in self._state_header().items():
            check_field(who, name, sd.get(name), value)
        check_field(who, "counters", sorted(sd["counters"]), sorted(self._COUNTERS))
        own = self._state_tensors()
        check_field(who, "tensors", sorted(sd["tensors"]), sorted(own))
        for name, ts in own.items():
            check_tensors(who, name, sd["tensors"][name], ts)
        if (sd["seed"] is None) != (getattr(self, "seed", None) is None):
            check_field(who, "seed", sd["seed"], getattr(self, "seed", None))

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Restores ``state_dict()``'s state in place; ValueError naming the first field that does not fit (kind, a shape, ...)
        before anything is changed.  The bound argument struct is dropped: the next ``train`` binds anew."""
        self._check_state(sd)
        for name, ts in self._state_tensors().items():
            for t, s in zip(ts, sd["tensors"][name]):
                t.copy_(s)
        for name, value in sd["counters"].items():
            setattr(self, name, int(value))
        if sd["seed"] is not None:
            self.seed = int(sd["seed"])
        self._args = self._one = None

    @torch.no_grad()
    def _take_action_of_two(self, state, critic1, critic2):
        """the two-actor agents' take_action: the proposal of actor1 / actor2 that its critic values higher"""
        import numpy as np
        s = torch.tensor(np.asarray([state], dtype=np.float32), device=self.device)
        a1, a2 = self.actor1(s), self.actor2(s)
        q1, q2 = critic1(s, a1), critic2(s, a2)
        return (a1 if bool(q1 >= q2) else a2).cpu().numpy()[0]
