"""What the populations of fused learners (fused_td3_pop.FusedTD3Population, fused_daddpg_pop.FusedDADDPGPopulation,
fused_datd3_pop.FusedDATD3Population / FusedDARCPopulation) share: the stacks [P][rows][cols] that hold every member's nets and Adam
moments and the re-pointing of the members' module parameters into them, the stacked batch buffers, the checks of a stacked batch,
what differs in FusedLearner's one call into libarmenv.so (armenv_<algo>_pop_update) and the member-state zip behind load_member /
export_member.  The step schedule is the agent's own, shared with its single learner (fused_td3.TD3Schedule, ...).

Per-member hyper-parameters: every constructor takes, for each of its agent's ``sweepable()`` names (the learning rates, tau, gamma,
the target-policy noise's two, DARC's two weights), a scalar for all members or a sequence of P values; ``hyper(p)`` / ``set_hyper(p,
...)`` read and change one member's, ``copy_member`` is the exploit step of a population-based schedule for one member and
``exploit(src)`` the same for a whole plan in ONE launch (armenv_pop_exploit); armenv.pbt makes the plans.  While every member holds
the same values the update is armenv_<algo>_pop_update, as before; once two members differ it is armenv_<algo>_pop_update_hyper,
which hands each member's values to the kernels.  Members always share the step schedule (so ``policy_freq``), Adam's constants,
``action_bound`` and the shapes."""
import ctypes as C

import torch

from . import _lib as L
from .checkpoint import AgentFiles, check_field
from .fused_base import FusedLearner, _mlp_of

MAX_MEMBERS = 64
_NOT_SWEEPABLE = ("hidden_dim", "policy_freq")          # a shape, and the step schedule: the members' one
_UNIT_RANGE = ("gamma", "tau", "q_weight")              # in [0, 1]; every other sweepable value: >= 0 (the C entry points' ranges)


def _check_range(who, name, value):
    """The C entry points' range of hyper-parameter `name`, checked where the value is given: ``train`` moves its counters before
    the call, so a value that the call would refuse must not get that far."""
    if not (0.0 <= value <= 1.0 if name in _UNIT_RANGE else 0.0 <= value < float("inf")):      # NaN fails both
        raise ValueError("%s: %s = %r out of range" % (who, name, value))


def _values(value):
    """the list of a sequence's values, or None for a scalar"""
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__"):
        return None
    try:
        return [float(v) for v in value]
    except TypeError:                                   # a 0-dim array or tensor
        return None


def check_plan(who, src, members):
    """An exploit plan as a list of `members` ints: member p becomes a copy of member src[p].  armenv_pop_exploit's rules, checked
    on the host: one entry per member, each a member's index, and no source that is itself replaced (src[src[p]] == src[p]), so the
    outcome does not depend on the order of the copies.  ValueError otherwise."""
    try:
        plan = [int(v) for v in src]
    except (TypeError, ValueError):
        raise ValueError("%s: src must be a sequence of %d member indices" % (who, members)) from None
    if len(plan) != members or any(v != w for v, w in zip(plan, src)):
        raise ValueError("%s: src must be a sequence of %d member indices" % (who, members))
    for p, v in enumerate(plan):
        if not 0 <= v < members:
            raise ValueError("%s: src[%d] = %d outside 0..%d" % (who, p, v, members - 1))
    for p, v in enumerate(plan):
        if plan[v] != v:
            raise ValueError("%s: src[%d] = %d is itself replaced (src[%d] = %d)" % (who, p, v, v, plan[v]))
    return plan


class TwoActorMember(AgentFiles):
    """Member p of a population of two-actor agents: the agent's modules, under the names its single learner gives them, whose
    parameters are views into the population's stacks (what the update writes, they show; what is written through them, the update
    reads), with the single learner's ``take_action``, ``policy_state_dicts()`` and ``save`` / ``load`` (through the views)."""

    _take_action_of_two = FusedLearner._take_action_of_two

    def __init__(self, index, device, names, nets, critics):
        self.index, self.device = index, device
        self._names = names
        for name, net in zip(names, nets):
            setattr(self, name, net)
        self._critics = critics            # names of the two critics take_action compares (DADDPG: the one critic twice)

    @property
    def actor(self):
        return self.actor1

    def _nets(self):
        return tuple(getattr(self, n) for n in self._names)

    def take_action(self, state):
        return self._take_action_of_two(state, getattr(self, self._critics[0]), getattr(self, self._critics[1]))

    def policy_state_dicts(self):
        """the learning nets that the rollout's fused policy reads, in set_policy_daddpg's / set_policy_datd3's order"""
        policy = [n for n in self._names if not n.startswith("target_")]
        return tuple({k: v.detach() for k, v in getattr(self, n).state_dict().items()} for n in policy)


class FusedPopulation(FusedLearner):
    """Base of the populations.  A subclass names its single learner ``_Single`` and its argument struct ``_PopArgs`` (``_Args`` is
    the struct of `one`), the stacks of its nets ``_NETS`` (ArmEnvMlpRW fields of `one`, in the order of ``_sixes``) and of its
    moments ``_MOMENTS`` (pairs (moment stack, the net it belongs to)); the schedule's counters ``_COUNTERS`` are the population's."""

    _Single = _PopArgs = None
    _NETS = _MOMENTS = ()
    _batch_axis = 1
    always_hyper = False        # take armenv_<algo>_pop_update_hyper even while the members' values coincide (tests, A/B timing)

    @classmethod
    def sweepable(cls):
        """the hyper-parameters that every member may have a value of its own of"""
        return tuple(n for n in cls._HYPER_KW if n not in _NOT_SWEEPABLE)

    def _configure_members(self, members, state_dim, action_dim, action_bound, **hyper):
        """``_configure`` for a population: each of `hyper` a scalar, or -- a sweepable name only -- a sequence of `members` values.
        An attribute of this object is the members' common value, as a scalar population's always was, or the tuple of their values."""
        who = type(self).__name__
        if not 1 <= int(members) <= MAX_MEMBERS:
            raise ValueError("%s: members must be 1..%d" % (who, MAX_MEMBERS))
        P, rows, first = int(members), {}, {}
        for name, value in hyper.items():
            values = _values(value)
            if values is None:
                values = [value] * P
            elif name not in self.sweepable():
                raise ValueError("%s: %s takes one value for all members" % (who, name))
            elif len(values) != P:
                raise ValueError("%s: %s has %d values for %d members" % (who, name, len(values), P))
            else:
                for v in values:
                    _check_range(who, name, v)
            first[name] = values[0]
            if name in self.sweepable():
                rows[name] = values
        self._configure(state_dim, action_dim, action_bound, **first)
        self._rows = [{name: values[p] for name, values in rows.items()} for p in range(P)]
        self._hyper_changed()

    def _hyper_changed(self):
        """after a change of the members' values: the attributes, and the call is bound anew"""
        for name in self._rows[0]:
            values = [row[name] for row in self._rows]
            setattr(self, name, values[0] if all(v == values[0] for v in values) else tuple(values))
        self._args = self._one = self._table = None

    def _hp(self, name):
        return self._rows[0][name] if name in self._rows[0] else getattr(self, name)

    def uniform(self):
        """whether all members hold the same hyper-parameters (then the update is the shared-scalar armenv_<algo>_pop_update)"""
        return all(row == self._rows[0] for row in self._rows)

    @property
    def entry_point(self):
        """the name of the C entry point that the next ``train`` calls"""
        return "armenv_%s_update%s" % (self._fn, "_hyper" if self.always_hyper or not self.uniform() else "")

    def hyper(self, p):
        """member p's hyper-parameters: a dict over ``sweepable()``"""
        return dict(self._rows[p])

    def set_hyper(self, p, **values):
        """Gives member p new values of sweepable hyper-parameters; in effect from the next ``train``.  A captured graph keeps the
        values it was captured with."""
        for name in values:
            if name not in self.sweepable():
                raise ValueError("%s.set_hyper: %s is not one of %s" % (type(self).__name__, name, ", ".join(self.sweepable())))
            _check_range(type(self).__name__ + ".set_hyper", name, float(values[name]))
        row = self._rows[range(self.members)[p]]
        row.update({name: float(v) for name, v in values.items()})
        self._hyper_changed()

    @torch.no_grad()
    def copy_member(self, src, dst, hyper=False):
        """Member `dst` becomes a copy of member `src`: nets, targets and Adam moments -- and, with `hyper`, its hyper-parameters.
        The exploit step of population-based training; follow it with ``set_hyper(dst, ...)`` to explore."""
        src, dst = range(self.members)[src], range(self.members)[dst]
        for six in self.stacks.values():
            for t in six:
                t[dst].copy_(t[src])
        if hyper:
            self._rows[dst] = dict(self._rows[src])
            self._hyper_changed()

    def exploit(self, src, hyper=True):
        """The exploit step of population-based training for all members at once: member p becomes a copy of member ``src[p]`` --
        nets, targets and Adam moments, every tensor of ``stacks`` -- in ONE launch (armenv_pop_exploit) on the current stream, and,
        with `hyper`, takes its source's hyper-parameters.  ``src[p] == p`` keeps member p.  The plan is checked first and a bad one
        (a wrong length, an index that is no member's, a source that is itself replaced) raises ValueError with nothing moved.  The
        step counters are the population's and stay; a member keeps its own noise seed, ``seed + p``.  Follow with
        ``set_hyper(p, ...)`` on the replaced members to explore.  Returns the list of the replaced members."""
        who = type(self).__name__ + ".exploit"
        plan = check_plan(who, src, self.members)
        replaced = [p for p, v in enumerate(plan) if v != p]
        if not replaced:
            return replaced
        if self.device.type != "cuda":
            raise RuntimeError("%s: the stacks are on %s; armenv_pop_exploit copies on a HIP device" % (who, self.device))
        tensors = [t for six in self.stacks.values() for t in six]
        a = L.ArmEnvPopExploitArgs()
        a.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        a.members, a.tensors = self.members, len(tensors)
        src_c = (C.c_int32 * self.members)(*plan)
        base_c = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        elems_c = (C.c_int64 * len(tensors))(*[t[0].numel() for t in tensors])
        a.src, a.base, a.elems = src_c, base_c, elems_c
        L.check(L.load().armenv_pop_exploit(C.byref(a), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        if hyper:
            for p in replaced:
                self._rows[p] = dict(self._rows[plan[p]])
            self._hyper_changed()
        return replaced

    # ---- files and state (armenv.checkpoint)
    def save(self, filename):
        """every member p in the reference's files, as ``filename + ".m%d" % p``; returns the files written"""
        return [path for p in range(self.members) for path in self.member(p).save("%s.m%d" % (filename, p))]

    def load(self, filename):
        """every member p from the files ``filename + ".m%d" % p``"""
        for p in range(self.members):
            self.member(p).load("%s.m%d" % (filename, p))

    def _state_tensors(self):
        return self.stacks

    def _state_header(self):
        return dict(super()._state_header(), members=self.members)

    def state_dict(self):
        """FusedLearner.state_dict with ``stacks`` as the tensors, and the members' hyper-parameter rows"""
        return dict(super().state_dict(), rows=[dict(row) for row in self._rows])

    def _check_state(self, sd):
        super()._check_state(sd)
        who = type(self).__name__
        check_field(who, "rows", len(sd["rows"]), self.members)
        for p, row in enumerate(sd["rows"]):
            check_field(who, "rows[%d]" % p, sorted(row), sorted(self._rows[p]))
            for name, value in row.items():
                _check_range(who + ".load_state_dict", name, float(value))

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self._rows = [{name: float(value) for name, value in row.items()} for row in sd["rows"]]
        self._hyper_changed()

    def _bind(self, args):
        super()._bind(args)
        self._table = None
        if self.always_hyper or not self.uniform():
            self._table = (L.ArmEnvPopHyper * self.members)()
            for row, h in zip(self._rows, self._table):
                for name, _ in L.ArmEnvPopHyper._fields_:
                    setattr(h, name, row[name] if name in row else getattr(self, name, 0.0))   # not the agent's: never read
        self._bound_fn = getattr(L.load(), self.entry_point)

    def _enqueue(self, stream):
        if self._table is None:
            return self._bound_fn(C.byref(self._args), stream)
        return self._bound_fn(C.byref(self._args), self._table, stream)

    def _create(self, members, seed, device):
        """Creates the stacks and the members: member p from the nets of ``torch.manual_seed(seed + p); _single("cpu", seed + p)``.
        The nets are created on the host, where torch's initialisers draw from the CPU generator whatever the device; the global
        generators are left as found."""
        if not 1 <= int(members) <= MAX_MEMBERS:
            raise ValueError("%s: members must be 1..%d" % (type(self).__name__, MAX_MEMBERS))
        self.members, self.device, self.seed = int(members), torch.device(device), int(seed)
        self._lead = (self.members,)
        cuda = range(torch.cuda.device_count()) if torch.cuda.is_available() and torch.cuda.is_initialized() else []
        agents = []
        with torch.random.fork_rng(devices=list(cuda)):
            for p in range(self.members):
                torch.manual_seed(self.seed + p)
                agents.append(self._single("cpu", self.seed + p, p))
        # stacks[name]: six tensors [P][rows][cols] (W1, b1, W2, b2, W3, b3) of net or moment `name`
        self.stacks = {}
        for name, six in zip(self._NETS, self._sixes(agents[0])):
            self.stacks[name] = [torch.empty((self.members,) + tuple(t.shape), dtype=torch.float32, device=self.device) for t in six]
        for name, net in self._MOMENTS:
            self.stacks[name] = [torch.zeros_like(t) for t in self.stacks[net]]
        self._members = []
        with torch.no_grad():
            for p, agent in enumerate(agents):
                for name, six in zip(self._NETS, self._sixes(agent)):
                    for t, stack in zip(six, self.stacks[name]):
                        stack[p].copy_(t)
                        t.data = stack[p]              # the module's parameter becomes the view
                self._members.append(self._member_of(p, agent))
        self._batch = None

    @staticmethod
    def _sixes(agent):
        """the parameters of a single learner's nets, six per entry of _NETS"""
        return tuple(list(net.parameters()) for net in agent._nets())

    def _member_of(self, p, agent):
        raise NotImplementedError

    def member(self, p):
        return self._members[p]

    def batch_buffers(self, batch_size):
        """the stacked static inputs [P][B][...] of one update; ``member_buffers(p)`` are member p's slices of them"""
        B, D, P, dev = int(batch_size), self.state_dim, self.members, self.device
        self._batch = dict(states=torch.zeros(P, B, D, device=dev), actions=torch.zeros(P, B, self.action_dim, device=dev),
                           next_states=torch.zeros(P, B, D, device=dev), rewards=torch.zeros(P, B, device=dev),
                           dones=torch.zeros(P, B, dtype=torch.uint8, device=dev))
        return self._batch

    def member_buffers(self, p):
        """member p's contiguous slices of the last ``batch_buffers``: the dict that ``TrajectoryStore.sample(out=...)`` fills"""
        if self._batch is None:
            raise RuntimeError("%s.member_buffers: call batch_buffers(batch_size) first" % type(self).__name__)
        return {k: t[p] for k, t in self._batch.items()}

    def _static_args(self):
        a = self._PopArgs()
        a.members = self.members
        one = super()._static_args()
        for name in self.stacks:
            setattr(one, name, _mlp_of(self.stacks[name]))
        a.one = one
        return a

    def _inputs(self, batch):
        """(states, actions, rewards, next_states, dones) of a stacked batch dict as the contiguous tensors the update reads"""
        P, dev = self.members, self.device
        f32 = lambda k: batch[k].to(dev, torch.float32).contiguous()
        s, a, s2 = f32("states"), f32("actions"), f32("next_states")
        if s.dim() != 3 or s.shape[0] != P or s.shape[2] != self.state_dim or a.shape != s.shape[:2] + (self.action_dim,) or s2.shape != s.shape:
            raise ValueError("%s.train: states / next_states must be [P][B][state_dim] and actions [P][B][action_dim]" % type(self).__name__)
        B = s.shape[1]
        r = batch["rewards"].to(dev, torch.float32).reshape(P, B).contiguous()
        d = batch["dones"].to(dev)
        d = (d if d.dtype == torch.uint8 else (d != 0).to(torch.uint8)).reshape(P, B).contiguous()
        return s, a, r, s2, d

    @staticmethod
    def _per_call_struct(args):
        return args.one

    def _member_state(self, p):
        """member p's parameters and moments as views, six per stack, in _NETS + _MOMENTS order"""
        return [t[p] for name in self._NETS + tuple(m for m, _ in self._MOMENTS) for t in self.stacks[name]]

    @classmethod
    def _single_state(cls, agent):
        """the same tensors of a single learner"""
        nets = [t for six in cls._sixes(agent) for t in six]
        return nets + [t for m, _ in cls._MOMENTS for t in getattr(agent, m)]

    def _single(self, device, seed, p):
        """a single learner with member p's hyper-parameters, and `seed` where the agent takes one"""
        kw = {name: self._rows[p][name] if name in self._rows[p] else getattr(self, name) for name in self._HYPER_KW}
        if self._takes_seed:
            kw["seed"] = seed
        return self._Single(self.state_dim, self.action_dim, self.action_bound, device=device, **kw)

    @torch.no_grad()
    def load_member(self, p, agent):
        """Copies a single learner's whole state into member p: parameters, targets, moments -- and its counters (total_it and the
        Adam step numbers), which are the population's: load every member from learners at the same step.  The member keeps its
        hyper-parameters."""
        for mine, theirs in zip(self._member_state(p), self._single_state(agent)):
            mine.copy_(theirs)
        for name in self._COUNTERS:
            setattr(self, name, getattr(agent, name))

    @torch.no_grad()
    def export_member(self, p):
        """a single learner on this device with member p's hyper-parameters, holding member p's whole state, counters and noise seed
        (``seed + p``) included: its ``train`` on member p's batch does what the population's does to member p"""
        p = range(self.members)[p]
        with torch.random.fork_rng(devices=[]):         # its initial weights are overwritten: leave the generator alone
            agent = self._single(self.device, self.seed + p, p)
        for theirs, mine in zip(self._single_state(agent), self._member_state(p)):
            theirs.copy_(mine)
        for name in self._COUNTERS:
            setattr(agent, name, getattr(self, name))
        return agent
