"""A population of independent TD3 learners updated by ONE fused HIP update (armenv_td3_pop_update, include/armenv.h; kernels in
csrc/armenv_learner_kernels.inc): as many kernel launches as one FusedTD3 update -- 9, 16 with the delayed actor step -- each over
P times the workgroups.  At the reference's batch of 256 one learner leaves the device nearly idle; a seed sweep of P learners costs
about what one does.

Members share the hyper-parameters and the step schedule (total_it, the Adam step numbers, policy_freq) and nothing else.  Every
parameter, target and Adam-moment tensor is member 0's slice of a stack [P][rows][cols] that this object owns; member p's update
equals, bit for bit, FusedTD3's on the same state with seed ``seed + p``."""
import ctypes as C

import torch

from . import _lib as L
from .fused_base import FusedLearner, _mlp_of
from .fused_td3 import FusedTD3

_NETS = ("actor", "q1", "q2", "target_actor", "target_q1", "target_q2")
_MOMENTS = ("actor_m", "actor_v", "q1_m", "q1_v", "q2_m", "q2_v")
MAX_MEMBERS = 64


def _six(net, half=0):
    """the six parameters W1, b1, W2, b2, W3, b3 of an Actor (half 0), or of Q1 (0) / Q2 (1) of a TwinCritic"""
    return list(net.parameters())[6 * half:6 * half + 6]


class Member:
    """Member p of a FusedTD3Population: the ``actor`` / ``critic`` / ``target_actor`` / ``target_critic`` modules of a TD3 agent
    whose parameters are views into the population's stacks (what the update writes, they show; what is written through them, the
    update reads)."""

    def __init__(self, index, device, nets):
        self.index, self.device = index, device
        self.actor, self.critic, self.target_actor, self.target_critic = nets

    def actor_state_dict(self):
        return {k: v.detach() for k, v in self.actor.state_dict().items()}

    def take_action(self, state):
        """TD3_MLP.take_action, as FusedTD3.take_action"""
        import numpy as np
        with torch.no_grad():
            s = torch.tensor(np.asarray([state], dtype=np.float32), device=self.device)
            return self.actor(s).detach().cpu().numpy()[0]


class FusedTD3Population(FusedLearner):
    """``members`` TD3 agents with FusedTD3's hyper-parameters.  Member p starts from the weights that
    ``torch.manual_seed(seed + p); FusedTD3(...)`` creates and draws its target-policy noise with seed ``seed + p``; the constructor
    leaves the global random generators as it found them."""

    _fn, _Args = "td3_pop", L.ArmEnvTd3Args
    _hyper = ("policy_noise", "noise_clip", "seed")

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0", seed=0):
        self._check_shapes(state_dim, action_dim, hidden_dim)
        if not 1 <= int(members) <= MAX_MEMBERS:
            raise ValueError("FusedTD3Population: members must be 1..%d" % MAX_MEMBERS)
        self.members, self.device, self.seed = int(members), torch.device(device), int(seed)
        self.state_dim, self.action_dim, self.hidden_dim = state_dim, action_dim, hidden_dim
        self.actor_lr, self.critic_lr, self.tau, self.gamma, self.action_bound = actor_lr, critic_lr, tau, gamma, action_bound
        self.policy_noise, self.noise_clip, self.policy_freq = policy_noise, noise_clip, policy_freq
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self._kw = dict(hidden_dim=hidden_dim, actor_lr=actor_lr, critic_lr=critic_lr, tau=tau, gamma=gamma, policy_noise=policy_noise,
                        noise_clip=noise_clip, policy_freq=policy_freq)
        # the nets are created on the host, where torch's initialisers draw from the CPU generator whatever the device
        cuda = range(torch.cuda.device_count()) if torch.cuda.is_available() and torch.cuda.is_initialized() else []
        agents = []
        with torch.random.fork_rng(devices=list(cuda)):
            for p in range(self.members):
                torch.manual_seed(self.seed + p)
                agents.append(FusedTD3(state_dim, action_dim, action_bound, device="cpu", seed=self.seed + p, **self._kw))
        # stacks[name]: six tensors [P][rows][cols] (W1, b1, W2, b2, W3, b3) of net or moment `name`
        self.stacks = {}
        for name, six in zip(_NETS, self._sixes(agents[0])):
            self.stacks[name] = [torch.empty((self.members,) + tuple(t.shape), dtype=torch.float32, device=self.device) for t in six]
        for name, net in zip(_MOMENTS, ("actor", "actor", "q1", "q1", "q2", "q2")):
            self.stacks[name] = [torch.zeros_like(t) for t in self.stacks[net]]
        self._members = []
        with torch.no_grad():
            for p, agent in enumerate(agents):
                for name, six in zip(_NETS, self._sixes(agent)):
                    for t, stack in zip(six, self.stacks[name]):
                        stack[p].copy_(t)
                        t.data = stack[p]              # the module's parameter becomes the view
                self._members.append(Member(p, self.device, agent._nets()))
        self.actor_step = self.critic_step = 0
        self.total_it = 0
        self._ws = self._args = self._batch = None

    @staticmethod
    def _sixes(agent):
        """the parameters of a FusedTD3's nets in _NETS order"""
        return (_six(agent.actor), _six(agent.critic, 0), _six(agent.critic, 1),
                _six(agent.target_actor), _six(agent.target_critic, 0), _six(agent.target_critic, 1))

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
            raise RuntimeError("FusedTD3Population.member_buffers: call batch_buffers(batch_size) first")
        return {k: t[p] for k, t in self._batch.items()}

    def _static_args(self):
        a = L.ArmEnvTd3PopArgs()
        a.members = self.members
        one = super()._static_args()
        for name in _NETS + _MOMENTS:
            setattr(one, name, _mlp_of(self.stacks[name]))
        a.one = one
        return a

    def train(self, batch, noise=None):
        """One update of every member from a dict of stacked device tensors: states [P,B,D], actions [P,B,3], next_states [P,B,D],
        rewards [P,B], dones [P,B] (any dtype).  `noise` (optional): [P,B,3] standard normals for the target-policy noise.  Returns
        the critic losses [P] (no host sync)."""
        P, dev = self.members, self.device
        f32 = lambda k: batch[k].to(dev, torch.float32).contiguous()
        s, a, s2 = f32("states"), f32("actions"), f32("next_states")
        if s.dim() != 3 or s.shape[0] != P or s.shape[2] != self.state_dim or a.shape != s.shape[:2] + (self.action_dim,) or s2.shape != s.shape:
            raise ValueError("FusedTD3Population.train: states / next_states must be [P][B][state_dim] and actions [P][B][action_dim]")
        B = s.shape[1]
        r = batch["rewards"].to(dev, torch.float32).reshape(P, B).contiguous()
        d = batch["dones"].to(dev)
        d = (d if d.dtype == torch.uint8 else (d != 0).to(torch.uint8)).reshape(P, B).contiguous()
        if noise is not None:
            noise = noise.to(dev, torch.float32).contiguous()
            if tuple(noise.shape) != (P, B, self.action_dim):
                raise ValueError("noise must be [P][B][%d] standard normals" % self.action_dim)
        lib = L.load()
        n = lib.armenv_td3_pop_workspace_bytes(self.state_dim, self.hidden_dim, B, P)
        if n < 0:
            raise ValueError("FusedTD3Population: unsupported batch size %d" % B)
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=torch.uint8, device=dev)
        if self._args is None:
            self._args = self._static_args()
        self.total_it += 1
        with_actor = self.total_it % self.policy_freq == 0
        loss = torch.empty(P, dtype=torch.float32, device=dev)
        one = self._args.one
        one.batch, one.with_actor, one.draw = B, int(with_actor), self.total_it
        one.critic_step, one.actor_step = self.critic_step + 1, self.actor_step + 1 if with_actor else 0
        one.noise_dev = noise.data_ptr() if noise is not None else None
        one.states_dev, one.actions_dev, one.next_states_dev = s.data_ptr(), a.data_ptr(), s2.data_ptr()
        one.rewards_dev, one.dones_dev, one.loss_dev = r.data_ptr(), d.data_ptr(), loss.data_ptr()
        one.workspace_dev, one.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        L.check(lib.armenv_td3_pop_update(C.byref(self._args), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self.critic_step += 1
        if with_actor:
            self.actor_step += 1
        return loss

    def _member_state(self, p):
        """member p's (parameters and moments) as 72 views, in _NETS + _MOMENTS order"""
        return [t[p] for name in _NETS + _MOMENTS for t in self.stacks[name]]

    @staticmethod
    def _single_state(agent):
        """the same 72 tensors of a FusedTD3"""
        nets = [t for six in FusedTD3Population._sixes(agent) for t in six]
        return nets + agent.actor_m + agent.actor_v + agent.critic_m[:6] + agent.critic_v[:6] + agent.critic_m[6:] + agent.critic_v[6:]

    @torch.no_grad()
    def load_member(self, p, agent):
        """Copies a FusedTD3's whole state into member p: parameters, targets, moments -- and its counters (total_it and the Adam
        step numbers), which are the population's: load every member from learners at the same step."""
        for mine, theirs in zip(self._member_state(p), self._single_state(agent)):
            mine.copy_(theirs)
        self.total_it, self.critic_step, self.actor_step = agent.total_it, agent.critic_step, agent.actor_step

    @torch.no_grad()
    def export_member(self, p):
        """a FusedTD3 on this device holding member p's whole state, counters and noise seed (``seed + p``) included"""
        with torch.random.fork_rng(devices=[]):         # its initial weights are overwritten: leave the generator alone
            agent = FusedTD3(self.state_dim, self.action_dim, self.action_bound, device=self.device, seed=self.seed + p, **self._kw)
        for theirs, mine in zip(self._single_state(agent), self._member_state(p)):
            theirs.copy_(mine)
        agent.total_it, agent.critic_step, agent.actor_step = self.total_it, self.critic_step, self.actor_step
        return agent
