"""A population of independent TD3 learners updated by ONE fused HIP update (armenv_td3_pop_update, include/armenv.h; kernels in
csrc/armenv_learner_kernels.inc): as many kernel launches as one FusedTD3 update -- 9, 16 with the delayed actor step -- each over
P times the workgroups.  At the reference's batch of 256 one learner leaves the device nearly idle; a seed sweep of P learners costs
about what one does.

Members share the hyper-parameters and the step schedule (total_it, the Adam step numbers, policy_freq) and nothing else.  Every
parameter, target and Adam-moment tensor is member 0's slice of a stack [P][rows][cols] that this object owns; member p's update
equals, bit for bit, FusedTD3's on the same state with seed ``seed + p``."""
import torch

from . import _lib as L
from .fused_pop_base import MAX_MEMBERS, FusedPopulation  # noqa: F401  (MAX_MEMBERS: importable from here as before)
from .fused_td3 import FusedTD3

_NETS = ("actor", "q1", "q2", "target_actor", "target_q1", "target_q2")
_MOMENTS = ("actor_m", "actor_v", "q1_m", "q1_v", "q2_m", "q2_v")


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


class FusedTD3Population(FusedPopulation):
    """``members`` TD3 agents with FusedTD3's hyper-parameters.  Member p starts from the weights that
    ``torch.manual_seed(seed + p); FusedTD3(...)`` creates and draws its target-policy noise with seed ``seed + p``; the constructor
    leaves the global random generators as it found them."""

    _fn, _Args, _PopArgs, _Single = "td3_pop", L.ArmEnvTd3Args, L.ArmEnvTd3PopArgs, FusedTD3
    _hyper = ("policy_noise", "noise_clip", "seed")
    _NETS = _NETS
    _MOMENTS = tuple(zip(_MOMENTS, ("actor", "actor", "q1", "q1", "q2", "q2")))
    _COUNTERS = ("total_it", "critic_step", "actor_step")

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0", seed=0):
        self._check_shapes(state_dim, action_dim, hidden_dim)
        self.state_dim, self.action_dim, self.hidden_dim = state_dim, action_dim, hidden_dim
        self.actor_lr, self.critic_lr, self.tau, self.gamma, self.action_bound = actor_lr, critic_lr, tau, gamma, action_bound
        self.policy_noise, self.noise_clip, self.policy_freq = policy_noise, noise_clip, policy_freq
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self._kw = dict(hidden_dim=hidden_dim, actor_lr=actor_lr, critic_lr=critic_lr, tau=tau, gamma=gamma, policy_noise=policy_noise,
                        noise_clip=noise_clip, policy_freq=policy_freq)
        self._create(members, seed, device, self._single)

    def _single(self, device, seed):
        return FusedTD3(self.state_dim, self.action_dim, self.action_bound, device=device, seed=seed, **self._kw)

    @staticmethod
    def _sixes(agent):
        """the parameters of a FusedTD3's nets in _NETS order"""
        return (_six(agent.actor), _six(agent.critic, 0), _six(agent.critic, 1),
                _six(agent.target_actor), _six(agent.target_critic, 0), _six(agent.target_critic, 1))

    def _member_of(self, p, agent):
        return Member(p, self.device, agent._nets())

    def train(self, batch, noise=None):
        """One update of every member from a dict of stacked device tensors: states [P,B,D], actions [P,B,3], next_states [P,B,D],
        rewards [P,B], dones [P,B] (any dtype).  `noise` (optional): [P,B,3] standard normals for the target-policy noise.  Returns
        the critic losses [P] (no host sync)."""
        inputs = self._inputs(batch)
        noise = self._noise(noise, inputs[0].shape[1])
        self._workspace(inputs[0].shape[1])             # an unsupported batch size is refused before the counters move
        self.total_it += 1
        with_actor = self.total_it % self.policy_freq == 0
        loss = self._call(*inputs, noise, with_actor=int(with_actor), draw=self.total_it, critic_step=self.critic_step + 1,
                          actor_step=self.actor_step + 1 if with_actor else 0)
        self.critic_step += 1
        if with_actor:
            self.actor_step += 1
        return loss

    @staticmethod
    def _single_state(agent):
        """the same 72 tensors of a FusedTD3"""
        nets = [t for six in FusedTD3Population._sixes(agent) for t in six]
        return nets + agent.actor_m + agent.actor_v + agent.critic_m[:6] + agent.critic_v[:6] + agent.critic_m[6:] + agent.critic_v[6:]
