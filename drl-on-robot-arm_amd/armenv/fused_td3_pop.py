"""A population of independent TD3 learners updated by ONE fused HIP update (armenv_td3_pop_update, include/armenv.h; kernels in
csrc/armenv_learner_kernels.inc): as many kernel launches as one FusedTD3 update -- 9, 16 with the delayed actor step -- each over
P times the workgroups.  At the reference's batch of 256 one learner leaves the device nearly idle; a seed sweep of P learners costs
about what one does.

Members share the step schedule (total_it, the Adam step numbers, policy_freq) and, unless given their own, the hyper-parameters:
``actor_lr``, ``critic_lr``, ``tau``, ``gamma``, ``policy_noise`` and ``noise_clip`` each take one value or a sequence of P
(fused_pop_base; armenv_td3_pop_update_hyper then runs the update).  Every parameter, target and Adam-moment tensor is member 0's
slice of a stack [P][rows][cols] that this object owns; member p's update equals, bit for bit, FusedTD3's with member p's
hyper-parameters on the same state with seed ``seed + p``."""
from . import _lib as L
from .checkpoint import AgentFiles
from .fused_pop_base import MAX_MEMBERS, FusedPopulation  # noqa: F401  (MAX_MEMBERS: importable from here as before)
from .fused_td3 import FusedTD3, TD3Schedule

_NETS = ("actor", "q1", "q2", "target_actor", "target_q1", "target_q2")
_MOMENTS = ("actor_m", "actor_v", "q1_m", "q1_v", "q2_m", "q2_v")


def _six(net, half=0):
    """the six parameters W1, b1, W2, b2, W3, b3 of an Actor (half 0), or of Q1 (0) / Q2 (1) of a TwinCritic"""
    return list(net.parameters())[6 * half:6 * half + 6]


class Member(AgentFiles):
    """Member p of a FusedTD3Population: the ``actor`` / ``critic`` / ``target_actor`` / ``target_critic`` modules of a TD3 agent
    whose parameters are views into the population's stacks (what the update writes, they show; what is written through them, the
    update reads); ``save`` / ``load`` as FusedTD3's, through the views."""

    def __init__(self, index, device, nets):
        self.index, self.device = index, device
        self.actor, self.critic, self.target_actor, self.target_critic = nets

    take_action, actor_state_dict = FusedTD3.take_action, FusedTD3.actor_state_dict


class FusedTD3Population(TD3Schedule, FusedPopulation):
    """``members`` TD3 agents with FusedTD3's hyper-parameters, each one value or P values.  Member p starts from the weights that
    ``torch.manual_seed(seed + p); FusedTD3(...)`` creates and draws its target-policy noise with seed ``seed + p``; the constructor
    leaves the global random generators as it found them."""

    _fn, _PopArgs, _Single = "td3_pop", L.ArmEnvTd3PopArgs, FusedTD3
    _NETS = _NETS
    _MOMENTS = tuple(zip(_MOMENTS, ("actor", "actor", "q1", "q1", "q2", "q2")))

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0", seed=0):
        self._configure_members(members, state_dim, action_dim, action_bound, hidden_dim=hidden_dim, actor_lr=actor_lr,
                                critic_lr=critic_lr, tau=tau, gamma=gamma, policy_noise=policy_noise, noise_clip=noise_clip,
                                policy_freq=policy_freq)
        self._create(members, seed, device)

    @staticmethod
    def _sixes(agent):
        """the parameters of a FusedTD3's nets in _NETS order"""
        return (_six(agent.actor), _six(agent.critic, 0), _six(agent.critic, 1),
                _six(agent.target_actor), _six(agent.target_critic, 0), _six(agent.target_critic, 1))

    def _member_of(self, p, agent):
        return Member(p, self.device, agent._nets())

    @staticmethod
    def _single_state(agent):
        """the same 72 tensors of a FusedTD3"""
        nets = [t for six in FusedTD3Population._sixes(agent) for t in six]
        return nets + agent.actor_m + agent.actor_v + agent.critic_m[:6] + agent.critic_v[:6] + agent.critic_m[6:] + agent.critic_v[6:]
