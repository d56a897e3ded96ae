"""A population of independent DADDPG learners -- the reference's default agent -- updated by ONE fused HIP update
(armenv_daddpg_pop_update, include/armenv.h; kernels in csrc/armenv_learner_kernels.inc): the 16 kernel launches of one FusedDADDPG
update, each over P times the workgroups.  At the reference's batch of 256 one learner leaves the device nearly idle; a seed sweep of
P learners costs about what one does.

Members share the step schedule (total_it, so which actor is stepped, and the three Adam step numbers) and, unless given their own,
the hyper-parameters: ``actor_lr``, ``critic_lr``, ``tau`` and ``gamma`` each take one value or a sequence of P (fused_pop_base;
armenv_daddpg_pop_update_hyper then runs the update).  Every parameter, target and Adam-moment tensor is member 0's slice of a stack
[P][rows][cols] that this object owns; member p's update equals, bit for bit, FusedDADDPG's with member p's hyper-parameters on the
same state."""
from . import _lib as L
from .fused_daddpg import DADDPGSchedule, FusedDADDPG
from .fused_pop_base import FusedPopulation, TwoActorMember

_NETS = ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic")
_LEARNING = ("actor1", "actor2", "critic")


class FusedDADDPGPopulation(DADDPGSchedule, FusedPopulation):
    """``members`` DADDPG agents with FusedDADDPG's hyper-parameters, each one value or P values.  Member p starts from the weights that
    ``torch.manual_seed(seed + p); FusedDADDPG(...)`` creates; the constructor leaves the global random generators as it found them."""

    _fn, _PopArgs, _Single = "daddpg_pop", L.ArmEnvDaddpgPopArgs, FusedDADDPG
    _NETS = _NETS
    _MOMENTS = tuple((n + sfx, n) for n in _LEARNING for sfx in ("_m", "_v"))

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, device="cuda:0", seed=0):
        self._configure_members(members, state_dim, action_dim, action_bound, hidden_dim=hidden_dim, actor_lr=actor_lr,
                                critic_lr=critic_lr, tau=tau, gamma=gamma)
        self._create(members, seed, device)

    def _member_of(self, p, agent):
        return TwoActorMember(p, self.device, _NETS, agent._nets(), ("critic", "critic"))
