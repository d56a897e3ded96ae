"""A population of independent DADDPG learners -- the reference's default agent -- updated by ONE fused HIP update
(armenv_daddpg_pop_update, include/armenv.h; kernels in csrc/armenv_learner_kernels.inc): the 16 kernel launches of one FusedDADDPG
update, each over P times the workgroups.  At the reference's batch of 256 one learner leaves the device nearly idle; a seed sweep of
P learners costs about what one does.

Members share the hyper-parameters and the step schedule (total_it, so which actor is stepped, and the three Adam step numbers) and
nothing else.  Every parameter, target and Adam-moment tensor is member 0's slice of a stack [P][rows][cols] that this object owns;
member p's update equals, bit for bit, FusedDADDPG's on the same state."""
from . import _lib as L
from .fused_daddpg import FusedDADDPG
from .fused_pop_base import FusedPopulation, TwoActorMember

_NETS = ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic")
_LEARNING = ("actor1", "actor2", "critic")


class FusedDADDPGPopulation(FusedPopulation):
    """``members`` DADDPG agents with FusedDADDPG's hyper-parameters.  Member p starts from the weights that
    ``torch.manual_seed(seed + p); FusedDADDPG(...)`` creates; the constructor leaves the global random generators as it found them."""

    _fn, _Args, _PopArgs, _Single = "daddpg_pop", L.ArmEnvDaddpgArgs, L.ArmEnvDaddpgPopArgs, FusedDADDPG
    _NETS = _NETS
    _MOMENTS = tuple((n + sfx, n) for n in _LEARNING for sfx in ("_m", "_v"))
    _COUNTERS = ("total_it", "critic_step", "actor1_step", "actor2_step")

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, device="cuda:0", seed=0):
        self._check_shapes(state_dim, action_dim, hidden_dim)
        self.state_dim, self.action_dim, self.hidden_dim = state_dim, action_dim, hidden_dim
        self.actor_lr, self.critic_lr, self.tau, self.gamma, self.action_bound = actor_lr, critic_lr, tau, gamma, action_bound
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self._kw = dict(hidden_dim=hidden_dim, actor_lr=actor_lr, critic_lr=critic_lr, tau=tau, gamma=gamma)
        self._create(members, seed, device, self._single)

    def _single(self, device, seed):
        return FusedDADDPG(self.state_dim, self.action_dim, self.action_bound, device=device, **self._kw)

    def _member_of(self, p, agent):
        return TwoActorMember(p, self.device, _NETS, agent._nets(), ("critic", "critic"))

    def train(self, batch):
        """One update of every member from a dict of stacked device tensors: states [P,B,D], actions [P,B,3], next_states [P,B,D],
        rewards [P,B], dones [P,B] (any dtype).  The actor alternation and the step counters are FusedDADDPG.train's.  Returns the
        critic losses [P] (no host sync)."""
        inputs = self._inputs(batch)
        self._workspace(inputs[0].shape[1])             # an unsupported batch size is refused before the counters move
        self.total_it += 1
        update_a1 = self.total_it % 2 == 0                        # DADDPG_mlp.py:119
        loss = self._call(*inputs, critic_step=self.critic_step + 1, update_actor=1 if update_a1 else 2,
                          actor_step=(self.actor1_step if update_a1 else self.actor2_step) + 1)
        self.critic_step += 1
        if update_a1:
            self.actor1_step += 1
        else:
            self.actor2_step += 1
        return loss
