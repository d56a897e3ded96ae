"""Populations of independent DATD3 and DARC learners updated by ONE fused HIP update (armenv_datd3_pop_update, include/armenv.h;
kernels in csrc/armenv_learner_kernels.inc): the 16 kernel launches of one FusedDATD3 / FusedDARC update, each over P times the
workgroups.  ``train`` is the reference's: update k = 1, then update k = 2, on the same stacked batch.

Members share the step schedule (total_it, the four Adam step numbers) and, unless given their own, the hyper-parameters:
``actor_lr``, ``critic_lr``, ``tau``, ``gamma``, ``policy_noise``, ``noise_clip`` and DARC's ``q_weight`` and
``regularization_weight`` each take one value or a sequence of P (fused_pop_base; armenv_datd3_pop_update_hyper then runs the update).
Every parameter, target and Adam-moment tensor is member 0's slice of a stack [P][rows][cols] that this object owns; member p's
update equals, bit for bit, FusedDATD3's / FusedDARC's with member p's hyper-parameters on the same state with seed ``seed + p``."""
from . import _lib as L
from .fused_datd3 import DARCSchedule, DATD3Schedule, FusedDARC, FusedDATD3
from .fused_pop_base import FusedPopulation, TwoActorMember

_LEARNING = ("actor1", "actor2", "critic1", "critic2")
_NETS = _LEARNING + tuple("target_" + n for n in _LEARNING)


class FusedDATD3Population(DATD3Schedule, FusedPopulation):
    """``members`` DATD3 agents with FusedDATD3's hyper-parameters, each one value or P values.  Member p starts from the weights that
    ``torch.manual_seed(seed + p); FusedDATD3(...)`` creates and draws its target-policy noise with seed ``seed + p``; the constructor
    leaves the global random generators as it found them."""

    _fn, _PopArgs, _Single = "datd3_pop", L.ArmEnvDatd3PopArgs, FusedDATD3
    _NETS = _NETS
    _MOMENTS = tuple((n + sfx, n) for n in _LEARNING for sfx in ("_m", "_v"))

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0", seed=0, **darc):
        self._configure_members(members, state_dim, action_dim, action_bound, hidden_dim=hidden_dim, actor_lr=actor_lr,
                                critic_lr=critic_lr, tau=tau, gamma=gamma, policy_noise=policy_noise, noise_clip=noise_clip,
                                policy_freq=policy_freq, **darc)
        self._create(members, seed, device)

    def _member_of(self, p, agent):
        return TwoActorMember(p, self.device, _NETS, agent._nets(), ("critic1", "critic2"))

    def _static_args(self):
        a = super()._static_args()
        a.one.darc = self._darc
        return a


class FusedDARCPopulation(DARCSchedule, FusedDATD3Population):
    """``members`` DARC agents with FusedDARC's hyper-parameters and defaults: the same call with `darc` = 1."""

    _Single = FusedDARC

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, q_weight=0.2, regularization_weight=0.005,
                 device="cuda:0", seed=0):
        super().__init__(members, state_dim, action_dim, action_bound, hidden_dim, actor_lr, critic_lr, tau, gamma, policy_noise,
                         noise_clip, policy_freq, device, seed, q_weight=q_weight, regularization_weight=regularization_weight)
