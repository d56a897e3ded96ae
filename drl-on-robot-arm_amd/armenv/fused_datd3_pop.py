"""Populations of independent DATD3 and DARC learners updated by ONE fused HIP update (armenv_datd3_pop_update, include/armenv.h;
kernels in csrc/armenv_learner_kernels.inc): the 16 kernel launches of one FusedDATD3 / FusedDARC update, each over P times the
workgroups.  ``train`` is the reference's: update k = 1, then update k = 2, on the same stacked batch.

Members share the hyper-parameters and the step schedule (total_it, the four Adam step numbers) and nothing else.  Every parameter,
target and Adam-moment tensor is member 0's slice of a stack [P][rows][cols] that this object owns; member p's update equals, bit
for bit, FusedDATD3's / FusedDARC's on the same state with seed ``seed + p``."""
from . import _lib as L
from .fused_datd3 import FusedDARC, FusedDATD3
from .fused_pop_base import FusedPopulation, TwoActorMember

_LEARNING = ("actor1", "actor2", "critic1", "critic2")
_NETS = _LEARNING + tuple("target_" + n for n in _LEARNING)


class FusedDATD3Population(FusedPopulation):
    """``members`` DATD3 agents with FusedDATD3's hyper-parameters.  Member p starts from the weights that
    ``torch.manual_seed(seed + p); FusedDATD3(...)`` creates and draws its target-policy noise with seed ``seed + p``; the constructor
    leaves the global random generators as it found them."""

    _darc = 0
    _fn, _Args, _PopArgs, _Single = "datd3_pop", L.ArmEnvDatd3Args, L.ArmEnvDatd3PopArgs, FusedDATD3
    _hyper = ("policy_noise", "noise_clip", "seed", "q_weight", "regularization_weight")
    _NETS = _NETS
    _MOMENTS = tuple((n + sfx, n) for n in _LEARNING for sfx in ("_m", "_v"))
    _COUNTERS = ("total_it",) + tuple(n + "_step" for n in _LEARNING)

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0", seed=0, **darc):
        self._check_shapes(state_dim, action_dim, hidden_dim)
        self.state_dim, self.action_dim, self.hidden_dim = state_dim, action_dim, hidden_dim
        self.actor_lr, self.critic_lr, self.tau, self.gamma, self.action_bound = actor_lr, critic_lr, tau, gamma, action_bound
        self.policy_noise, self.noise_clip, self.policy_freq = policy_noise, noise_clip, policy_freq     # policy_freq: never read
        self.q_weight, self.regularization_weight = darc.get("q_weight", 0.0), darc.get("regularization_weight", 0.0)
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self._kw = dict(hidden_dim=hidden_dim, actor_lr=actor_lr, critic_lr=critic_lr, tau=tau, gamma=gamma, policy_noise=policy_noise,
                        noise_clip=noise_clip, policy_freq=policy_freq, **darc)
        self._create(members, seed, device, self._single)

    def _single(self, device, seed):
        return self._Single(self.state_dim, self.action_dim, self.action_bound, device=device, seed=seed, **self._kw)

    def _member_of(self, p, agent):
        return TwoActorMember(p, self.device, _NETS, agent._nets(), ("critic1", "critic2"))

    def _static_args(self):
        a = super()._static_args()
        a.one.darc = self._darc
        return a

    def _update(self, s, a, r, s2, d, update_a1, noise=None):
        """one armenv_datd3_pop_update over prepared tensors; its `draw` is the update's number"""
        noise = self._noise(noise, s.shape[1])
        self._workspace(s.shape[1])                     # an unsupported batch size is refused before the counters move
        self.total_it += 1
        k = 1 if update_a1 else 2
        steps = dict(critic_step=getattr(self, "critic%d_step" % k) + 1, actor_step=getattr(self, "actor%d_step" % k) + 1)
        loss = self._call(s, a, r, s2, d, noise, update_actor=k, draw=self.total_it, **steps)
        setattr(self, "critic%d_step" % k, steps["critic_step"])
        setattr(self, "actor%d_step" % k, steps["actor_step"])
        return loss

    def update(self, batch, update_a1=True, noise=None):
        """One update of every member (the reference's `update(transition_dict, update_a1)`) from a dict of stacked device tensors;
        `noise` (optional): [P,B,3] standard normals.  Returns the stepped critics' losses [P] (no host sync)."""
        return self._update(*self._inputs(batch), update_a1, noise)

    def train(self, batch, noise=None):
        """The reference's `train` for every member from a dict of stacked device tensors (states [P,B,D], actions [P,B,3],
        next_states [P,B,D], rewards [P,B], dones [P,B], any dtype): update k = 1 then update k = 2 on the same batch, with
        consecutive `draw`s.  `noise` (optional): a pair of [P,B,3] tensors of standard normals, one per update.  Returns the two
        loss tensors [P] (no host sync); total_it counts updates."""
        inputs = self._inputs(batch)
        n1, n2 = (None, None) if noise is None else noise
        return self._update(*inputs, True, n1), self._update(*inputs, False, n2)


class FusedDARCPopulation(FusedDATD3Population):
    """``members`` DARC agents with FusedDARC's hyper-parameters and defaults: the same call with `darc` = 1."""

    _darc = 1
    _Single = FusedDARC

    def __init__(self, members, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, q_weight=0.2, regularization_weight=0.005,
                 device="cuda:0", seed=0):
        super().__init__(members, state_dim, action_dim, action_bound, hidden_dim, actor_lr, critic_lr, tau, gamma, policy_noise,
                         noise_clip, policy_freq, device, seed, q_weight=q_weight, regularization_weight=regularization_weight)
