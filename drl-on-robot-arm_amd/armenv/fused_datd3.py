"""DATD3 and DARC learners whose update is the fused HIP update of libarmenv.so (armenv_datd3_update, include/armenv.h; kernels in
csrc/armenv_learner.h): ONE DATD3_MLP.update / DARC_MLP.update (the reference's algo/DATD3/DATD3_mlp.py:146-211,
algo/DARC/DARC_mlp.py:140-222) as 16 kernel launches on the current stream, exact f32 on the matrix cores, bitwise reproducible run to
run, no hipGraph needed.  ``train`` is the reference's: update k = 1, then update k = 2, on the same batch.

The networks are the same torch modules as armenv.datd3.DATD3's, created in the same order (so ``torch.manual_seed(s)`` gives both
learners the same initial weights) and updated in place by the kernels; the Adam moments are tensors of this object and the four
Adam step counters live on the host."""
import torch

from . import _lib as L
from .fused_base import FusedLearner, _mlp, _mlp_of
from .policies import QValueNet
from .td3 import Actor

_LEARNING = ("actor1", "actor2", "critic1", "critic2")


class DATD3Schedule:
    """DATD3's and DARC's step schedule, written once for FusedDATD3 / FusedDARC and fused_datd3_pop's populations: the
    hyper-parameters, the host counters and ``update`` / ``train``, in terms of the base's ``_inputs``, ``_noise``, ``_workspace`` and
    ``_call``."""

    _darc = 0
    _Args = L.ArmEnvDatd3Args
    _hyper = ("policy_noise", "noise_clip", "seed", "q_weight", "regularization_weight")
    _takes_seed = True
    _HYPER_KW = ("hidden_dim", "actor_lr", "critic_lr", "tau", "gamma", "policy_noise", "noise_clip", "policy_freq")   # policy_freq: never read
    _COUNTERS = ("total_it",) + tuple(n + "_step" for n in _LEARNING)          # total_it counts updates: two per train()
    q_weight = regularization_weight = 0.0

    def _update(self, inputs, update_a1, noise):
        """one armenv_datd3_update over prepared tensors and checked `noise`; its `draw` is the update's number"""
        ws = self._workspace(inputs[0].shape[self._batch_axis])
        self.total_it += 1
        k = 1 if update_a1 else 2
        steps = dict(critic_step=getattr(self, "critic%d_step" % k) + 1, actor_step=getattr(self, "actor%d_step" % k) + 1)
        loss = self._call(ws, *inputs, noise, update_actor=k, draw=self.total_it, **steps)
        setattr(self, "critic%d_step" % k, steps["critic_step"])
        setattr(self, "actor%d_step" % k, steps["actor_step"])
        return loss

    def update(self, batch, update_a1=True, noise=None):
        """One update (the reference's `update(transition_dict, update_a1)`); `noise` (optional): [B,3] standard normals.  Returns the
        stepped critic's loss as a 0-dim tensor (no host sync); a population, from stacked tensors, the stepped critics' losses [P].
        A batch size or a `noise` that is refused raises before a counter moves."""
        inputs = self._inputs(batch)
        return self._update(inputs, update_a1, self._noise(noise, inputs[0].shape[self._batch_axis]))

    def train(self, batch, noise=None):
        """The reference's `train` from a dict of device tensors (states [B,D], actions [B,3], next_states [B,D], rewards [B], dones
        [B], any dtype): update k = 1 then update k = 2 on the same batch, with consecutive `draw`s.  `noise` (optional): a pair of
        [B,3] tensors of standard normals, one per update.  Returns the two critic losses as 0-dim tensors (no host sync).  A
        population updates every member: each tensor stacked under a leading [P], two loss tensors [P].  Both of `noise` are checked
        before the first update."""
        inputs = self._inputs(batch)
        B = inputs[0].shape[self._batch_axis]
        n1, n2 = (None, None) if noise is None else noise
        n1, n2 = self._noise(n1, B), self._noise(n2, B)
        return self._update(inputs, True, n1), self._update(inputs, False, n2)


class DARCSchedule(DATD3Schedule):
    """`darc` = 1, and DARC's two further hyper-parameters"""

    _darc = 1
    _HYPER_KW = DATD3Schedule._HYPER_KW + ("q_weight", "regularization_weight")


class FusedDATD3(DATD3Schedule, FusedLearner):
    """armenv.datd3.DATD3's constructor and public surface (``train(batch, noise=None)``, ``update``, ``total_it``, the eight modules,
    the ``actor`` property, ``take_action``, ``policy_state_dicts()``, ``_nets()``) with the update in HIP; ``load_from`` copies a
    DATD3's whole state.  ``seed`` keys the in-kernel target-policy noise (Philox4x32-10 over (seed, row, update number): both
    proposals of a row receive the same noise); ``noise=`` supplies it instead."""

    _fn = "datd3"
    _LEARNING = _LEARNING

    def __init__(self, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005, gamma=0.98,
                 policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0", seed=0):
        self._build(state_dim, action_dim, action_bound, device, seed, hidden_dim=hidden_dim, actor_lr=actor_lr, critic_lr=critic_lr,
                    tau=tau, gamma=gamma, policy_noise=policy_noise, noise_clip=noise_clip, policy_freq=policy_freq)

    def _build(self, state_dim, action_dim, action_bound, device, seed, **hyper):
        """the constructor's work, for FusedDARC's too: `hyper` is every name of ``_HYPER_KW``"""
        self._configure(state_dim, action_dim, action_bound, **hyper)
        self.device, self.seed = torch.device(device), int(seed)
        mk_a = lambda: Actor(state_dim, self.hidden_dim, action_dim, action_bound).to(self.device)
        mk_q = lambda: QValueNet(state_dim, self.hidden_dim, action_dim).to(self.device)
        self.actor1, self.actor2 = mk_a(), mk_a()               # DATD3's creation order
        self.critic1, self.critic2 = mk_q(), mk_q()
        self.target_actor1, self.target_actor2 = mk_a(), mk_a()
        self.target_critic1, self.target_critic2 = mk_q(), mk_q()
        for t_, n_ in zip(self._nets()[4:], self._nets()[:4]):
            t_.load_state_dict(n_.state_dict())
        for n in self._nets():
            n.requires_grad_(False)
        # Adam moments in parameters() order of each learning net
        for name in _LEARNING:
            net = getattr(self, name)
            setattr(self, name + "_m", [torch.zeros_like(p) for p in net.parameters()])
            setattr(self, name + "_v", [torch.zeros_like(p) for p in net.parameters()])

    @property
    def actor(self):
        return self.actor1

    def _nets(self):
        return (self.actor1, self.actor2, self.critic1, self.critic2,
                self.target_actor1, self.target_actor2, self.target_critic1, self.target_critic2)

    def _static_args(self):
        """the part of ArmEnvDatd3Args that does not change between updates"""
        a = super()._static_args()
        a.darc = self._darc
        for name in _LEARNING:
            setattr(a, name, _mlp(getattr(self, name)))
            setattr(a, "target_" + name, _mlp(getattr(self, "target_" + name)))
            setattr(a, name + "_m", _mlp_of(getattr(self, name + "_m")))
            setattr(a, name + "_v", _mlp_of(getattr(self, name + "_v")))
        return a

    def load_from(self, learner):
        """Copies parameters, Adam moments, the four step counters and total_it from an armenv.datd3.DATD3 / DARC (identical state for
        comparisons)."""
        self._load_from(learner, _LEARNING)

    def take_action(self, state):
        """DATD3_MLP.take_action (DATD3_mlp.py:88-109), as armenv.datd3.DATD3.take_action"""
        return self._take_action_of_two(state, self.critic1, self.critic2)

    def policy_state_dicts(self):
        """(actor1, actor2, critic1, critic2) for BatchedArmEnv.set_policy_datd3 / set_policy_darc"""
        return tuple({k: v.detach() for k, v in n.state_dict().items()} for n in self._nets()[:4])


class FusedDARC(DARCSchedule, FusedDATD3):
    """armenv.datd3.DARC's constructor and surface over the same call with `darc` = 1: the mixed target and the pull of critic k
    towards the other critic (which is read and never written)."""

    def __init__(self, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005, gamma=0.98,
                 policy_noise=0.2, noise_clip=0.5, policy_freq=3, q_weight=0.2, regularization_weight=0.005, device="cuda:0", seed=0):
        self._build(state_dim, action_dim, action_bound, device, seed, hidden_dim=hidden_dim, actor_lr=actor_lr, critic_lr=critic_lr,
                    tau=tau, gamma=gamma, policy_noise=policy_noise, noise_clip=noise_clip, policy_freq=policy_freq, q_weight=q_weight,
                    regularization_weight=regularization_weight)
