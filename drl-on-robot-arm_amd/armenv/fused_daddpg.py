"""DADDPG learner whose update is the fused HIP update of libarmenv.so (armenv_daddpg_update, include/armenv.h; kernels in
csrc/armenv_learner.h): DADDPG_MLP.update (the reference's algo/DADDPG/DADDPG_mlp.py:117-171, its default agent) as 16 kernel
launches on the current stream, exact f32 on the matrix cores, bitwise reproducible run to run, no hipGraph needed.

The networks are the same torch modules as armenv.daddpg.DADDPG's, created in the same order (so ``torch.manual_seed(s)`` gives both
learners the same initial weights) and updated in place by the kernels; the Adam moments are tensors of this object and the three
Adam step counters live on the host."""
import torch

from . import _lib as L
from .fused_base import FusedLearner, _mlp, _mlp_of
from .policies import QValueNet
from .td3 import Actor


class DADDPGSchedule:
    """DADDPG's step schedule, written once for FusedDADDPG and fused_daddpg_pop.FusedDADDPGPopulation: the hyper-parameters, the host
    counters and ``train``, in terms of the base's ``_inputs``, ``_workspace`` and ``_call``."""

    _Args = L.ArmEnvDaddpgArgs
    _HYPER_KW = ("hidden_dim", "actor_lr", "critic_lr", "tau", "gamma")
    _COUNTERS = ("total_it", "critic_step", "actor1_step", "actor2_step")

    def train(self, batch):
        """One update from a dict of device tensors: states [B,D], actions [B,3], next_states [B,D], rewards [B], dones [B] (any
        dtype).  Returns the critic loss as a 0-dim tensor (no host sync).  A population updates every member: each tensor stacked
        under a leading [P], the critic losses [P].  A batch size that is refused raises before a counter moves."""
        inputs = self._inputs(batch)
        ws = self._workspace(inputs[0].shape[self._batch_axis])
        self.total_it += 1
        update_a1 = self.total_it % 2 == 0                        # DADDPG_mlp.py:119
        loss = self._call(ws, *inputs, critic_step=self.critic_step + 1, update_actor=1 if update_a1 else 2,
                          actor_step=(self.actor1_step if update_a1 else self.actor2_step) + 1)
        self.critic_step += 1
        if update_a1:
            self.actor1_step += 1
        else:
            self.actor2_step += 1
        return loss


class FusedDADDPG(DADDPGSchedule, FusedLearner):
    """armenv.daddpg.DADDPG's constructor and public surface (``train(batch)``, ``total_it``, the six modules, the ``actor`` property,
    ``take_action``, ``policy_state_dicts()``, ``_nets()``) with the update in HIP; ``load_from`` copies a DADDPG's whole state."""

    _fn = "daddpg"
    _LEARNING = ("actor1", "actor2", "critic")

    def __init__(self, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005, gamma=0.98,
                 device="cuda:0"):
        self._configure(state_dim, action_dim, action_bound, hidden_dim=hidden_dim, actor_lr=actor_lr, critic_lr=critic_lr, tau=tau,
                        gamma=gamma)
        self.device = torch.device(device)
        mk_a = lambda: Actor(state_dim, hidden_dim, action_dim, action_bound).to(self.device)
        mk_q = lambda: QValueNet(state_dim, hidden_dim, action_dim).to(self.device)
        self.actor1, self.actor2 = mk_a(), mk_a()               # DADDPG's creation order
        self.critic = mk_q()
        self.target_actor1, self.target_actor2 = mk_a(), mk_a()
        self.target_critic = mk_q()
        for t_, n_ in ((self.target_actor1, self.actor1), (self.target_actor2, self.actor2), (self.target_critic, self.critic)):
            t_.load_state_dict(n_.state_dict())
        for n in self._nets():
            n.requires_grad_(False)
        # Adam moments in parameters() order of each learning net
        zeros = lambda net: [torch.zeros_like(p) for p in net.parameters()]
        self.actor1_m, self.actor1_v = zeros(self.actor1), zeros(self.actor1)
        self.actor2_m, self.actor2_v = zeros(self.actor2), zeros(self.actor2)
        self.critic_m, self.critic_v = zeros(self.critic), zeros(self.critic)

    @property
    def actor(self):
        return self.actor1

    def _nets(self):
        return (self.actor1, self.actor2, self.critic, self.target_actor1, self.target_actor2, self.target_critic)

    def _static_args(self):
        """the part of ArmEnvDaddpgArgs that does not change between updates"""
        a = super()._static_args()
        for name in ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic"):
            setattr(a, name, _mlp(getattr(self, name)))
        for name in ("actor1", "actor2", "critic"):
            setattr(a, name + "_m", _mlp_of(getattr(self, name + "_m")))
            setattr(a, name + "_v", _mlp_of(getattr(self, name + "_v")))
        return a

    def load_from(self, daddpg):
        """Copies parameters, Adam moments, the three step counters and total_it from an armenv.daddpg.DADDPG (identical state for
        comparisons)."""
        self._load_from(daddpg, ("actor1", "actor2", "critic"))

    def take_action(self, state):
        """DADDPG_MLP.take_action (DADDPG_mlp.py:77-97), as armenv.daddpg.DADDPG.take_action"""
        return self._take_action_of_two(state, self.critic, self.critic)

    def policy_state_dicts(self):
        """(actor1, actor2, critic) for BatchedArmEnv.set_policy_daddpg"""
        return tuple({k: v.detach() for k, v in n.state_dict().items()} for n in (self.actor1, self.actor2, self.critic))
