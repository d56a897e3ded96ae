"""TD3 learner whose update is the fused HIP update of libarmenv.so (armenv_td3_update, include/armenv.h; kernels in
csrc/armenv_learner.h): TD3_MLP.train (the reference's algo/TD3/TD3_mlp.py:114-161) as 9 kernel launches (16 with the delayed
actor step) on the current stream, exact f32 on the matrix cores, bitwise reproducible run to run, no hipGraph needed.

The networks are the same torch modules as armenv.td3.TD3's, created in the same order (so ``torch.manual_seed(s)`` gives both
learners the same initial weights) and updated in place by the kernels; the Adam moments are tensors of this object and the Adam
step counters live on the host."""
import torch

from . import _lib as L
from .fused_base import FusedLearner, _mlp, _mlp_of  # noqa: F401  (_mlp, _mlp_of: importable from here as before)
from .td3 import Actor, TwinCritic


class TD3Schedule:
    """TD3's step schedule, written once for FusedTD3 and fused_td3_pop.FusedTD3Population: the hyper-parameters, the host counters and
    ``train``, in terms of the base's ``_inputs``, ``_noise``, ``_workspace`` and ``_call``."""

    _Args = L.ArmEnvTd3Args
    _hyper = ("policy_noise", "noise_clip", "seed")
    _takes_seed = True
    _HYPER_KW = ("hidden_dim", "actor_lr", "critic_lr", "tau", "gamma", "policy_noise", "noise_clip", "policy_freq")
    _COUNTERS = ("total_it", "critic_step", "actor_step")

    def train(self, batch, noise=None):
        """One update from a dict of device tensors: states [B,D], actions [B,3], next_states [B,D], rewards [B], dones [B] (any
        dtype).  `noise` (optional): [B,3] standard normals for the target-policy noise.  Returns the critic loss as a 0-dim tensor
        (no host sync).  A population updates every member: each tensor stacked under a leading [P], the critic losses [P].  A batch
        size or a `noise` that is refused raises before a counter moves."""
        inputs = self._inputs(batch)
        B = inputs[0].shape[self._batch_axis]
        noise = self._noise(noise, B)
        ws = self._workspace(B)
        self.total_it += 1
        with_actor = self.total_it % self.policy_freq == 0          # delayed actor + soft updates, TD3_mlp.py:144
        loss = self._call(ws, *inputs, noise, critic_step=self.critic_step + 1, actor_step=self.actor_step + 1 if with_actor else 0,
                          with_actor=int(with_actor), draw=self.total_it)
        self.critic_step += 1
        if with_actor:
            self.actor_step += 1
        return loss


class FusedTD3(TD3Schedule, FusedLearner):
    """armenv.td3.TD3's constructor and public surface (``train(batch)``, ``total_it``, ``actor_state_dict()``, ``take_action``, the
    ``actor`` / ``critic`` / ``target_actor`` / ``target_critic`` modules) with the update in HIP.  ``seed`` keys the in-kernel
    target-policy noise (Philox4x32-10 over (seed, row, update number)); ``train(batch, noise=...)`` supplies it instead."""

    _fn, _noise_error = "td3", AssertionError
    _LEARNING = ("actor", "critic")

    def __init__(self, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0", seed=0):
        self._configure(state_dim, action_dim, action_bound, hidden_dim=hidden_dim, actor_lr=actor_lr, critic_lr=critic_lr, tau=tau,
                        gamma=gamma, policy_noise=policy_noise, noise_clip=noise_clip, policy_freq=policy_freq)
        self.device, self.seed = torch.device(device), int(seed)
        self.actor = Actor(state_dim, hidden_dim, action_dim, action_bound).to(self.device)       # TD3's creation order
        self.critic = TwinCritic(state_dim, hidden_dim, action_dim).to(self.device)
        self.target_actor = Actor(state_dim, hidden_dim, action_dim, action_bound).to(self.device)
        self.target_critic = TwinCritic(state_dim, hidden_dim, action_dim).to(self.device)
        self.target_critic.load_state_dict(self.critic.state_dict())
        self.target_actor.load_state_dict(self.actor.state_dict())
        for n in self._nets():
            n.requires_grad_(False)
        # Adam moments in parameters() order of the actor and of the critic
        self.actor_m = [torch.zeros_like(p) for p in self.actor.parameters()]
        self.actor_v = [torch.zeros_like(p) for p in self.actor.parameters()]
        self.critic_m = [torch.zeros_like(p) for p in self.critic.parameters()]
        self.critic_v = [torch.zeros_like(p) for p in self.critic.parameters()]

    def _nets(self):
        return (self.actor, self.critic, self.target_actor, self.target_critic)

    def _static_args(self):
        """the part of ArmEnvTd3Args that does not change between updates"""
        a = super()._static_args()
        a.actor, a.target_actor = _mlp(self.actor), _mlp(self.target_actor)
        q1, q2 = ("fc1", "fc2", "fc3"), ("fc4", "fc5", "fc6")
        a.q1, a.q2 = _mlp(self.critic, q1), _mlp(self.critic, q2)
        a.target_q1, a.target_q2 = _mlp(self.target_critic, q1), _mlp(self.target_critic, q2)
        a.actor_m, a.actor_v = _mlp_of(self.actor_m), _mlp_of(self.actor_v)
        a.q1_m, a.q1_v = _mlp_of(self.critic_m[:6]), _mlp_of(self.critic_v[:6])
        a.q2_m, a.q2_v = _mlp_of(self.critic_m[6:]), _mlp_of(self.critic_v[6:])
        return a

    def load_from(self, td3):
        """Copies parameters, Adam moments, step counters and total_it from an armenv.td3.TD3 (identical state for comparisons)."""
        self._load_from(td3, ("actor", "critic"))

    def take_action(self, state):
        """TD3_MLP.take_action (TD3_mlp.py:82-97), as armenv.td3.TD3.take_action"""
        import numpy as np
        with torch.no_grad():
            s = torch.tensor(np.asarray([state], dtype=np.float32), device=self.device)
            return self.actor(s).detach().cpu().numpy()[0]

    def actor_state_dict(self):
        return {k: v.detach() for k, v in self.actor.state_dict().items()}
