"""DADDPG learner whose update is the fused HIP update of libarmenv.so (armenv_daddpg_update, include/armenv.h; kernels in
csrc/armenv_learner.h): DADDPG_MLP.update (the reference's algo/DADDPG/DADDPG_mlp.py:117-171, its default agent) as 16 kernel
launches on the current stream, exact f32 on the matrix cores, bitwise reproducible run to run, no hipGraph needed.

The networks are the same torch modules as armenv.daddpg.DADDPG's, created in the same order (so ``torch.manual_seed(s)`` gives both
learners the same initial weights) and updated in place by the kernels; the Adam moments are tensors of this object and the three
Adam step counters live on the host."""
import ctypes as C

import torch

from . import _lib as L
from .fused_td3 import _mlp, _mlp_of
from .policies import QValueNet
from .td3 import Actor


class FusedDADDPG:
    """armenv.daddpg.DADDPG's constructor and public surface (``train(batch)``, ``total_it``, the six modules, the ``actor`` property,
    ``take_action``, ``policy_state_dicts()``, ``_nets()``) with the update in HIP; ``load_from`` copies a DADDPG's whole state."""

    def __init__(self, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005, gamma=0.98,
                 device="cuda:0"):
        if hidden_dim != 256 or action_dim != 3 or not 1 <= state_dim <= 12:
            raise ValueError("FusedDADDPG: the fused update is built for hidden_dim 256, action_dim 3, state_dim 1..12")
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
        self.state_dim, self.action_dim, self.hidden_dim = state_dim, action_dim, hidden_dim
        self.actor_lr, self.critic_lr, self.tau, self.gamma, self.action_bound = actor_lr, critic_lr, tau, gamma, action_bound
        self.betas, self.eps = (0.9, 0.999), 1e-8                 # torch.optim.Adam's defaults, as DADDPG's optimisers
        # Adam moments in parameters() order of each learning net
        zeros = lambda net: [torch.zeros_like(p) for p in net.parameters()]
        self.actor1_m, self.actor1_v = zeros(self.actor1), zeros(self.actor1)
        self.actor2_m, self.actor2_v = zeros(self.actor2), zeros(self.actor2)
        self.critic_m, self.critic_v = zeros(self.critic), zeros(self.critic)
        self.critic_step = self.actor1_step = self.actor2_step = 0
        self.total_it = 0
        self._ws = None
        self._args = None

    @property
    def actor(self):
        return self.actor1

    def _nets(self):
        return (self.actor1, self.actor2, self.critic, self.target_actor1, self.target_actor2, self.target_critic)

    def _static_args(self):
        """the part of ArmEnvDaddpgArgs that does not change between updates"""
        a = L.ArmEnvDaddpgArgs()
        a.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        a.state_dim, a.action_dim, a.hidden_dim = self.state_dim, self.action_dim, self.hidden_dim
        a.action_bound, a.gamma, a.tau = self.action_bound, self.gamma, self.tau
        a.actor_lr, a.critic_lr = self.actor_lr, self.critic_lr
        a.beta1, a.beta2, a.eps = self.betas[0], self.betas[1], self.eps
        for name in ("actor1", "actor2", "critic", "target_actor1", "target_actor2", "target_critic"):
            setattr(a, name, _mlp(getattr(self, name)))
        for name in ("actor1", "actor2", "critic"):
            setattr(a, name + "_m", _mlp_of(getattr(self, name + "_m")))
            setattr(a, name + "_v", _mlp_of(getattr(self, name + "_v")))
        return a

    def batch_buffers(self, batch_size):
        """static input tensors of `batch_size` rows that ``TrajectoryStore.sample(out=...)`` fills in place"""
        B, D, dev = int(batch_size), self.state_dim, self.device
        return dict(states=torch.zeros(B, D, device=dev), actions=torch.zeros(B, self.action_dim, device=dev),
                    next_states=torch.zeros(B, D, device=dev), rewards=torch.zeros(B, device=dev),
                    dones=torch.zeros(B, dtype=torch.uint8, device=dev))

    def _workspace(self, B):
        n = L.load().armenv_daddpg_workspace_bytes(self.state_dim, self.hidden_dim, B)
        if n < 0:
            raise ValueError("FusedDADDPG: unsupported batch size %d" % B)
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._ws

    def train(self, batch):
        """One update from a dict of device tensors: states [B,D], actions [B,3], next_states [B,D], rewards [B], dones [B] (any
        dtype).  Returns the critic loss as a 0-dim tensor (no host sync)."""
        dev = self.device
        f32 = lambda k: batch[k].to(dev, torch.float32).contiguous()
        s, a, s2 = f32("states"), f32("actions"), f32("next_states")
        r = batch["rewards"].to(dev, torch.float32).reshape(-1).contiguous()
        d = batch["dones"].to(dev)
        d = (d if d.dtype == torch.uint8 else (d != 0).to(torch.uint8)).reshape(-1).contiguous()
        B = s.shape[0]
        self.total_it += 1
        update_a1 = self.total_it % 2 == 0                        # DADDPG_mlp.py:119
        if self._args is None:
            self._args = self._static_args()
        args = self._args
        ws = self._workspace(B)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        args.batch = B
        args.critic_step = self.critic_step + 1
        args.update_actor = 1 if update_a1 else 2
        args.actor_step = (self.actor1_step if update_a1 else self.actor2_step) + 1
        args.states_dev, args.actions_dev, args.next_states_dev = s.data_ptr(), a.data_ptr(), s2.data_ptr()
        args.rewards_dev, args.dones_dev, args.loss_dev = r.data_ptr(), d.data_ptr(), loss.data_ptr()
        args.workspace_dev, args.workspace_bytes = ws.data_ptr(), ws.numel()
        L.check(L.load().armenv_daddpg_update(C.byref(args), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self.critic_step += 1
        if update_a1:
            self.actor1_step += 1
        else:
            self.actor2_step += 1
        return loss

    @torch.no_grad()
    def load_from(self, daddpg):
        """Copies parameters, Adam moments, the three step counters and total_it from an armenv.daddpg.DADDPG (identical state for
        comparisons)."""
        for mine, theirs in zip(self._nets(), daddpg._nets()):
            for p, q in zip(mine.parameters(), theirs.parameters()):
                p.copy_(q)
        for name in ("actor1", "actor2", "critic"):
            opt = getattr(daddpg, name + "_opt")
            step = 0
            for p, m, v in zip(getattr(daddpg, name).parameters(), getattr(self, name + "_m"), getattr(self, name + "_v")):
                st = opt.state.get(p, {})
                if "exp_avg" in st:
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                    step = int(st["step"])
                else:
                    m.zero_()
                    v.zero_()
            setattr(self, name + "_step", step)
        self.total_it = daddpg.total_it

    @torch.no_grad()
    def take_action(self, state):
        """DADDPG_MLP.take_action (DADDPG_mlp.py:77-97), as armenv.daddpg.DADDPG.take_action"""
        import numpy as np
        s = torch.tensor(np.asarray([state], dtype=np.float32), device=self.device)
        a1, a2 = self.actor1(s), self.actor2(s)
        q1, q2 = self.critic(s, a1), self.critic(s, a2)
        return (a1 if bool(q1 >= q2) else a2).cpu().numpy()[0]

    def policy_state_dicts(self):
        """(actor1, actor2, critic) for BatchedArmEnv.set_policy_daddpg"""
        return tuple({k: v.detach() for k, v in n.state_dict().items()} for n in (self.actor1, self.actor2, self.critic))
