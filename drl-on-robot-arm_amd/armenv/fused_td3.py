"""TD3 learner whose update is the fused HIP update of libarmenv.so (armenv_td3_update, include/armenv.h; kernels in
csrc/armenv_learner.h): TD3_MLP.train (the reference's algo/TD3/TD3_mlp.py:114-161) as 9 kernel launches (16 with the delayed
actor step) on the current stream, exact f32 on the matrix cores, bitwise reproducible run to run, no hipGraph needed.

The networks are the same torch modules as armenv.td3.TD3's, created in the same order (so ``torch.manual_seed(s)`` gives both
learners the same initial weights) and updated in place by the kernels; the Adam moments are tensors of this object and the Adam
step counters live on the host."""
import ctypes as C

import torch

from . import _lib as L
from .td3 import Actor, TwinCritic


def _mlp(net, heads=("fc1", "fc2", "fc3")):
    m = L.ArmEnvMlpRW()
    for i, name in enumerate(heads):
        layer = getattr(net, name)
        for key, t in (("W%d" % (i + 1), layer.weight), ("b%d" % (i + 1), layer.bias)):
            assert t.is_contiguous() and t.dtype == torch.float32
            setattr(m, key, t.data_ptr())
    return m


def _mlp_of(tensors):
    """ArmEnvMlpRW over six tensors in W1, b1, W2, b2, W3, b3 order"""
    m = L.ArmEnvMlpRW()
    for key, t in zip(("W1", "b1", "W2", "b2", "W3", "b3"), tensors):
        setattr(m, key, t.data_ptr())
    return m


class FusedTD3:
    """armenv.td3.TD3's constructor and public surface (``train(batch)``, ``total_it``, ``actor_state_dict()``, ``take_action``, the
    ``actor`` / ``critic`` / ``target_actor`` / ``target_critic`` modules) with the update in HIP.  ``seed`` keys the in-kernel
    target-policy noise (Philox4x32-10 over (seed, row, update number)); ``train(batch, noise=...)`` supplies it instead."""

    def __init__(self, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.98, policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0", seed=0):
        self.device = torch.device(device)
        self.actor = Actor(state_dim, hidden_dim, action_dim, action_bound).to(self.device)       # TD3's creation order
        self.critic = TwinCritic(state_dim, hidden_dim, action_dim).to(self.device)
        self.target_actor = Actor(state_dim, hidden_dim, action_dim, action_bound).to(self.device)
        self.target_critic = TwinCritic(state_dim, hidden_dim, action_dim).to(self.device)
        self.target_critic.load_state_dict(self.critic.state_dict())
        self.target_actor.load_state_dict(self.actor.state_dict())
        for n in self._nets():
            n.requires_grad_(False)
        self.state_dim, self.action_dim, self.hidden_dim = state_dim, action_dim, hidden_dim
        self.actor_lr, self.critic_lr, self.tau, self.gamma, self.action_bound = actor_lr, critic_lr, tau, gamma, action_bound
        self.policy_noise, self.noise_clip, self.policy_freq = policy_noise, noise_clip, policy_freq
        self.betas, self.eps = (0.9, 0.999), 1e-8                 # torch.optim.Adam's defaults, as TD3's optimisers
        self.seed = int(seed)
        # Adam moments in parameters() order of the actor and of the critic
        self.actor_m = [torch.zeros_like(p) for p in self.actor.parameters()]
        self.actor_v = [torch.zeros_like(p) for p in self.actor.parameters()]
        self.critic_m = [torch.zeros_like(p) for p in self.critic.parameters()]
        self.critic_v = [torch.zeros_like(p) for p in self.critic.parameters()]
        self.actor_step = self.critic_step = 0
        self.total_it = 0
        self._ws = None
        self._args = None
        if hidden_dim != 256 or action_dim != 3 or not 1 <= state_dim <= 12:
            raise ValueError("FusedTD3: the fused update is built for hidden_dim 256, action_dim 3, state_dim 1..12")

    def _nets(self):
        return (self.actor, self.critic, self.target_actor, self.target_critic)

    def _static_args(self):
        """the part of ArmEnvTd3Args that does not change between updates"""
        a = L.ArmEnvTd3Args()
        a.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        a.state_dim, a.action_dim, a.hidden_dim = self.state_dim, self.action_dim, self.hidden_dim
        a.action_bound, a.gamma, a.tau = self.action_bound, self.gamma, self.tau
        a.policy_noise, a.noise_clip, a.actor_lr, a.critic_lr = self.policy_noise, self.noise_clip, self.actor_lr, self.critic_lr
        a.beta1, a.beta2, a.eps = self.betas[0], self.betas[1], self.eps
        a.seed = self.seed
        a.actor, a.target_actor = _mlp(self.actor), _mlp(self.target_actor)
        q1, q2 = ("fc1", "fc2", "fc3"), ("fc4", "fc5", "fc6")
        a.q1, a.q2 = _mlp(self.critic, q1), _mlp(self.critic, q2)
        a.target_q1, a.target_q2 = _mlp(self.target_critic, q1), _mlp(self.target_critic, q2)
        a.actor_m, a.actor_v = _mlp_of(self.actor_m), _mlp_of(self.actor_v)
        a.q1_m, a.q1_v = _mlp_of(self.critic_m[:6]), _mlp_of(self.critic_v[:6])
        a.q2_m, a.q2_v = _mlp_of(self.critic_m[6:]), _mlp_of(self.critic_v[6:])
        return a

    def batch_buffers(self, batch_size):
        """static input tensors of `batch_size` rows that ``TrajectoryStore.sample(out=...)`` fills in place"""
        B, D, dev = int(batch_size), self.state_dim, self.device
        return dict(states=torch.zeros(B, D, device=dev), actions=torch.zeros(B, self.action_dim, device=dev),
                    next_states=torch.zeros(B, D, device=dev), rewards=torch.zeros(B, device=dev),
                    dones=torch.zeros(B, dtype=torch.uint8, device=dev))

    def _workspace(self, B):
        n = L.load().armenv_td3_workspace_bytes(self.state_dim, self.hidden_dim, B)
        if n < 0:
            raise ValueError("FusedTD3: unsupported batch size %d" % B)
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._ws

    def train(self, batch, noise=None):
        """One update from a dict of device tensors: states [B,D], actions [B,3], next_states [B,D], rewards [B], dones [B] (any
        dtype).  `noise` (optional): [B,3] standard normals for the target-policy noise.  Returns the critic loss as a 0-dim tensor
        (no host sync)."""
        dev = self.device
        f32 = lambda k: batch[k].to(dev, torch.float32).contiguous()
        s, a, s2 = f32("states"), f32("actions"), f32("next_states")
        r = batch["rewards"].to(dev, torch.float32).reshape(-1).contiguous()
        d = batch["dones"].to(dev)
        d = (d if d.dtype == torch.uint8 else (d != 0).to(torch.uint8)).reshape(-1).contiguous()
        B = s.shape[0]
        if noise is not None:
            noise = noise.to(dev, torch.float32).contiguous()
            assert tuple(noise.shape) == (B, self.action_dim)
        self.total_it += 1
        with_actor = self.total_it % self.policy_freq == 0          # delayed actor + soft updates, TD3_mlp.py:144
        if self._args is None:
            self._args = self._static_args()
        args = self._args
        ws = self._workspace(B)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        args.batch = B
        args.critic_step = self.critic_step + 1
        args.actor_step = self.actor_step + 1 if with_actor else 0
        args.with_actor = int(with_actor)
        args.draw = self.total_it
        args.noise_dev = noise.data_ptr() if noise is not None else None
        args.states_dev, args.actions_dev, args.next_states_dev = s.data_ptr(), a.data_ptr(), s2.data_ptr()
        args.rewards_dev, args.dones_dev, args.loss_dev = r.data_ptr(), d.data_ptr(), loss.data_ptr()
        args.workspace_dev, args.workspace_bytes = ws.data_ptr(), ws.numel()
        L.check(L.load().armenv_td3_update(C.byref(args), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self.critic_step += 1
        if with_actor:
            self.actor_step += 1
        return loss

    @torch.no_grad()
    def load_from(self, td3):
        """Copies parameters, Adam moments, step counters and total_it from an armenv.td3.TD3 (identical state for comparisons)."""
        for mine, theirs in zip(self._nets(), td3._nets()):
            for p, q in zip(mine.parameters(), theirs.parameters()):
                p.copy_(q)
        for params, opt, ms, vs, which in ((list(td3.actor.parameters()), td3.actor_opt, self.actor_m, self.actor_v, "actor"),
                                           (list(td3.critic.parameters()), td3.critic_opt, self.critic_m, self.critic_v, "critic")):
            step = 0
            for p, m, v in zip(params, ms, vs):
                st = opt.state.get(p, {})
                if "exp_avg" in st:
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                    step = int(st["step"])
                else:
                    m.zero_()
                    v.zero_()
            setattr(self, which + "_step", step)
        self.total_it = td3.total_it

    def take_action(self, state):
        """TD3_MLP.take_action (TD3_mlp.py:82-97), as armenv.td3.TD3.take_action"""
        import numpy as np
        with torch.no_grad():
            s = torch.tensor(np.asarray([state], dtype=np.float32), device=self.device)
            return self.actor(s).detach().cpu().numpy()[0]

    def actor_state_dict(self):
        return {k: v.detach() for k, v in self.actor.state_dict().items()}
