"""What the fused learners (fused_td3.FusedTD3, fused_daddpg.FusedDADDPG, fused_datd3.FusedDATD3 / FusedDARC) share: the ArmEnvMlpRW
views of their nets, the batch and workspace tensors, the argument struct's common part and the one call into libarmenv.so."""
import ctypes as C

import torch

from . import _lib as L


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


class FusedLearner:
    """Base of the fused learners.  A subclass names its C entry points (``_fn`` of armenv_<_fn>_update and
    armenv_<_fn>_workspace_bytes), its argument struct ``_Args``, the hyper-parameters ``_hyper`` it copies into it beside the
    common ones, and which exception ``_noise_error`` a wrongly shaped ``noise`` raises; it creates its own nets, in its torch
    learner's order."""

    _fn = _Args = None
    _hyper = ()
    _noise_error = ValueError

    def _check_shapes(self, state_dim, action_dim, hidden_dim):
        if hidden_dim != 256 or action_dim != 3 or not 1 <= state_dim <= 12:
            raise ValueError("%s: the fused update is built for hidden_dim 256, action_dim 3, state_dim 1..12" % type(self).__name__)

    def _static_args(self):
        """the part of the argument struct that does not change between updates: what every update has; a subclass adds its nets"""
        a = self._Args()
        a.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        a.state_dim, a.action_dim, a.hidden_dim = self.state_dim, self.action_dim, self.hidden_dim
        a.action_bound, a.gamma, a.tau = self.action_bound, self.gamma, self.tau
        a.actor_lr, a.critic_lr = self.actor_lr, self.critic_lr
        a.beta1, a.beta2, a.eps = self.betas[0], self.betas[1], self.eps
        for name in self._hyper:
            setattr(a, name, getattr(self, name))
        return a

    def batch_buffers(self, batch_size):
        """static input tensors of `batch_size` rows that ``TrajectoryStore.sample(out=...)`` fills in place"""
        B, D, dev = int(batch_size), self.state_dim, self.device
        return dict(states=torch.zeros(B, D, device=dev), actions=torch.zeros(B, self.action_dim, device=dev),
                    next_states=torch.zeros(B, D, device=dev), rewards=torch.zeros(B, device=dev),
                    dones=torch.zeros(B, dtype=torch.uint8, device=dev))

    def _workspace(self, B):
        n = getattr(L.load(), "armenv_%s_workspace_bytes" % self._fn)(self.state_dim, self.hidden_dim, B)
        if n < 0:
            raise ValueError("%s: unsupported batch size %d" % (type(self).__name__, B))
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._ws

    def _inputs(self, batch):
        """(states, actions, rewards, next_states, dones) of a batch dict as the contiguous f32 / uint8 device tensors the update reads"""
        dev = self.device
        f32 = lambda k: batch[k].to(dev, torch.float32).contiguous()
        r = batch["rewards"].to(dev, torch.float32).reshape(-1).contiguous()
        d = batch["dones"].to(dev)
        d = (d if d.dtype == torch.uint8 else (d != 0).to(torch.uint8)).reshape(-1).contiguous()
        return f32("states"), f32("actions"), r, f32("next_states"), d

    def _noise(self, noise, B):
        """`noise` as the [B][action_dim] f32 device tensor the update reads, or None"""
        if noise is not None:
            noise = noise.to(self.device, torch.float32).contiguous()
            if tuple(noise.shape) != (B, self.action_dim):
                raise self._noise_error("noise must be [B][%d] standard normals" % self.action_dim)
        return noise

    def _call(self, s, a, r, s2, d, noise=None, **per_call):
        """One armenv_<_fn>_update over prepared tensors on the current stream, with `per_call` (step numbers, which nets, draw)
        written into the argument struct first; returns the critic loss as a 0-dim tensor (no host sync)."""
        if self._args is None:
            self._args = self._static_args()
        args = self._args
        B = s.shape[0]
        ws = self._workspace(B)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        args.batch = B
        for key, value in per_call.items():
            setattr(args, key, value)
        if hasattr(args, "noise_dev"):
            args.noise_dev = noise.data_ptr() if noise is not None else None
        args.states_dev, args.actions_dev, args.next_states_dev = s.data_ptr(), a.data_ptr(), s2.data_ptr()
        args.rewards_dev, args.dones_dev, args.loss_dev = r.data_ptr(), d.data_ptr(), loss.data_ptr()
        args.workspace_dev, args.workspace_bytes = ws.data_ptr(), ws.numel()
        update = getattr(L.load(), "armenv_%s_update" % self._fn)
        L.check(update(C.byref(args), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return loss

    @torch.no_grad()
    def _load_from(self, learner, names):
        """Copies parameters, the Adam moments and step counters of the nets `names` (`<name>_opt` of the torch learner) and total_it."""
        for mine, theirs in zip(self._nets(), learner._nets()):
            for p, q in zip(mine.parameters(), theirs.parameters()):
                p.copy_(q)
        for name in names:
            opt = getattr(learner, name + "_opt")
            step = 0
            for p, m, v in zip(getattr(learner, name).parameters(), getattr(self, name + "_m"), getattr(self, name + "_v")):
                st = opt.state.get(p, {})
                if "exp_avg" in st:
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                    step = int(st["step"])
                else:
                    m.zero_()
                    v.zero_()
            setattr(self, name + "_step", step)
        self.total_it = learner.total_it

    @torch.no_grad()
    def _take_action_of_two(self, state, critic1, critic2):
        """the two-actor agents' take_action: the proposal of actor1 / actor2 that its critic values higher"""
        import numpy as np
        s = torch.tensor(np.asarray([state], dtype=np.float32), device=self.device)
        a1, a2 = self.actor1(s), self.actor2(s)
        q1, q2 = critic1(s, a1), critic2(s, a2)
        return (a1 if bool(q1 >= q2) else a2).cpu().numpy()[0]
