"""The reference's two double-actor / double-critic agents on PyTorch-ROCm tensors: DATD3_MLP (the reference's
algo/DATD3/DATD3_mlp.py:140-211) and DARC_MLP (algo/DARC/DARC_mlp.py:134-222) -- two actors, two critics, a cross-update scheme: one
``train`` is update(batch, k = 1) followed by update(batch, k = 2) on the SAME batch, each update stepping critic k and actor k only.
DARC is DATD3 with a mixed target and one more term in the critic's loss.  Like armenv.daddpg they consume device-resident HER batches
(armenv.replay.TrajectoryStore.sample) and hand their four learning nets to the env engine for fused rollouts
(BatchedArmEnv.set_policy_datd3 / set_policy_darc: take_action inside the rollout kernel).  Stock torch ops: the learner is
integration, not a kernel (the fused HIP update: armenv.fused_datd3)."""
import torch

from .policies import QValueNet
from .td3 import Actor, GraphedLearner, mean_sq, neg_mean


def _batch_tensors(batch, device):
    s = batch["states"].to(device, torch.float32)
    a = batch["actions"].to(device, torch.float32)
    r = batch["rewards"].to(device, torch.float32).view(-1, 1)
    s2 = batch["next_states"].to(device, torch.float32)
    d = batch["dones"].to(device, torch.float32).view(-1, 1)
    return s, a, r, s2, d


class DATD3(GraphedLearner):
    """Hyper-parameters default to config.py (hidden 256, lr 1e-3, tau 0.005, gamma 0.98, policy noise 0.2, clip 0.5).  `policy_freq`
    is accepted because the reference's constructor has it; like there it is never read: no update is delayed."""

    def __init__(self, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005, gamma=0.98,
                 policy_noise=0.2, noise_clip=0.5, policy_freq=3, device="cuda:0"):
        self.device = torch.device(device)
        cap = self.device.type == "cuda"      # step counters on the device: the update can be captured in a hipGraph
        mk_a = lambda: Actor(state_dim, hidden_dim, action_dim, action_bound).to(self.device)
        mk_q = lambda: QValueNet(state_dim, hidden_dim, action_dim).to(self.device)
        # the four learning nets in the reference's creation order (DATD3_mlp.py:62-76: their initial weights are a function of it
        # under torch.manual_seed; the reference's targets are deep copies, which draw nothing) -- the targets after them
        self.actor1, self.actor2 = mk_a(), mk_a()
        self.critic1, self.critic2 = mk_q(), mk_q()
        self.target_actor1, self.target_actor2 = mk_a(), mk_a()
        self.target_critic1, self.target_critic2 = mk_q(), mk_q()
        for t_, n_ in zip(self._nets()[4:], self._nets()[:4]):
            t_.load_state_dict(n_.state_dict())
        self.actor1_opt = torch.optim.Adam(self.actor1.parameters(), lr=actor_lr, capturable=cap)
        self.actor2_opt = torch.optim.Adam(self.actor2.parameters(), lr=actor_lr, capturable=cap)
        self.critic1_opt = torch.optim.Adam(self.critic1.parameters(), lr=critic_lr, capturable=cap)
        self.critic2_opt = torch.optim.Adam(self.critic2.parameters(), lr=critic_lr, capturable=cap)
        self.tau, self.gamma, self.action_bound = tau, gamma, action_bound
        self.policy_noise, self.noise_clip, self.policy_freq = policy_noise, noise_clip, policy_freq
        self.total_it = 0                     # counts updates: two per train()
        self._graphs = None

    @property
    def actor(self):          # (GraphedLearner.capture reads the observation / action widths off `actor`)
        return self.actor1

    def _nets(self):
        return (self.actor1, self.actor2, self.critic1, self.critic2,
                self.target_actor1, self.target_actor2, self.target_critic1, self.target_critic2)

    def _opts(self):
        return (self.actor1_opt, self.actor2_opt, self.critic1_opt, self.critic2_opt)

    def _target_value(self, t):
        """what the target's `gamma (1 - done)` multiplies, given t = min(target_critic1(s2, a2_1), target_critic2(s2, a2_2))"""
        return t

    def _critic_loss(self, q, s, a, other, target_q):
        return mean_sq(q - target_q)                                               # F.mse_loss, DATD3_mlp.py:180 / :197

    def _update(self, s, a, r, s2, d, update_a1, noise=None):
        """ONE DATD3_MLP.update (DATD3_mlp.py:146-211): both target actors propose under ONE noise draw, each target critic values
        its own actor's proposal, critic k regresses on r + gamma (1 - done) min of the two, then actor k ascends the stepped critic k;
        soft updates of target actor k and target critic k.  The other actor, the other critic and their targets are not written."""
        with torch.no_grad():
            z = torch.randn_like(a) if noise is None else noise
            nz = (z * self.policy_noise).clamp(-self.noise_clip, self.noise_clip)
            a2_1 = (self.target_actor1(s2) + nz).clamp(-self.action_bound, self.action_bound)
            a2_2 = (self.target_actor2(s2) + nz).clamp(-self.action_bound, self.action_bound)
            t = torch.min(self.target_critic1(s2, a2_1), self.target_critic2(s2, a2_2))
            target_q = r + (1 - d) * self.gamma * self._target_value(t)
        if update_a1:
            critic, other, actor, copt, aopt = self.critic1, self.critic2, self.actor1, self.critic1_opt, self.actor1_opt
            t_critic, t_actor = self.target_critic1, self.target_actor1
        else:
            critic, other, actor, copt, aopt = self.critic2, self.critic1, self.actor2, self.critic2_opt, self.actor2_opt
            t_critic, t_actor = self.target_critic2, self.target_actor2
        critic_loss = self._critic_loss(critic(s, a), s, a, other, target_q)
        self._step(critic_loss, copt)
        self._step(neg_mean(critic(s, actor(s))), aopt)
        self._soft_update(actor, t_actor)
        self._soft_update(critic, t_critic)
        return critic_loss.detach()

    def update(self, batch, update_a1=True, noise=None):
        """One update (the reference's `update(transition_dict, update_a1)`); `noise`: [B][action_dim] standard normals in place of the
        draw.  Returns the stepped critic's loss as a 0-dim tensor."""
        self.total_it += 1
        return self._update(*_batch_tensors(batch, self.device), update_a1, noise)

    def train(self, batch, noise=None):
        """The reference's `train`: update k = 1 then update k = 2 on the same batch.  `noise`: a pair of [B][action_dim] tensors of
        standard normals, one per update, in place of the two draws.  Returns the two critic losses (0-dim tensors, no host sync)."""
        n1, n2 = (None, None) if noise is None else noise
        return self.update(batch, True, n1), self.update(batch, False, n2)

    def capture(self, batch_size):
        buf = super().capture(batch_size)
        self._graphs["loss2"] = torch.zeros_like(self._graphs["loss"])
        return buf

    def train_graphed(self, batch):
        """``train`` through the captured graphs: two replays (k = 1, then k = 2) over the static buffers.  Returns the two losses."""
        g = self._graphs
        if g is None:
            raise RuntimeError("%s.train_graphed: call capture(batch_size) first" % type(self).__name__)
        if batch is not g["buf"]:
            for k, v in g["buf"].items():
                v.copy_(batch[k].view_as(v))
        self.total_it += 2
        g["g"][True].replay()
        g["loss2"].copy_(g["loss"])
        g["g"][False].replay()
        return g["loss2"], g["loss"]

    @torch.no_grad()
    def take_action(self, state):
        """DATD3_MLP.take_action (DATD3_mlp.py:88-109) / DARC_MLP.take_action: one state -> np.float32[action_dim], the proposal whose
        OWN critic values it higher (`a1 if q1 >= q2 else a2`), no exploration noise; one host round trip, like the reference.
        Batched and fused: BatchedArmEnv.set_policy_datd3 / set_policy_darc."""
        import numpy as np
        s = torch.tensor(np.asarray([state], dtype=np.float32), device=self.device)
        a1, a2 = self.actor1(s), self.actor2(s)
        q1, q2 = self.critic1(s, a1), self.critic2(s, a2)
        return (a1 if bool(q1 >= q2) else a2).cpu().numpy()[0]

    def policy_state_dicts(self):
        """(actor1, actor2, critic1, critic2) for BatchedArmEnv.set_policy_datd3 / set_policy_darc"""
        return tuple({k: v.detach() for k, v in n.state_dict().items()} for n in self._nets()[:4])


class DARC(DATD3):
    """DARC_MLP: DATD3 whose target mixes min and max of the two target values (both ARE the same min in the reference, so the mix is
    q_weight T + (1 - q_weight) T: two rounded products and a rounded sum, not T) and whose critic k is also pulled towards the other
    critic: loss + regularization_weight mse(critic_k(s, a), critic_other(s, a)).  The other critic is not stepped."""

    def __init__(self, state_dim, action_dim, action_bound, hidden_dim=256, actor_lr=1e-3, critic_lr=1e-3, tau=0.005, gamma=0.98,
                 policy_noise=0.2, noise_clip=0.5, policy_freq=3, q_weight=0.2, regularization_weight=0.005, device="cuda:0"):
        super().__init__(state_dim, action_dim, action_bound, hidden_dim, actor_lr, critic_lr, tau, gamma, policy_noise, noise_clip,
                         policy_freq, device)
        self.q_weight, self.regularization_weight = q_weight, regularization_weight

    def _target_value(self, t):
        return self.q_weight * t + (1.0 - self.q_weight) * t                        # DARC_mlp.py:173: min(T, T), max(T, T)

    def _critic_loss(self, q, s, a, other, target_q):
        with torch.no_grad():      # the reference lets gradient reach the other critic and never steps it with it
            q_other = other(s, a)
        return mean_sq(q - target_q) + self.regularization_weight * mean_sq(q - q_other)      # DARC_mlp.py:182 / :203
