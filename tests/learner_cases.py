"""The cases of tests/test_gpu_td3_ref64.py and tests/test_gpu_da_ref64.py, built on the CPU (test infrastructure): every input of a
fused TD3 / DADDPG / DATD3 / DARC update that is compared with tests/learner_ref64.py -- parameters, perturbed targets, non-zero Adam
moments, step counters, the batch and the noise -- comes from CPU generators as f32 tensors and is then moved to the device, so that
tests/test_td3_ref64.py and tests/test_da_ref64.py can evaluate the reference on exactly those inputs without a GPU (the share of
ambiguous relu units must stay under AMB_MAX, or the allowance would make a comparison vacuous)."""
import numpy as np
import torch

import learner_ref64 as R

AGENTS = R.AGENTS
AMB_MAX = 1e-3          # at most this share of relu units may be ambiguous: a condition on the inputs, not a measurement
KEYS = ("states", "actions", "next_states", "rewards", "dones")
# step counters before the update, one per optimiser and all different, so that a counter read from the wrong net shows
STEPS = dict(actor=4, actor1=4, actor2=6, critic=3, critic1=3, critic2=5)

HP = dict(action_bound=0.7, gamma=0.98, tau=0.005, actor_lr=1e-3, critic_lr=1e-3, beta1=0.0, beta2=0.999, eps=1e-8, policy_noise=0.2,
          noise_clip=0.5, q_weight=0.2, regularization_weight=0.005)
# hyper-parameters under which every defect of learner_ref64.DEFECTS changes something: noise clip and action clamp bind on many
# elements (target actions of order one through `gain`), and a third of the rows are terminal; a regulariser of the TD term's order
HP_DEFECT = dict(action_bound=0.25, policy_noise=0.4, noise_clip=0.1, regularization_weight=0.5)
# the noise reaches the proposals unclipped and unclamped: |z| <= sqrt(-2 ln 2^-24) = 5.8, so |noise| < noise_clip, and
# |bound tanh(u) + noise| < bound for the small u of a fresh target actor (the GPU test asserts both).  DATD3: tau = 0, so that the
# second update of a train (critic 2, actor 2) reads nothing that the first one wrote.  TD3 keeps the values it has always had: a
# bound of 8 under noise of 0.5 gives the target critics' inputs magnitudes far above their values, and with them about 8e-4 of
# ambiguous relu units
HP_NOISE = dict(td3=dict(action_bound=8.0, policy_noise=0.5, noise_clip=5.0),
                datd3=dict(action_bound=1.0, policy_noise=0.12, noise_clip=0.8, tau=0.0))


def hp32(agent, **kw):
    """the hyper-parameters of `agent` as the f32 values the kernel sees"""
    hp = dict(HP)
    hp.update(kw)
    return {k: float(np.float32(hp[k])) for k in R.HP_KEYS[agent]}


def make_case(agent, k, B, D, seed, tag, hp=None, steps=None, gain=1.0, done_p=0.1, dones=None, noise="randn", lone_feature=False,
              twin_targets=False, with_actor=True):
    """a case: `k` is the actor (and for DATD3 / DARC the critic) that the update steps, None for TD3, whose `with_actor` says
    whether the update takes the delayed actor step.  `noise`: "randn", None (DADDPG; in-kernel noise) or ("kernel", seed, draw);
    `dones`: 0 / 1 sets every done flag; lone_feature: state feature 0 is zero except on row B // 2; twin_targets: target critic 2 is
    a perturbed copy of target critic 1, so that the min picks either proposal on many rows"""
    assert (k is None) == (agent == "td3") and (with_actor or agent == "td3"), (agent, k, with_actor)
    return dict(agent=agent, k=k, with_actor=with_actor, B=B, D=D, seed=seed, tag=tag, hp=hp32(agent, **(hp or {})),
                steps=dict(STEPS, **(steps or {})), gain=gain, done_p=done_p, dones=dones, noise=None if agent == "daddpg" else noise,
                lone_feature=lone_feature, twin_targets=twin_targets)


def case_id(c):
    return "%s-%s-%s" % (c["agent"], "k%d" % c["k"] if c["k"] else "actor" if c["with_actor"] else "noactor", c["tag"])


def stepped(c):
    """the names of the critic and the actor that the update of case `c` steps (TD3's actor: on its delayed steps only)"""
    if c["agent"] == "td3":
        return "critic", "actor"
    return "critic" if c["agent"] == "daddpg" else "critic%d" % c["k"], "actor%d" % c["k"]


def _mlp(g, n_in, n_out, hidden=256):
    """six tensors in parameters() order, each uniform in +-1 / sqrt(fan_in) as torch.nn.Linear draws them"""
    out = []
    for fan_in, fan_out in ((n_in, hidden), (hidden, hidden), (hidden, n_out)):
        b = 1.0 / np.sqrt(fan_in)
        out += [(torch.rand(fan_out, fan_in, generator=g) * 2 - 1) * b, (torch.rand(fan_out, generator=g) * 2 - 1) * b]
    return out


def build(c):
    """the inputs of case `c` as f32 (dones uint8) CPU tensors: nets {name: tensors in parameters() order} over learner_ref64.NETS
    (TD3's twin critic: twelve), moments {name: (m, v)}, steps, batch, noise ([B, 3] or None)"""
    agent, B, D = c["agent"], c["B"], c["D"]
    g = torch.Generator().manual_seed(c["seed"])
    nets = {}
    for name in R.LEARNING[agent]:
        nets[name] = _mlp(g, D, 3) if name.startswith("actor") else _mlp(g, D + 3, 1) + (_mlp(g, D + 3, 1) if agent == "td3" else [])
    for name in R.LEARNING[agent]:
        nets["target_" + name] = [p + torch.randn(p.shape, generator=g) * 0.02 * p.abs().mean() for p in nets[name]]
    for name in R.NETS[agent]:
        if name.startswith("target_actor"):
            nets[name][4] = nets[name][4] * c["gain"]
    if c["twin_targets"] and agent in ("datd3", "darc"):
        nets["target_critic2"] = [p + torch.randn(p.shape, generator=g) * 0.02 * p.abs().mean() for p in nets["target_critic1"]]
    moments = {name: ([torch.randn(p.shape, generator=g) * 1e-3 for p in nets[name]],
                      [torch.rand(p.shape, generator=g) * 1e-6 for p in nets[name]]) for name in R.LEARNING[agent]}
    batch = dict(states=torch.rand(B, D, generator=g), actions=torch.rand(B, 3, generator=g) * 1.4 - 0.7,
                 next_states=torch.rand(B, D, generator=g), rewards=torch.rand(B, generator=g) - 0.5,
                 dones=(torch.rand(B, generator=g) < c["done_p"]).to(torch.uint8))
    if c["dones"] is not None:
        batch["dones"].fill_(c["dones"])
    if c["lone_feature"]:
        batch["states"][:, 0] = 0.0
        batch["states"][B // 2, 0] = 1.0
    noise = None
    if c["noise"] == "randn":
        noise = torch.randn(B, 3, generator=g)
    elif c["noise"] is not None:
        noise = torch.from_numpy(R.kernel_noise(c["noise"][1], c["noise"][2], np.arange(B)))          # float64, as the host restates it
    return dict(nets=nets, moments=moments, steps={n: c["steps"][n] for n in R.LEARNING[agent]}, batch=batch, noise=noise)


def state64(c, built, device=None):
    return R.state_from(c["agent"], built["nets"], built["moments"], built["steps"], device=device)


def batch64(built, device=None):
    return {k: v.to(device=device, dtype=torch.float64) for k, v in built["batch"].items()}


def noise64(built, device=None):
    return None if built["noise"] is None else built["noise"].to(device=device, dtype=torch.float64)


def reference(c, built, device=None, **kw):
    """learner_ref64's update of case `c` on the inputs `built`"""
    kw = dict(dict(k=c["k"], with_actor=c["with_actor"]), **kw)
    return R.update(c["agent"], state64(c, built, device), batch64(built, device), noise64(built, device), c["hp"], **kw)


# ---- the cases ----

GRAD_SHAPES = [(B, 6) for B in (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 1000, 2048, 4097)] + \
              [(B, D) for D in (1, 3, 9, 12) for B in (5, 257)]
TD3_GRAD_SHAPES = GRAD_SHAPES + [(65536, 6)] + [(2048, D) for D in (1, 3, 9, 12)]
AGENT_K = [("td3", None)] + [(agent, k) for agent in AGENTS[1:] for k in (1, 2)]
SEED_K = {None: 7, 1: 1, 2: 2}


def grad_case(agent, k, B, D, **kw):
    return make_case(agent, k, B, D, seed=1000 * SEED_K[k] + 13 * B + D, tag="B%d-D%d" % (B, D), **kw)


# TD3 takes every shape also without the actor step (through a policy_freq that never fires), on the same inputs
GRAD_CASES = [grad_case("td3", None, B, D, with_actor=wa) for B, D in TD3_GRAD_SHAPES for wa in (True, False)] + \
             [grad_case(agent, k, B, D) for agent, k in AGENT_K[1:] for B, D in GRAD_SHAPES]
LARGEST_CASE = grad_case("td3", None, 1 << 20, 6)          # kMaxBatch; too long for the CPU tests, so in no list
DEFECT_CASES = [make_case("td3", None, B, 6, seed=2007 + B, tag="defects-B%d" % B, hp=HP_DEFECT, gain=30.0, done_p=0.3,
                          steps={n: 0 for n in STEPS}) for B in (65, 257, 2048)] + \
               [make_case(agent, k, B, 6, seed=2000 + B + k, tag="defects-B%d" % B, hp=HP_DEFECT, gain=100.0, done_p=0.3,
                          steps={n: 0 for n in STEPS}, twin_targets=True) for agent, k in AGENT_K[1:] for B in (65, 257)]
ADAM_STEPS = (1, 2, 10, 10 ** 6)
EDGES = dict(gamma_0=dict(hp=dict(gamma=0.0)), gamma_1=dict(hp=dict(gamma=1.0)), dones_all_0=dict(dones=0), dones_all_1=dict(dones=1),
             clamp_binds=dict(hp=dict(action_bound=0.05)), reg_1=dict(hp=dict(regularization_weight=1.0)))


def adam_case(agent, k, step, side):
    """default betas; the actor's side with critic_lr = 0, so that its beta1 = 0 twin sees the same critic"""
    hp = dict(beta1=0.9, **(dict(critic_lr=0.0) if side == "actor" else {}))
    return make_case(agent, k, 257, 6, seed=3000 + step % 997 + SEED_K[k], tag="adam-step%d-%s" % (step, side), hp=hp,
                     steps={n: step - 1 for n in STEPS})


def edge_cases(agent, k):
    names = [n for n in EDGES if not (n == "clamp_binds" and agent == "daddpg") and not (n == "reg_1" and agent != "darc")]
    return [make_case(agent, k, 257, 6, seed=4000 + SEED_K[k], tag="edge-" + n, **EDGES[n]) for n in names]


ADAM_CASES = [adam_case(agent, k, step, side) for agent, k in AGENT_K for step in ADAM_STEPS for side in ("critic", "actor")]
EDGE_CASES = [c for agent, k in AGENT_K for c in edge_cases(agent, k)]
NOISE_AGENTS = ("td3", "datd3")
NOISE_PARAMS = [(B, seed, draw) for B in (1, 65, 2048) for seed in (0, (1 << 32) + 5) for draw in (1, (1 << 32) + 1)]


def noise_cases(agent, B, seed, draw):
    """the updates of one `train` whose first update has the draw `draw`.  TD3: the one update, without the actor step.  DATD3:
    update 1 and update 2, which uses the next draw"""
    return [make_case(agent, k, B, 6, seed=5000 + B, tag="noise-B%d-s%d-d%d" % (B, seed, draw), hp=HP_NOISE[agent], done_p=0.0,
                      noise=("kernel", seed, draw + i), lone_feature=True, with_actor=agent != "td3")
            for i, k in enumerate((None,) if agent == "td3" else (1, 2))]


NOISE_CASES = [c for agent in NOISE_AGENTS for B, seed, draw in NOISE_PARAMS for c in noise_cases(agent, B, seed, draw)]

# the bit-for-bit edges (B = 65: two gemm tiles, one slice), default betas
EXACT = dict(lr_0=dict(hp=dict(actor_lr=0.0, critic_lr=0.0)), tau_0=dict(hp=dict(tau=0.0)), tau_1=dict(hp=dict(tau=1.0)),
             all_done=dict(dones=1), noise_clip_0=dict(hp=dict(noise_clip=0.0)), policy_noise_0=dict(hp=dict(policy_noise=0.0)),
             as_datd3_q0=dict(hp=dict(regularization_weight=0.0, q_weight=0.0)),
             as_datd3_q1=dict(hp=dict(regularization_weight=0.0, q_weight=1.0)))


def exact_case(agent, k, name):
    kw = dict(EXACT[name])
    # TD3's two noise cases keep the 257 rows they have always had
    B = 257 if agent == "td3" and name in ("noise_clip_0", "policy_noise_0") else 65
    return make_case(agent, k, B, 6, seed=6000 + SEED_K[k], tag="exact-" + name, hp=dict(beta1=0.9, **kw.pop("hp", {})), **kw)


def exact_names(agent):
    return [n for n in EXACT if not (n.endswith("noise_0") and agent == "daddpg") and not (n.startswith("as_datd3") and agent != "darc")]


EXACT_CASES = [exact_case(agent, k, n) for agent, k in AGENT_K for n in exact_names(agent)]
ALL_CASES = GRAD_CASES + DEFECT_CASES + ADAM_CASES + EDGE_CASES + NOISE_CASES + EXACT_CASES


def amb_capped(c):
    """whether AMB_MAX is asserted on case `c`.  TD3's noise cases are exempt, as they have always been: their comparison is between
    two kernel runs, the reference supplies magnitudes only (no allowance enters the bound), and under TD3's HP_NOISE the share is
    about 8e-4, so at B = 1 (2560 units) the cap would hold or fail by seed"""
    return not (c["agent"] == "td3" and c["tag"].startswith("noise-"))


def target_actions(st, batch, noise, hp, clamp=True):
    """the proposals of TD3 (one) or DATD3 / DARC (two) over a float64 state, restated without learner_ref64 (for the assertions
    that a clamp binds)"""
    out = []
    for name in ("target_actor", "target_actor1", "target_actor2"):
        if name in st:
            TA = st[name]
            h = torch.relu(torch.relu(batch["next_states"] @ TA[0].T + TA[1]) @ TA[2].T + TA[3])
            a = hp["action_bound"] * torch.tanh(h @ TA[4].T + TA[5]) + (noise * hp["policy_noise"]).clamp(-hp["noise_clip"], hp["noise_clip"])
            out.append(a.clamp(-hp["action_bound"], hp["action_bound"]) if clamp else a)
    return out


def pick_share(agent, st, batch, noise, hp):
    """the share of rows on which the min under the target takes the FIRST of its two values, restated without learner_ref64"""
    def q(p, s, a):
        h = torch.relu(torch.relu(torch.cat([s, a], 1) @ p[0].T + p[1]) @ p[2].T + p[3])
        return h @ p[4].T + p[5]
    if agent == "daddpg":
        acts = target_actions(st, batch, torch.zeros_like(batch["actions"]), dict(hp, policy_noise=0.0, noise_clip=0.0), clamp=False)
        tq = [q(st["target_critic"], batch["next_states"], a) for a in acts]
    elif agent == "td3":
        a = target_actions(st, batch, noise, hp)[0]
        tq = [q(st["target_critic"][i:i + 6], batch["next_states"], a) for i in (0, 6)]
    else:
        tq = [q(st["target_critic%d" % (j + 1)], batch["next_states"], a) for j, a in enumerate(target_actions(st, batch, noise, hp))]
    return float((tq[0] <= tq[1]).double().mean())
