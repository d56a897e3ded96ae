"""Device-resident trajectory store with the reference's HER-"future" sampling (the reference's utils/rl_utils.py:91-199:
Trajectory, ReplayBuffer_Trajectory_reach / _push), fed directly by the [T, N, ...] tensors a rollout produces.  Nothing leaves HBM:
episodes are indexed and batches are gathered by HIP kernels behind the C ABI.

The store is written once, in ``_Store``: the ring and its allocation, the append (``ring_append`` and the segment copies), the
episode index (count, cumsum, write), the sampler's argument struct and ``sample``.  Every tensor carries the leading shape ``_lead``
in front, so the time axis of a ring is ``len(_lead)``.  Two thin classes set ``_lead`` and name the three C calls:

  TrajectoryStore             _lead = ()     armenv_count_episodes / armenv_write_episodes / armenv_her_sample
  PopulationTrajectoryStore   _lead = (P,)   armenv_pop_count_episodes / armenv_pop_write_episodes / armenv_her_pop_sample
                                             (``sample(share_ratio=...)`` other than 0: armenv_her_pop_sample_shared)

The population store (armenv.train_pop) indexes and samples all P members in one launch each.  The single store keeps its own entry
points and kernels: they are what the population kernels are proven against, bit for bit."""
import ctypes as C

import torch

from . import _lib as L


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ring_append(cap, base, T, at_reset, Tc):
    """The ring arithmetic of appending a chunk of ``Tc`` steps to a window of ``T`` logical steps that starts at physical row
    ``base`` of ``cap`` rows: the oldest steps that no longer fit fall out (the window then starts mid-episode).  Returns
    (base, T, at_reset, segments) after the append; segments = [(ring row, chunk row, rows)], one entry, or two where the chunk
    wraps."""
    drop = max(0, T + Tc - cap)                            # oldest steps that fall out of the window
    if drop:
        base = (base + drop) % cap
        T -= drop
        at_reset = False                                   # the window now starts mid-episode
    w = (base + T) % cap                                   # physical row of the first new step
    first = min(Tc, cap - w)
    segments = [(w, 0, first)]
    if first < Tc:
        segments.append((0, first, Tc - first))
    return base, T + Tc, at_reset, segments


class Trajectory:
    """One episode collected step by step on the host, as the reference's single-env loops do
    (utils/rl_utils.py:91-105, call sites main.py:109,128): ``Trajectory(init_state)``,
    ``store_step(action, state, reward, done)``; handed to ``TrajectoryStore.add_trajectory``."""

    def __init__(self, init_state):
        self.states = [init_state]
        self.actions = []
        self.rewards = []
        self.dones = []
        self.length = 0

    def store_step(self, action, state, reward, done):
        self.actions.append(action)
        self.states.append(state)
        self.rewards.append(reward)
        self.dones.append(done)
        self.length += 1


# ring tensor <- the key of the rollout's output dict that feeds it (BatchedEnv.bind_rollout's names)
_RING_SOURCES = dict(obs_after="obs", next_obs="terminal_obs", action="actions", reward="reward", done="done_u8")
_BATCH_KEYS = ("states", "actions", "next_states", "rewards", "dones")


class _Store:
    """What TrajectoryStore and PopulationTrajectoryStore share -- everything but the three C calls (``_count``, ``_write``,
    ``_launch``) and how rollouts reach ``_append``.  ``_ring`` is the ring dict: the geometry (cap, base, T, N, D, at_reset), obs0,
    the five rings [cap][N][...] and the index (counts, offsets, episodes, num_episodes), every tensor with ``_lead`` in front."""

    _lead = ()

    def __init__(self, device, seed, capacity_steps):
        self.device, self.seed, self.capacity = torch.device(device), int(seed), capacity_steps
        self._lib = L.load()
        self._draw = 0
        self._ring = None
        self._bound = None             # (key, out, argument struct) of the last ``sample``; dropped whenever the ring or its index moves
        self._started = False          # the first append has stored obs0

    @property
    def chunk(self):
        """None before the first add, then the indexed ring dict.  Assignable: a store adopts another's ring
        (``PopulationTrajectoryStore.member_view``) this way."""
        return self._ring

    @chunk.setter
    def chunk(self, ring):
        self._ring, self._bound = ring, None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _new(self, shape, dtype):
        return torch.zeros(self._lead + shape, dtype=dtype, device=self.device)

    def _index_buffers(self, cap, N):
        return dict(counts=self._new((N,), torch.int32), offsets=self._new((N,), torch.int64),
                    episodes=self._new((cap * N, 3), torch.int32),                                   # bound: one per step
                    num_episodes=self._new((), torch.int64))

    def _allocate(self, N, D, cap=None):
        """an empty ring of ``capacity`` (or `cap`) steps of N envs with D observations (no row outside the window is ever read)"""
        cap, f32 = int(self.capacity if cap is None else cap), torch.float32
        self.chunk = dict(cap=cap, base=0, T=0, N=N, D=D, at_reset=True, obs0=self._new((N, D), f32),
                          obs_after=self._new((cap, N, D), f32), next_obs=self._new((cap, N, D), f32),
                          action=self._new((cap, N, 3), f32), reward=self._new((cap, N), f32),
                          done=self._new((cap, N), torch.uint8), **self._index_buffers(cap, N))
        return self._ring

    def _append(self, src, obs0, starts_at_reset):
        """Appends the chunk ``src`` (ring key -> tensor ``_lead`` + [Tc][N][...]) to the ring, allocated on the first call, and
        indexes it: the oldest steps fall out.  ``obs0`` and ``starts_at_reset`` are read by the first call only (later windows start
        at rows the ring holds)."""
        ax = len(self._lead)
        Tc, N, D = src["obs_after"].shape[ax:]
        r = self._ring
        if r is None:
            if int(self.capacity) < Tc:
                raise ValueError("capacity_steps smaller than one rollout chunk")
            r = self._allocate(N, D)
        elif (r["N"], r["D"]) != (N, D):
            raise ValueError("%s: the chunk's [N][D] changed" % type(self).__name__)
        if not self._started:
            r["obs0"].copy_(obs0)
            r["at_reset"] = bool(starts_at_reset)
            self._started = True
        r["base"], r["T"], r["at_reset"], segments = ring_append(r["cap"], r["base"], r["T"], r["at_reset"], Tc)
        for k, v in src.items():
            for row, at, rows in segments:
                r[k].narrow(ax, row, rows).copy_(v.narrow(ax, at, rows))
        self._index()

    def _index(self):
        """The episode index of the window: count per env, cumsum within each member, write, num_episodes.  A ring that came without
        an index (a view another store handed over) gets its own buffers."""
        r = self._ring
        if "episodes" not in r:
            r.update(self._index_buffers(r["cap"], r["N"]))
        dev, stream = self.device.index or 0, self._stream()
        geometry = (r["T"], r["N"], r["base"], r["cap"], _p(r["done"]), int(r["at_reset"]), _p(r["counts"]))
        L.check(self._count(dev, geometry, stream))
        torch.cumsum(r["counts"], -1, dtype=torch.int64, out=r["offsets"])
        L.check(self._write(dev, geometry, _p(r["offsets"]), r["episodes"], stream))
        last = r["offsets"][..., -1]                              # i64 _lead: contiguous as it stands where there is one member
        r["num_episodes"] = last if last.is_contiguous() else r["num_episodes"].copy_(last)
        self.chunk = r                                            # T and base moved: the binding goes

    # ---- the store's whole state (armenv.checkpoint)
    def _ring_spec(self, cap, N, D):
        """key -> (shape, dtype) of the ring's saved tensors"""
        lead, f32 = self._lead, torch.float32
        return dict(obs0=(lead + (N, D), f32), obs_after=(lead + (cap, N, D), f32), next_obs=(lead + (cap, N, D), f32),
                    action=(lead + (cap, N, 3), f32), reward=(lead + (cap, N), f32), done=(lead + (cap, N), torch.uint8))

    def state_dict(self):
        """The store's whole state as CPU tensors and plain numbers: the ring's geometry (cap, base, T, N, D, at_reset), obs0 and
        the five rings, the seed, the draw counter and whether the first append has happened.  The episode index is not part of
        it: ``load_state_dict`` makes it again from the ring."""
        r, ring = self._ring, None
        if r is not None:
            ring = {k: int(r[k]) for k in ("cap", "base", "T", "N", "D")}
            ring["at_reset"] = bool(r["at_reset"])
            ring.update({k: r[k].detach().to("cpu", copy=True) for k in self._ring_spec(0, 0, 0)})
        return dict(kind=type(self).__name__, members=(self._lead or (None,))[0], capacity=self.capacity, seed=self.seed,
                    draw=self._draw, started=self._started, ring=ring)

    def load_state_dict(self, sd):
        """Restores ``state_dict()``'s state in place (the rings are allocated here if they are not yet) and indexes the window
        anew; the sampler's binding is dropped.  ValueError naming the first field that does not fit -- kind, members, capacity, the
        ring's N or D where this store already holds one, a tensor's shape -- before anything is changed."""
        who, own = type(self).__name__, self._ring
        for name, mine in (("kind", who), ("members", (self._lead or (None,))[0]), ("capacity", self.capacity)):
            if sd.get(name) != mine:
                raise ValueError("%s.load_state_dict: %s is %r in the state, %r here" % (who, name, sd.get(name), mine))
        ring = sd["ring"]
        if ring is not None:
            cap, N, D = ring["cap"], ring["N"], ring["D"]
            if own is not None:
                for name in ("N", "D"):
                    if own[name] != ring[name]:
                        raise ValueError("%s.load_state_dict: %s is %r in the state, %r here" % (who, name, ring[name], own[name]))
            if not (0 <= ring["base"] < cap and 0 <= ring["T"] <= cap):
                raise ValueError("%s.load_state_dict: base %r, T %r do not fit cap %r" % (who, ring["base"], ring["T"], cap))
            for k, (shape, dt) in self._ring_spec(cap, N, D).items():
                t = ring.get(k)
                if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt:
                    raise ValueError("%s.load_state_dict: %s must be a %s tensor of shape %s, not %s %s"
                                     % (who, k, dt, shape, getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ()))))
            if own is None or own["cap"] != cap or own["obs_after"].device != self.device:
                own = self._allocate(N, D, cap)
            for k in self._ring_spec(cap, N, D):
                own[k].copy_(ring[k])
            own.update(base=int(ring["base"]), T=int(ring["T"]), at_reset=bool(ring["at_reset"]))
        self.seed, self._draw, self._started = int(sd["seed"]), int(sd["draw"]), bool(sd["started"])
        if ring is None:
            self.chunk = None
        else:
            self._ring = own
            self._index()                                         # counts, offsets, episodes, num_episodes: from the ring

    def _batch_spec(self, B):
        """key -> (shape, dtype) of a batch of B rows"""
        lead, D, f32 = self._lead, self._ring["D"], torch.float32
        return dict(states=(lead + (B, D), f32), actions=(lead + (B, 3), f32), next_states=(lead + (B, D), f32),
                    rewards=(lead + (B,), f32), dones=(lead + (B,), torch.uint8))

    def _bind(self, B, use_her, dis_threshold, her_ratio, out):
        """the sampler's argument struct over the ring and ``out``, everything but `draw` and the two picks pointers; its ``.one`` is
        the ArmEnvHerArgs of the single call"""
        r, lead, dev, D = self._ring, self._lead, self.device, self._ring["D"]
        for k, (shape, dt) in self._batch_spec(B).items():
            t = out[k]
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{type(self).__name__}.sample: out[{k!r}] must be a contiguous {dt} tensor of shape {shape} on {dev}")
        args = L.ArmEnvHerPopArgs()
        args.members, args.episodes_stride = (lead or (1,))[0], r["episodes"].shape[-2]
        a = args.one
        a.T, a.N, a.ring_base, a.ring_cap, a.obs_dim, a.use_her = r["T"], r["N"], r["base"], r["cap"], D, int(bool(use_her))
        a.obs0_dev, a.obs_after_dev, a.next_obs_dev = r["obs0"].data_ptr(), r["obs_after"].data_ptr(), r["next_obs"].data_ptr()
        a.action_dev, a.reward_dev, a.done_dev = r["action"].data_ptr(), r["reward"].data_ptr(), r["done"].data_ptr()
        a.episodes_dev, a.num_episodes_dev = r["episodes"].data_ptr(), r["num_episodes"].data_ptr()
        a.batch, a.seed = B, self.seed & 0xFFFFFFFFFFFFFFFF
        a.her_ratio, a.dis_threshold = float(her_ratio), float(dis_threshold)
        a.states_dev, a.actions_dev, a.next_states_dev = out["states"].data_ptr(), out["actions"].data_ptr(), out["next_states"].data_ptr()
        a.rewards_dev, a.dones_dev = out["rewards"].data_ptr(), out["dones"].data_ptr()
        return args

    def sample(self, batch_size, use_her=True, dis_threshold=0.1, her_ratio=0.8, picks=None, return_picks=False, out=None):
        """A batch of B = ``batch_size`` rows (of every member, in one launch) under the reference's keys, as device tensors
        ``_lead`` + [B][...].  ``out`` (optional): a dict of preallocated tensors under the same keys (``batch_buffers`` of a fused
        learner or population, the static buffers of ``TD3.capture``); the batch is then written in place and no memory is allocated.
        ``picks`` i32 ``_lead`` + [B][4]: teacher-forced draws.  ``return_picks``: ``out["picks"]`` i32 ``_lead`` + [B][4]; a tensor
        of that kind already in ``out`` is written in place, by both stores.  The argument struct is built once per (``out``,
        settings, state of the ring); later calls only refresh `draw` and the two picks pointers."""
        return self._sample(batch_size, use_her, dis_threshold, her_ratio, picks, return_picks, out)

    def _sample(self, batch_size, use_her, dis_threshold, her_ratio, picks, return_picks, out, share_ratio=0.0):
        """``sample``'s body.  ``share_ratio`` (the population store's, see its ``sample``): 0.0 is ``sample`` as it stands; any other
        value goes through ``_launch_shared`` with the struct wrapped in an ArmEnvHerPopSharedArgs, and the picks are 5 wide, the
        source member in front."""
        if self._ring is None:
            raise RuntimeError("%s.sample: no rollout stored" % type(self).__name__)
        lead, B, dev, share = self._lead, int(batch_size), self.device, float(share_ratio)
        width = 5 if share else 4                                 # of a pick
        if out is None:
            out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in self._batch_spec(B).items()}
        key = (B, bool(use_her), float(dis_threshold), float(her_ratio), share) + tuple(out[k].data_ptr() for k in _BATCH_KEYS)
        bound = self._bound
        if bound is not None and bound[0] == key and bound[1] is out:
            args = bound[2]
        else:
            args = self._bind(B, use_her, dis_threshold, her_ratio, out)
            if share:
                args = L.ArmEnvHerPopSharedArgs(args, share)
            self._bound = (key, out, args)                        # holds `out`: the pointers in `args` stay valid
        a = args.pop.one if share else args.one
        pk = None
        if picks is not None:
            pk = torch.as_tensor(picks).to(device=dev, dtype=torch.int32).contiguous()
            assert tuple(pk.shape) == lead + (B, width)
        a.picks_dev = None if pk is None else pk.data_ptr()
        if return_picks:
            t = out.get("picks")
            if t is None or tuple(t.shape) != lead + (B, width) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
                out["picks"] = torch.empty(lead + (B, width), dtype=torch.int32, device=dev)
        a.picks_out_dev = out["picks"].data_ptr() if return_picks else None
        a.draw = self._draw
        self._draw += 1
        L.check((self._launch_shared if share else self._launch)(dev.index or 0, args, self._stream()))
        if pk is not None:
            torch.cuda.current_stream(dev).synchronize()
        return out


class TrajectoryStore(_Store):
    """A time-major ring of the last ``capacity_steps`` env steps of N envs (the reference's deque keeps the last
    `capacity` trajectories, rl_utils.py:109-113).  ``size()`` = number of complete episodes currently in the window;
    ``sample(batch_size, use_her, dis_threshold, her_ratio)`` returns device tensors under the reference's keys."""

    def __init__(self, device="cuda:0", seed=0, capacity_steps=None):
        super().__init__(device, seed, capacity_steps)

    def _count(self, dev, geometry, stream):
        return self._lib.armenv_count_episodes(dev, *geometry, stream)

    def _write(self, dev, geometry, offsets, episodes, stream):
        return self._lib.armenv_write_episodes(dev, *geometry, offsets, _p(episodes), stream)

    def _launch(self, dev, args, stream):
        return self._lib.armenv_her_sample(dev, C.byref(args.one), stream)

    def add_rollout(self, obs0, out, actions=None, starts_at_reset=True):
        """Append a rollout chunk.  obs0: observation [N, D] before the chunk's first step (only used when the window
        starts at a reset); out: the dict returned by ``env.rollout(..., want_terminal_obs=True)`` (obs, terminal_obs,
        reward, done_u8, and actions unless `actions` is given).  Without ``capacity_steps`` the store holds exactly
        this chunk (zero-copy); with it, chunks accumulate in a ring and the oldest steps fall out."""
        acts = actions if actions is not None else out["actions"]
        src = dict(obs_after=out["obs"], next_obs=out["terminal_obs"], action=acts, reward=out["reward"], done=out["done_u8"])
        if self.capacity is not None:
            return self._append(src, obs0, starts_at_reset)
        Tc, N, D = src["obs_after"].shape
        self.chunk = dict(cap=Tc, base=0, T=Tc, N=N, D=D, obs0=obs0.contiguous(), at_reset=bool(starts_at_reset),
                          **{k: v.contiguous() for k, v in src.items()})
        self._index()

    def add_trajectory(self, traj):
        """``ReplayBuffer_Trajectory_*.add_trajectory`` (rl_utils.py:112-113) for an episode of ONE env collected on the host: the
        episode becomes a [length, 1, ...] chunk of the device ring (needs ``capacity_steps``).  The episode must end with
        done = True and start at a reset, as the reference's loops produce them (main.py:108-129)."""
        import numpy as np
        if self.capacity is None:
            raise RuntimeError("TrajectoryStore.add_trajectory: construct the store with capacity_steps")
        if traj.length < 1 or not traj.dones[-1]:
            raise ValueError("TrajectoryStore.add_trajectory: a trajectory is one complete episode (last done must be True)")
        dev = self.device
        st = torch.as_tensor(np.asarray(traj.states, dtype=np.float32), device=dev)                    # [L + 1, D]
        out = dict(obs=st[1:, None, :].contiguous(), terminal_obs=st[1:, None, :].contiguous(),
                   reward=torch.as_tensor(np.asarray(traj.rewards, dtype=np.float32), device=dev)[:, None].contiguous(),
                   done_u8=torch.as_tensor(np.asarray(traj.dones, dtype=np.uint8), device=dev)[:, None].contiguous())
        acts = torch.as_tensor(np.asarray(traj.actions, dtype=np.float32), device=dev)[:, None, :].contiguous()
        first = self._ring is None
        if not first:
            # The sampler reads an episode's first state from obs_after of the step before it (auto-reset semantics: the observation
            # after a finishing step is the next episode's first one) and only the window's very first episode from obs0.  A host
            # trajectory brings its own first state: write it where the kernel looks for it, over the previous episode's last
            # obs_after row (that episode's own last next_state lives in next_obs and is not touched).  (without this
            # every episode after the first started, for the sampler, at the previous episode's terminal observation.)
            r = self._ring
            if r["N"] != 1 or r["T"] < 1:
                raise RuntimeError("TrajectoryStore.add_trajectory: the ring holds a batched rollout, not single-env trajectories")
            r["obs_after"][(r["base"] + r["T"] - 1) % r["cap"], 0].copy_(st[0])
        self.add_rollout(st[0:1].contiguous(), out, actions=acts, starts_at_reset=first)

    def size(self):
        """number of complete episodes in the window (host sync)"""
        return 0 if self._ring is None else int(self._ring["num_episodes"].item())


class PopulationTrajectoryStore(_Store):
    """The trajectory stores of P members that run in lockstep (armenv.train_pop): P rings of one geometry, stacked
    [P][capacity_steps][N][...], with one episode index [P][capacity_steps * N][3] and one count i64 [P].  The members' rollouts write
    straight into the store's staging block (``rollout_buffers``); ``add_rollouts`` moves it into the rings and indexes every member,
    ``sample`` draws every member's batch, each in one launch.  Member p draws with ``seed + p``, and every ``sample`` advances one
    shared draw counter: member p's ring, index and batches are, bit for bit, those of a ``TrajectoryStore(seed=seed + p)`` that is
    given member p's rollouts and sampled as often.  Everything is allocated on the first ``add_rollouts``."""

    def __init__(self, members, device="cuda:0", seed=0, capacity_steps=None):
        if not 1 <= int(members) <= 64:
            raise ValueError("PopulationTrajectoryStore: members must be 1..64")
        if capacity_steps is None or int(capacity_steps) < 1:
            raise ValueError("PopulationTrajectoryStore: capacity_steps (the rows of every member's ring) is required")
        super().__init__(device, seed, int(capacity_steps))
        self.members = int(members)
        self._lead = (self.members,)
        self._staging = None

    def _count(self, dev, geometry, stream):
        return self._lib.armenv_pop_count_episodes(dev, self.members, *geometry, stream)

    def _write(self, dev, geometry, offsets, episodes, stream):
        return self._lib.armenv_pop_write_episodes(dev, self.members, *geometry, offsets, _p(episodes), episodes.shape[1], stream)

    def _launch(self, dev, args, stream):
        return self._lib.armenv_her_pop_sample(dev, C.byref(args), stream)

    def _launch_shared(self, dev, args, stream):
        return self._lib.armenv_her_pop_sample_shared(dev, C.byref(args), stream)

    def sample(self, batch_size, use_her=True, dis_threshold=0.1, her_ratio=0.8, picks=None, return_picks=False, out=None,
               share_ratio=0.0):
        """``_Store.sample`` for every member in one launch.  ``share_ratio`` in [0, 1]: the probability that a row of a member's
        batch is drawn from the trajectories of ALL members (a shared replay buffer: uniform over the union of their episodes)
        and not from its own; the draw rule is armenv_her_pop_sample_shared's in include/armenv.h.  0.0 (the default) is the call
        without the argument: the same entry point, bytes and picks [P][B][4].  Any other value: ``picks`` and ``out["picks"]``
        are [P][B][5] = (source member, episode within it, step_state, use_her, step_goal).  The draw counter advances by one
        either way.  ValueError for a value outside [0, 1] or NaN, before any device call."""
        share = float(share_ratio)
        if not 0.0 <= share <= 1.0:
            raise ValueError("PopulationTrajectoryStore.sample: share_ratio must be in [0, 1], not %r" % (share_ratio,))
        return self._sample(batch_size, use_her, dis_threshold, her_ratio, picks, return_picks, out, share)

    def rollout_buffers(self, steps, N, D):
        """P dicts, member p's being contiguous views [steps][N][...] into one stacked staging block [P][steps][N][...], under the
        keys ``BatchedEnv.bind_rollout`` looks up: pass member p's as ``out=`` and its rollout writes straight into the block."""
        T, f32, u8 = int(steps), torch.float32, torch.uint8
        self._staging = dict(obs=self._new((T, N, D), f32), reward=self._new((T, N), f32), done_u8=self._new((T, N), u8),
                             success_u8=self._new((T, N), u8), actions=self._new((T, N, 3), f32), terminal_obs=self._new((T, N, D), f32))
        return [{k: t[p] for k, t in self._staging.items()} for p in range(self.members)]

    def add_rollouts(self, obs0, starts_at_reset=True):
        """Appends the staging block -- every member's last rollout -- to the rings and indexes every member.  obs0 f32 [P][N][D]:
        the members' observations before the chunk's first step (read on the first call only: later windows start at rows the ring
        holds)."""
        stage = self._staging
        if stage is None:
            raise RuntimeError("PopulationTrajectoryStore.add_rollouts: call rollout_buffers(steps, N, D) and roll out into them first")
        P, _, N, D = stage["obs"].shape
        if not self._started and tuple(obs0.shape) != (P, N, D):
            raise ValueError("PopulationTrajectoryStore.add_rollouts: obs0 must be [%d][%d][%d]" % (P, N, D))
        self._append({k: stage[name] for k, name in _RING_SOURCES.items()}, obs0, starts_at_reset)

    def sizes(self):
        """the members' numbers of complete episodes in the window: a list of P ints from one device-to-host transfer"""
        return [0] * self.members if self._ring is None else self._ring["num_episodes"].tolist()

    def ready(self, minimal_episodes):
        """armenv.train_pop's lockstep rule: EVERY member holds ``minimal_episodes`` complete episodes (one transfer)"""
        return min(self.sizes()) >= minimal_episodes

    def member_view(self, p):
        """member p's ring as the dict ``TrajectoryStore.chunk`` holds: views, no copy"""
        r = self._ring
        if r is None:
            raise RuntimeError("PopulationTrajectoryStore.member_view: no rollout stored")
        view = {k: r[k] for k in ("cap", "base", "T", "N", "D", "at_reset")}
        view.update({k: r[k][p] for k in ("obs0", "episodes") + tuple(_RING_SOURCES)})
        view["num_episodes"] = r["num_episodes"][p:p + 1]
        return view
