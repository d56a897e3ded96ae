"""Population-based training (Jaderberg et al. 2017, arXiv:1711.09846) for the populations of fused learners: the schedule that says
who is replaced by whom (``plan``: truncation selection -- exploit) and what the replaced members' hyper-parameters become
(``explore``: perturb).  Host-only: pure functions of their arguments and of one ``random.Random``, so a run is a function of `seed`
alone.  The copies themselves are ``FusedPopulation.exploit`` (ONE launch, armenv_pop_exploit); armenv.train_pop drives both
(``train_reach_population(pbt=...)``, ``--pbt-every``).

    sched = PBTSchedule(every=10).bind(pop.sweepable() + ("expl_sigma",))
    src, new = sched.step(fitness, rows)          # rows[p]: member p's values, a dict over the bound names at least
    pop.exploit(src); [pop.set_hyper(p, **values) for p, values in new.items()]

Draw order of one ``step``: all of ``plan``'s draws (one ``randrange`` per member of the bottom, ascending), then, for the replaced
members ascending, one ``random`` per name in ``names`` order."""
import math
import random

from ._lib import ArmEnvPopHyper
from .fused_pop_base import _UNIT_RANGE

KNOWN_NAMES = tuple(name for name, _ in ArmEnvPopHyper._fields_) + ("expl_sigma",)     # what any agent may let a member own
_NOT_BY_DEFAULT = ("gamma",)      # the discount defines the task's return: not perturbed unless asked for by name


class PBTSchedule:
    """``every``: a PBT step after every that many iterations.  ``fraction``: the share of the population that is the bottom (and
    the top) of a step, in (0, 0.5] so that the two never meet.  ``perturb``: the two factors of ``explore``.  ``names``: the
    hyper-parameters that ``explore`` perturbs; None: once bound to an agent, every name the agent lets a member own except gamma
    -- and the rollout's ``expl_sigma``.  ValueError: every < 1, a fraction outside (0, 0.5], a factor that is <= 0 or not
    finite, a name that no agent knows (here) or that the agent does not have (``bind``)."""

    def __init__(self, every, fraction=0.25, perturb=(0.8, 1.2), names=None, seed=0):
        if isinstance(every, bool) or int(every) != every or every < 1:
            raise ValueError("PBTSchedule: every = %r must be an integer >= 1" % (every,))
        fraction = float(fraction)
        if not 0.0 < fraction <= 0.5:                       # NaN fails
            raise ValueError("PBTSchedule: fraction = %r outside (0, 0.5]" % (fraction,))
        try:
            lo, hi = (float(v) for v in perturb)
        except (TypeError, ValueError):
            raise ValueError("PBTSchedule: perturb = %r must be two factors" % (perturb,)) from None
        for v in (lo, hi):
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError("PBTSchedule: perturb factor %r must be finite and > 0" % (v,))
        if names is not None:
            names = (names,) if isinstance(names, str) else tuple(names)
            for name in names:
                if name not in KNOWN_NAMES:
                    raise ValueError("PBTSchedule: %s is not one of %s" % (name, ", ".join(KNOWN_NAMES)))
        self.every, self.fraction, self.perturb, self.names, self.seed = int(every), fraction, (lo, hi), names, seed
        self.rng = random.Random(seed)

    def bind(self, allowed):
        """Settles ``names`` for an agent whose members may own `allowed` (``train_pop.sweepable_names(algo)``): the default, or
        the given names checked against it.  Returns self."""
        allowed = tuple(allowed)
        if self.names is None:
            self.names = tuple(n for n in allowed if n not in _NOT_BY_DEFAULT)
        for name in self.names:
            if name not in allowed:
                raise ValueError("PBTSchedule: %s is not one of the agent's %s" % (name, ", ".join(allowed)))
        return self

    def state_dict(self):
        """The schedule as plain numbers, strings and lists: the constructor's arguments, the bound names and the generator's
        state -- what ``step`` will draw next (armenv.checkpoint)."""
        version, words, gauss = self.rng.getstate()
        return dict(kind=type(self).__name__, every=self.every, fraction=self.fraction, perturb=list(self.perturb), seed=self.seed,
                    names=None if self.names is None else list(self.names), rng=[version, list(words), gauss])

    def load_state_dict(self, sd):
        """Continues the saved schedule's draws: takes its bound names and its generator's state.  The constructor's arguments
        must be the saved ones: ValueError naming the first that is not, before anything is changed."""
        for name, mine in (("kind", type(self).__name__), ("every", self.every), ("fraction", self.fraction),
                           ("perturb", list(self.perturb)), ("seed", self.seed)):
            if sd.get(name) != mine:
                raise ValueError("PBTSchedule.load_state_dict: %s is %r in the state, %r here" % (name, sd.get(name), mine))
        names = None if sd["names"] is None else tuple(sd["names"])
        for name in names or ():
            if name not in KNOWN_NAMES:
                raise ValueError("PBTSchedule.load_state_dict: %s is not one of %s" % (name, ", ".join(KNOWN_NAMES)))
        version, words, gauss = sd["rng"]
        state = (int(version), tuple(int(w) for w in words), gauss)
        random.Random().setstate(state)                      # a malformed state raises here, before this schedule is touched
        self.names = names
        self.rng.setstate(state)

    def due(self, iteration):
        """whether a PBT step follows iteration `iteration` (counted from 1)"""
        return iteration % self.every == 0

    def plan(self, fitness):
        """Truncation selection over one fitness per member (higher is better; NaN ranks last): ``src`` with ``src[p]`` the member
        that p becomes a copy of, p itself for a member that stays.  The members are ranked by fitness descending, ties by the
        lower index; n = max(1, int(P * fraction)) for P >= 2, else 0.  Each of the bottom n, in ascending member order, draws
        ``k = rng.randrange(n)`` and takes the k-th best as its source -- and is replaced only if the source's fitness is strictly
        greater, so nothing churns while all members are level.  The top and the bottom are disjoint: src[src[p]] == src[p]."""
        f = [-math.inf if v != v else float(v) for v in fitness]
        P = len(f)
        order = sorted(range(P), key=lambda p: (-f[p], p))
        n = max(1, int(P * self.fraction)) if P >= 2 else 0
        src = list(range(P))
        for p in sorted(order[P - n:]) if n else ():
            s = order[self.rng.randrange(n)]
            if f[s] > f[p]:
                src[p] = s
        return src

    def explore(self, row):
        """`row` (a member's values by name) with each of ``names``, in order, multiplied by ``perturb[0]`` if ``rng.random() <
        0.5``, else by ``perturb[1]``; a name whose range is [0, 1] (tau, gamma, q_weight) is then clipped to 1.  A new dict."""
        if self.names is None:
            raise ValueError("PBTSchedule.explore: bind(...) the schedule to an agent's names first")
        out = dict(row)
        for name in self.names:
            value = out[name] * (self.perturb[0] if self.rng.random() < 0.5 else self.perturb[1])
            out[name] = min(value, 1.0) if name in _UNIT_RANGE else value
        return out

    def step(self, fitness, rows):
        """One PBT step: ``(src, new)`` with ``src = plan(fitness)`` and ``new[p]``, for each replaced member p ascending, its
        source's row explored.  `rows` is left as it is."""
        src = self.plan(fitness)
        return src, {p: self.explore(rows[s]) for p, s in enumerate(src) if s != p}
