"""Adversary search: find HO schedules under which an algorithm violates its
Spec, shrink them, and save them as replayable counterexamples (SURVEY §8f
rank 4: "makes the executor a bug-finder; uses livenessPredicate /
safetyPredicate as schedule constraints").

The reference proves its algorithms with the z3 verifier under the Spec's
environment assumptions (psync/verification/Verifier.scala:145-168: the
`safetyPredicate` conjoined to every transition, a `livenessPredicate` to the
rounds of a progress step). Here the same assumptions constrain explicit HO
schedules (round_amd/schedules.py) and the GPU executes and checks
populations of them per launch (psg_load_schedule + psg_run_batch), so a
search is one loop (Adversary.search) of: run a population on the device, keep
the schedules that get closest to a violation, mutate them. Where the
population lives is behind one interface: _HostPopulation generates and mutates
with numpy and uploads every generation, _DevicePopulation keeps it in HBM
(psg_population_*: the general-omission safety search always, the crash family
and the liveness search with device_models=True).

  * safety search: schedules satisfy the safety predicate on their HO sets;
    a violation of a target check slot is genuine only while the predicate
    also held on the *effective* HO sets (slot "SafetyPredicate", halted
    senders send nothing, psync/Round.scala:42-55), i.e. first_fail[target] <
    first_fail[SafetyPredicate].
  * liveness search (mode="liveness"): schedules satisfy the liveness
    predicate in at least `live_rounds` rounds; the target is non-termination
    within R rounds (term_round == never).
  * fault models: general omission (OTR, OTR2, LastVoting, ShortLastVoting,
    BenOr, EpsilonConsensus, TwoPhaseCommit, LatticeAgreement) or crash-stop with at most f crashes (FloodMin,
    KSetAgreement, KSetEarlyStopping — their runners' fault model).
Every counterexample is shrunk (batched delta debugging: all candidate
simplifications of one step run as one GPU batch). One driver holds the plan
and the selection rule (Adversary._shrink_plan); a step of it either builds the
candidates on the host (schedules.shrink_candidates) or, with
device_shrink=True, on the device (psg_shrink_*, only the shrunk schedule comes
back). Counterexamples can be written to a .psgr file (round_amd/records.py)
that `records.replay` re-executes.
"""
import time
from dataclasses import dataclass, field, replace
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import abi, psync, records, schedules as S

NEVER = abi.PSG_NEVER

# The generators' constants: the host generators use them as they are, the device ones
# (psg_population_params / psg_population_model) in /256 fixed point.
LOSS_SPREAD = (0.7, 0.85, 1.0, 1.15)       # a fresh population's loss rates around `keep`, one per quarter
CRASH_DELIVERY = (0.05, 0.15, 0.5, 0.85)   # crash family: densities of the crash-round deliveries
FLIP_STRENGTH = 0.01                       # links flipped in a mutant, as a share of n * R (at least one)
INIT_REDRAW = 0.02                         # share of a mutant's initial values drawn again
CRASH_MUTATE = 0.3                         # schedules.mutate_crash: move and add w.p. this each, drop w.p. half


def _p256(p: float) -> int:
    return int(round(p * 256))


# ------------------------------------------------------------------ evaluation

@dataclass
class Eval:
    """Outcome of a batch of explicit-schedule instances (numpy, one row per instance)."""
    summary: np.ndarray      # records.SUMMARY_DTYPE [I]
    decision: np.ndarray     # [I][n] int32 (float64 for EpsilonConsensus)
    decision_round: np.ndarray  # [I][n] int32, -1 = none

    @property
    def first_fail(self):
        return self.summary["first_fail"]


class GpuEvaluator:
    """Runs explicit-schedule batches on one MI355X through the C ABI."""

    def __init__(self, alg: psync.Algorithm, n: int, rounds: int, capacity: int, device: int = 0,
                 value_range: Optional[int] = None, seed: int = 1, tiebreak: int = abi.PSG_TIE_CHAMP):
        self.gr = psync.GpuRound(alg, n, rounds, seed=seed, value_range=value_range, tiebreak=tiebreak,
                                 device=device, batch_capacity=capacity)
        self.cfg = self.gr.cfg
        self.capacity = capacity

    def __call__(self, inst_begin: int, ho: np.ndarray, crash: Optional[np.ndarray], init: np.ndarray) -> Eval:
        I = ho.shape[0]
        outs = []
        for a in range(0, I, self.capacity):
            b = min(I, a + self.capacity)
            ctx = self.gr._ctx
            ctx.load_inputs(inst_begin + a, b - a, init[a:b])
            ctx.load_schedule(inst_begin + a, b - a, ho[a:b], None if crash is None else crash[a:b])
            _, pi = ctx.run_batch_np(inst_begin + a, b - a)
            dec, dr = ctx.copy_decisions_np()
            outs.append((pi, dec, dr))
        return Eval(np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]),
                    np.concatenate([o[2] for o in outs]))

    def close(self):
        self.gr.close()


# ------------------------------------------------------------------ fault models per algorithm

@dataclass
class Model:
    family: str                      # "omission" | "crash"
    min_size: Optional[int] = None   # safety predicate |HO(p)| >= min_size (omission family)
    fmax: int = 0                    # crash family: at most fmax crashes
    predicate_slot: Optional[int] = None  # check slot recording the predicate on effective HO sets
    liveness: Optional[str] = None   # "good_round" | "coord_hears_all" | "fixed_coord"
    phase: int = 4                   # coordinator period (coord = (r / phase) % n)
    coord: int = 0                   # "fixed_coord": the coordinator of every phase


# Model.liveness -> enum psg_pop_live
LIVE_KIND = {"good_round": abi.PSG_LIVE_GOOD_ROUND, "coord_hears_all": abi.PSG_LIVE_COORD_HEARS_ALL,
             "fixed_coord": abi.PSG_LIVE_FIXED_COORD}


def default_model(alg: psync.Algorithm, n: int) -> Model:
    a = alg.alg_id
    if a in (abi.PSG_ALG_OTR, abi.PSG_ALG_OTR2):
        return Model("omission", liveness="good_round")
    if a in (abi.PSG_ALG_LAST_VOTING, abi.PSG_ALG_SLV):
        return Model("omission", liveness="coord_hears_all", phase=4)  # SLV: coord(r/4) literally
    if a == abi.PSG_ALG_BENOR:
        return Model("omission", min_size=n // 2 + 1, predicate_slot=4)  # BenOr.scala:92
    if a == abi.PSG_ALG_EPSILON:
        return Model("omission", min_size=n - alg.param, predicate_slot=2)  # Epsilon.scala:57
    if a == abi.PSG_ALG_FLOODMIN:
        return Model("crash", fmax=alg.param)
    if a == abi.PSG_ALG_KSET:
        return Model("crash", fmax=alg.param - 1)
    if a == abi.PSG_ALG_KSET_ES:
        return Model("crash", fmax=alg.param)
    if a == abi.PSG_ALG_TPC:
        return Model("omission", liveness="fixed_coord", phase=3, coord=alg.param)  # TwoPhaseCommit.scala:90-92
    if a == abi.PSG_ALG_LATTICE:
        return Model("omission")  # (TrivialSpec: no livenessPredicate to assume, no liveness search)
    raise ValueError(f"no fault model for {alg.class_name}")


def default_init(alg: psync.Algorithm, rng, I: int, n: int, values: int) -> np.ndarray:
    """Initial values: a small domain makes conflicting proposals likely."""
    if alg.real:
        return rng.random((I, n))
    if alg.alg_id == abi.PSG_ALG_BENOR:
        return rng.integers(0, 2, (I, n), dtype=np.int32)
    if alg.alg_id == abi.PSG_ALG_TPC:  # votes io.canCommit, mostly yes: no w.p. 1 / values
        return (rng.integers(0, max(values, 1), (I, n)) != 0).astype(np.int32)
    if alg.alg_id == abi.PSG_ALG_LATTICE:  # subsets of {0..values-1} as bit masks: lattice_init's one or two elements
        v = rng.integers(0, values * values, (I, n))
        return ((1 << (v // values)) | (1 << (v % values))).astype(np.int32)
    return rng.integers(1, values + 1, (I, n), dtype=np.int32)  # nonzero (LastVoting.scala:134)


# ------------------------------------------------------------------ results

@dataclass
class Counterexample:
    inst_id: int
    init: np.ndarray                 # [n]
    ho: np.ndarray                   # [R][n][W]
    crash: Optional[np.ndarray]      # [n] or None
    summary: np.ndarray              # records.SUMMARY_DTYPE scalar
    violated: List[str]              # target slots violated (or ["Termination"])
    check_point: int                 # first check point of the violation
    omitted_links: int = 0           # links missing from the HO sets (self links excluded)

    def same(self, other: "Counterexample") -> bool:
        """The same counterexample bit for bit, every field."""
        def eq(a, b):
            return (a is None) == (b is None) and (a is None or np.array_equal(a, b))
        return bool(self.inst_id == other.inst_id and eq(self.init, other.init) and eq(self.ho, other.ho)
                    and eq(self.crash, other.crash) and self.violated == other.violated
                    and self.check_point == other.check_point and self.omitted_links == other.omitted_links
                    and np.asarray(self.summary).tobytes() == np.asarray(other.summary).tobytes())


@dataclass
class SearchResult:
    counterexamples: List[Counterexample]
    schedules_evaluated: int
    generations: int
    seconds: float
    gpu_seconds: float = 0.0
    history: List[float] = field(default_factory=list)   # best score per generation

    @property
    def schedules_per_second(self):
        return self.schedules_evaluated / self.seconds if self.seconds > 0 else 0.0


# ------------------------------------------------------------------ populations
# What Adversary.search needs of a population: fresh() makes generation 0; evaluate() runs it and
# returns (Eval, valid [P], seconds on the GPU), valid[i] = instance i satisfies the model's
# constraints, and sets `base`, the instance id of row 0; read(rows) returns (init, ho, crash) of
# these rows; advance(elite, parents, n_fresh, generation) replaces it by the elite rows, one
# mutant per parent row and n_fresh fresh schedules, in this order, and returns its GPU seconds.

class _HostPopulation:
    """Genome and initial values as numpy arrays, drawn from the adversary's generator; every
    generation is uploaded and runs under an instance id block of its own."""

    def __init__(self, adv: "Adversary"):
        self.adv = adv

    def fresh(self):
        a = self.adv
        self.genome = a._fresh(a.population)
        self.init = default_init(a.alg, a.rng, a.population, a.n, a.values)

    def evaluate(self):
        a = self.adv
        self.ho, self.crash, valid = a._realize(self.genome)
        self.base = a.next_id
        a.next_id += a.population
        t = time.perf_counter()
        ev = a.evaluator(self.base, self.ho, self.crash, self.init)
        return ev, valid, time.perf_counter() - t

    def read(self, rows):
        return self.init[rows], self.ho[rows], None if self.crash is None else self.crash[rows]

    def advance(self, elite, parents, n_fresh, generation):
        a = self.adv
        children = a._mutate(a._take(self.genome, parents), max(1, int(a.n * a.R * FLIP_STRENGTH)))
        genome = a._cat(a._take(self.genome, elite), children)
        self.genome = a._cat(genome, a._fresh(n_fresh)) if n_fresh else genome
        cinit = self.init[parents].copy()
        flip = a.rng.random(cinit.shape) < INIT_REDRAW
        cinit[flip] = default_init(a.alg, a.rng, len(parents), a.n, a.values)[flip]
        self.init = np.concatenate([self.init[elite], cinit, default_init(a.alg, a.rng, n_fresh, a.n, a.values)])
        return 0.0


class _DevicePopulation:
    """The population resident in HBM (psg_population_*), generated and mutated there from one
    seed under one instance id block: per generation the per-instance summaries and decisions
    come to the host and the chosen parents go back (no HO set crosses PCIe but a counterexample's)."""

    def __init__(self, adv: "Adversary"):
        self.adv, self.ctx, self.pm = adv, adv.evaluator.gr._ctx, adv._pop_model()

    def _params(self, generation):
        a = self.adv
        p = abi.PopulationParams()
        p.seed, p.generation = self.seed, generation
        # (crash family: one crash-round delivery toggled per mutant, as schedules.mutate_crash)
        p.flips = 1 if a.model.family == "crash" else max(1, int(a.n * a.R * FLIP_STRENGTH))
        p.min_size = a.model.min_size or 0
        p.self_bit = 1 if a.self_bit else 0
        for j, kp in enumerate(a._keep_levels()):
            p.keep_p256[j] = _p256(kp)
        p.value_range = a.values
        p.redraw_p256 = _p256(INIT_REDRAW)
        return p

    def fresh(self):
        a = self.adv
        self.base = a.next_id
        a.next_id += a.population
        self.seed = int(a.rng.integers(0, 1 << 63))
        if self.pm is None:
            self.ctx.population_fresh(self.base, a.population, self._params(0))
        else:
            self.ctx.population_fresh_model(self.base, a.population, self._params(0), self.pm)

    def evaluate(self):
        a, pm = self.adv, self.pm
        t = time.perf_counter()
        _, pi = self.ctx.run_batch_np(self.base, a.population)
        dec, dr = self.ctx.copy_decisions_np()
        valid = np.ones(a.population, bool)
        if a.mode == "liveness":  # only instances with enough live rounds count
            valid = self.ctx.population_live(pm.live_kind, pm.phase, pm.coord).sum(1) >= a.live_rounds
        return Eval(pi, dec, dr), valid, time.perf_counter() - t

    def read(self, rows):
        hos, inits = self.ctx.population_read(rows)
        return inits, hos, self.ctx.population_read_crash(rows)[0] if self.adv.model.family == "crash" else None

    def advance(self, elite, parents, n_fresh, generation):
        P, ne, nm = self.adv.population, len(elite), len(parents)
        parent = np.zeros(P, np.uint32)
        op = np.full(P, 2, np.uint8)  # 0: copy, 1: mutate, 2: fresh
        parent[:ne], op[:ne] = elite, 0
        parent[ne:ne + nm], op[ne:ne + nm] = parents, 1
        t = time.perf_counter()
        if self.pm is None:
            self.ctx.population_next(parent, op, self._params(generation))
        else:
            self.ctx.population_next_model(parent, op, self._params(generation), self.pm)
        return time.perf_counter() - t


class Adversary:
    """Schedule search for one algorithm configuration.

    `evaluator(inst_begin, ho, crash, init) -> Eval` runs a batch (default: the
    GPU through GpuEvaluator); tests may inject another one."""

    def __init__(self, alg: psync.Algorithm, n: int, rounds: int, mode: str = "safety",
                 targets: Optional[Sequence[str]] = None, model: Optional[Model] = None,
                 population: int = 4096, values: int = 3, keep: float = 0.75, self_bit: bool = True,
                 live_rounds: int = 2, live_at: Optional[Sequence[int]] = None, seed: int = 1,
                 evaluator: Optional[Callable] = None, device: int = 0, device_pop: bool = True,
                 device_models: bool = False, device_shrink: bool = False):
        if mode not in ("safety", "liveness"):
            raise ValueError("mode must be 'safety' or 'liveness'")
        self.alg, self.n, self.R = alg, n, rounds
        self.mode = mode
        self.model = model or default_model(alg, n)
        self.names = alg.check_names
        if mode == "liveness":
            if self.model.liveness is None:
                raise ValueError(f"{alg.class_name} has no livenessPredicate to assume")
            self.targets = []
        else:
            want = list(targets) if targets else [self.names[i] for i in alg.violation_slots]
            for t in want:
                if t not in self.names:
                    raise ValueError(f"unknown check slot {t!r} for {alg.class_name}: {self.names}")
            self.targets = [self.names.index(t) for t in want if self.names.index(t) != self.model.predicate_slot]
        self.population, self.values, self.keep = population, values, keep
        self.self_bit, self.live_rounds = self_bit, live_rounds
        self.live_at = None if live_at is None else list(live_at)
        self.device_pop = device_pop
        self.device_models = device_models
        self.device_shrink = device_shrink
        self.shrink_stats = {"steps": 0, "batches": 0, "candidates": 0}  # of the last shrink / shrink_device call
        self.rng = np.random.default_rng(seed)
        self._own = evaluator is None
        self.evaluator = evaluator or GpuEvaluator(alg, n, rounds, population, device=device,
                                                   value_range=values)
        self.next_id = 0

    def close(self):
        if self._own:
            self.evaluator.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -------------------------------------------------------------- schedules
    def _fresh(self, I):
        m, n, R = self.model, self.n, self.R
        if m.family == "crash":
            crash, partial = S.random_crash(self.rng, I, R, n, m.fmax, p_partial=CRASH_DELIVERY)
            return {"crash": crash, "partial": partial}
        # a spread of loss rates around `keep` (each quarter of the population its own)
        parts = []
        for j, kp in enumerate(self._keep_levels()):
            m = I // 4 + (1 if j < I % 4 else 0)
            if m:
                parts.append(S.random_omission(self.rng, m, R, n, kp, self.self_bit))
        return {"ho": np.concatenate(parts)}

    def _keep_levels(self):
        return [min(0.97, self.keep * f) for f in LOSS_SPREAD]

    def _realize(self, g):
        """Genome -> (ho, crash, valid): HO sets repaired to the model's constraints;
        valid[i] = instance i satisfies them (liveness: the predicate holds in at
        least `live_rounds` rounds)."""
        m, n, R = self.model, self.n, self.R
        if m.family == "crash":
            ho = S.crash_to_ho(g["crash"], g["partial"], R, n, self.self_bit)
            return ho, g["crash"], np.ones(ho.shape[0], bool)
        ho = g["ho"].copy()
        S.apply_universe(ho, n, self.self_bit)
        if m.min_size is not None:
            S.repair_min_size(ho, self.rng, n, m.min_size)
        valid = np.ones(ho.shape[0], bool)
        if self.mode == "liveness":
            I = ho.shape[0]
            for j in range(self.live_rounds):
                if self.live_at is not None:
                    ks = np.full(I, self.live_at[j % len(self.live_at)])
                else:
                    ks = self.rng.integers(0, R, I)
                if m.liveness == "good_round":
                    S.force_good_round(ho, self.rng, n, np.arange(I), ks, self_bit=self.self_bit)
                elif m.liveness == "fixed_coord":
                    for k in np.unique(ks):  # the whole phase: the coordinator hears all, then all hear it
                        base = (int(k) // m.phase) * m.phase
                        sel = np.nonzero(ks == k)[0]
                        ho[sel] = S.force_fixed_coord(ho[sel], n, m.coord, range(base, min(R, base + m.phase)), m.phase)
                else:
                    for i, k in enumerate(ks):
                        base = (k // m.phase) * m.phase  # a whole phase with the coordinator hearing all
                        S.force_coord_hears_all(ho[i:i + 1], n, range(base, min(R, base + m.phase)), m.phase)
            if m.min_size is not None:
                S.repair_min_size(ho, self.rng, n, m.min_size)
            valid = self._live_count(ho) >= self.live_rounds
        return ho, None, valid

    def _live_count(self, ho):
        m = self.model
        if m.liveness == "good_round":
            return S.good_round(ho, self.n).sum(1)
        if m.liveness == "fixed_coord":
            return S.fixed_coord_live(ho, self.n, m.coord).sum(1)
        return S.coord_hears_all(ho, self.n, m.phase).sum(1)

    def _mutate(self, g, strength):
        m = self.model
        if m.family == "crash":
            c, p = S.mutate_crash(g["crash"], g["partial"], self.rng, self.R, self.n, m.fmax, CRASH_MUTATE)
            return {"crash": c, "partial": p}
        ho = g["ho"].copy()
        S.flip_links(ho, self.rng, self.n, strength, self.self_bit)
        return {"ho": ho}

    @staticmethod
    def _take(g, idx):
        return {k: v[idx] for k, v in g.items()}

    @staticmethod
    def _cat(a, b):
        return {k: np.concatenate([a[k], b[k]]) for k in a}

    # -------------------------------------------------------------- scoring
    def _violations(self, ev: Eval):
        """(genuine violation mask [I], first violating check point [I])."""
        ff = ev.first_fail.astype(np.int32)
        I = ff.shape[0]
        if self.mode == "liveness":
            bad = ev.summary["term_round"] == NEVER
            return bad, np.where(bad, self.R, NEVER)
        first = ff[:, self.targets].min(1) if self.targets else np.full(I, NEVER)
        bad = first < NEVER
        if self.model.predicate_slot is not None:
            bad &= first < ff[:, self.model.predicate_slot]
        return bad, first

    def _score(self, ev: Eval):
        ff = ev.first_fail
        k = len(self.names)
        failed = (ff[:, :k] != NEVER)
        if self.model.predicate_slot is not None:
            failed[:, self.model.predicate_slot] = False
        dec, dr = ev.decision, ev.decision_round
        decided = dr >= 0
        if self.alg.real:
            lo = np.where(decided, dec, np.inf).min(1)
            hi = np.where(decided, dec, -np.inf).max(1)
            spread = np.where(decided.any(1), (hi - lo) / max(self.alg.epsilon, 1e-300), 0.0)
            distinct = np.minimum(spread, 10.0)
        else:
            lo = np.where(decided, dec, np.iinfo(np.int32).max).min(1)
            hi = np.where(decided, dec, np.iinfo(np.int32).min).max(1)
            distinct = (decided.any(1) & (hi != lo)).astype(np.int64)
            multi = np.nonzero(distinct)[0]
            if len(multi):  # exact count only where decisions differ (rare)
                d = np.where(decided[multi], dec[multi], np.iinfo(np.int32).min)
                srt = np.sort(d, 1)
                distinct[multi] = ((np.diff(srt, axis=1) != 0) & (srt[:, 1:] != np.iinfo(np.int32).min)).sum(1)
        if self.mode == "liveness":
            late = ev.summary["term_round"].astype(np.float64)
            return late + 0.1 * (~decided).sum(1) + self.rng.random(len(late)) * 1e-3
        return 4.0 * distinct + failed.sum(1) + 0.05 * decided.sum(1) / self.n + self.rng.random(len(ff)) * 1e-3

    # -------------------------------------------------------------- search
    def device_population(self) -> bool:
        """Can generations be generated and mutated on the GPU (psg_population_*)?
        General omission, safety search, integer inputs, the GPU evaluator; with
        device_models also the crash family and the liveness search (psg_population_*_model)."""
        ok = not self.alg.real and isinstance(self.evaluator, GpuEvaluator) and self.device_pop
        if self.model.family == "omission" and self.mode == "safety":
            return ok
        return ok and self.device_models and self.live_rounds <= abi.PSG_POP_MAX_LIVE

    def _pop_model(self):
        """The psg_population_model of this search, or None for the plain omission family."""
        m = self.model
        if m.family == "omission" and self.mode == "safety":
            return None
        pm = abi.PopulationModel()
        if m.family == "crash":
            pm.family, pm.fmax = abi.PSG_POP_CRASH, m.fmax
            for j, d in enumerate(CRASH_DELIVERY):
                pm.partial_p256[j] = _p256(d)
            pm.move_p256, pm.add_p256, pm.drop_p256 = _p256(CRASH_MUTATE), _p256(CRASH_MUTATE), _p256(CRASH_MUTATE / 2)
            return pm
        pm.family = abi.PSG_POP_OMISSION
        pm.live_kind = LIVE_KIND[m.liveness]
        pm.live_rounds = self.live_rounds
        for j in range(self.live_rounds):
            pm.live_at[j] = -1 if self.live_at is None else self.live_at[j % len(self.live_at)]
        pm.phase, pm.coord = m.phase, m.coord
        return pm

    def search(self, generations: int = 50, want: int = 1, time_budget: Optional[float] = None,
               elite_frac: float = 0.25, fresh_frac: float = 0.25, shrink: bool = True) -> SearchResult:
        """The search loop: evaluate the population, collect genuine violations, score, and build
        the next generation from elites, mutants of elites and fresh schedules."""
        P = self.population
        pop = _DevicePopulation(self) if self.device_population() else _HostPopulation(self)
        pop.fresh()
        found: List[Counterexample] = []
        t0 = time.perf_counter()
        gpu = 0.0
        history = []
        g = 0
        for g in range(1, generations + 1):
            ev, valid, t = pop.evaluate()
            gpu += t
            bad, first = self._violations(ev)
            bad &= valid
            rows = np.nonzero(bad)[0][:max(0, want - len(found))]
            if len(rows):
                inits, hos, crashes = pop.read(rows)
                for j, i in enumerate(rows):
                    found.append(self._cex(pop.base + int(i), inits[j], hos[j], None if crashes is None else crashes[j],
                                           ev.summary[i], int(first[i])))
            score = self._score(ev)
            history.append(float(score.max()))
            if len(found) >= want or (time_budget is not None and time.perf_counter() - t0 > time_budget):
                break
            order = np.argsort(-score)
            ne = max(1, int(P * elite_frac))
            nf = int(P * fresh_frac)
            nm = P - ne - nf
            elite = order[:ne]
            gpu += pop.advance(elite, elite[self.rng.integers(0, ne, nm)], nf, g)
        secs = time.perf_counter() - t0
        if shrink:
            found = [self._shrink(c) for c in found]
        return SearchResult(found, P * g, g, secs, gpu, history)

    def _cex(self, inst, init, ho, crash, summ, first):
        ff = summ["first_fail"]
        if self.mode == "liveness":
            viol = ["Termination"]
        else:
            viol = [self.names[t] for t in self.targets if ff[t] == first]
        return Counterexample(inst, np.array(init), np.array(ho), None if crash is None else np.array(crash),
                              np.array(summ), viol, first, self._omitted(ho))

    def _omitted(self, ho):
        """Links (k, p, q) missing from one schedule [R][n][W] (q == p excluded with self_bit)."""
        have = int(S.sizes(ho[None]).sum())
        R = ho.shape[0]
        total = R * self.n * self.n
        return total - have

    # -------------------------------------------------------------- shrinking
    def _still_bad(self, c: Counterexample, hos, crashes):
        """Evaluate candidate schedules of counterexample c (same init and instance id)."""
        I = hos.shape[0]
        init = np.repeat(c.init[None], I, 0)
        bads, firsts, sums = [], [], []
        for a in range(0, I, self.population):
            b = min(I, a + self.population)
            # every candidate replays the counterexample's own instance id (same coins)
            ev = self._eval_same_id(c.inst_id, hos[a:b], None if crashes is None else crashes[a:b], init[a:b])
            bad, first = self._violations(ev)
            bads.append(bad)
            firsts.append(first)
            sums.append(ev.summary)
        return np.concatenate(bads), np.concatenate(firsts), np.concatenate(sums)

    def _eval_same_id(self, inst, ho, crash, init):
        """BenOr's coins are keyed by the instance id, so its candidates run one per call under
        the counterexample's id. Other algorithms do not depend on the id under an explicit
        schedule, so they run as one batch."""
        if self.alg.alg_id != abi.PSG_ALG_BENOR:
            return self.evaluator(inst, ho, crash, init)
        outs = [self.evaluator(inst, ho[j:j + 1], None if crash is None else crash[j:j + 1], init[j:j + 1])
                for j in range(ho.shape[0])]
        return Eval(np.concatenate([o.summary for o in outs]), np.concatenate([o.decision for o in outs]),
                    np.concatenate([o.decision_round for o in outs]))

    def _shrink_plan(self, c: Counterexample, max_steps, step) -> Counterexample:
        """Greedy batched delta debugging, the plan of both paths. step(cur, level, arg) evaluates
        the candidates of one abi.PSG_SHRINK_* level over the current counterexample and returns
        the one it adopted, or None (no candidate, or none still bad). Crash-stop: un-crash
        processes and crash them later (CRASH, arg = the self bit) while that succeeds. Omission:
        make the rounds after the violation fault-free (TAIL, not counted as a step), then restore
        whole rounds, whole heard-of sets and single links (LINK: at most about 4 * population
        candidates); restoring links only grows HO sets, so the model's predicates keep holding.
        The levels share the budget of max_steps, and a level ends with its first step that
        adopts nothing. Fills shrink_stats."""
        self.shrink_stats = stats = {"steps": 0, "batches": 0, "candidates": 0}
        cur = c

        def once(level, arg):
            nonlocal cur
            nxt = step(cur, level, arg)
            if nxt is not None:
                cur = nxt
            return nxt is not None

        def repeat(level, arg):
            while stats["steps"] < max_steps:
                stats["steps"] += 1
                if not once(level, arg):
                    break

        if self.model.family == "crash":
            repeat(abi.PSG_SHRINK_CRASH, 1 if self.self_bit else 0)
            return cur
        if self.mode == "safety" and c.check_point < NEVER:
            once(abi.PSG_SHRINK_TAIL, c.check_point)
        repeat(abi.PSG_SHRINK_ROUND, 0)
        repeat(abi.PSG_SHRINK_SET, 0)
        repeat(abi.PSG_SHRINK_LINK, 4 * self.population)
        return cur

    @staticmethod
    def _simplest(bad, first, links, valid=None):
        """The selection rule of a shrink step: among the candidates still bad the one with the
        most links present, then the earliest violation; the first one of several. (key, index);
        candidates that are not `valid` rank below every other."""
        key = np.where(bad, links.astype(np.int64) * 1024 - first, -1)
        if valid is not None:
            key[~valid] = np.iinfo(np.int64).min
        j = int(np.argmax(key))
        return int(key[j]), j

    def _adopted(self, cur: Counterexample, summ, first, **fields) -> Counterexample:
        """cur after a step chose the candidate with this summary and first violating check point."""
        viol = cur.violated if self.mode == "liveness" else \
            [self.names[t] for t in self.targets if summ["first_fail"][t] == first]
        return replace(cur, summary=summ, violated=viol, check_point=int(first), **fields)

    def _shrink_step_host(self, cur: Counterexample, level, arg) -> Optional[Counterexample]:
        """One step with the candidates built and uploaded by the host, in chunks of `population`."""
        hos, crashes = S.shrink_candidates(cur.ho, cur.crash, level, arg, self.n, self.self_bit)
        if len(hos) and self.mode == "liveness":
            assert crashes is None  # (liveness models are of the omission family: no crash rounds to filter along)
            hos = hos[self._live_count(hos) >= self.live_rounds]
        if not len(hos):
            return None
        bad, first, summ = self._still_bad(cur, hos, crashes)
        self.shrink_stats["batches"] += 1
        self.shrink_stats["candidates"] += len(hos)
        if not bad.any():
            return None
        _, j = self._simplest(bad, first, S.sizes(hos).sum((-1, -2)))
        return self._adopted(cur, summ[j], first[j], ho=hos[j].copy(),
                             crash=None if crashes is None else crashes[j].copy(), omitted_links=self._omitted(hos[j]))

    def _shrink_step_device(self, cur: Counterexample, level, arg) -> Optional[Counterexample]:
        """One step with the candidates written on the device (psg_shrink_load) over the base
        resident there; per chunk of `population` candidates only the summaries, the link counts
        and (liveness) the live rounds come to the host. cur keeps the ho / crash / omitted_links
        it came with: shrink_device reads them once, at the end."""
        ctx, m, P = self.evaluator.gr._ctx, self.model, self.population
        total = ctx.shrink_count(level, arg)
        self.shrink_stats["batches"] += int(total > 0)
        best = (np.iinfo(np.int64).min,)  # (key, index, summary, first) of the first maximum so far
        any_bad = False
        for a in range(0, total, P):
            k = min(P, total - a)
            ctx.shrink_load(level, arg, a, k, cur.inst_id)  # every candidate replays the counterexample's id
            _, pi = ctx.run_batch_np(cur.inst_id, k)
            self.shrink_stats["candidates"] += k
            bad, first = self._violations(Eval(pi, None, None))
            links, valid = ctx.population_links(), None
            if self.mode == "liveness":  # the host drops these candidates before it evaluates
                valid = ctx.population_live(LIVE_KIND[m.liveness], m.phase, m.coord).sum(1) >= self.live_rounds
                bad &= valid
            any_bad |= bool(bad.any())
            key, j = self._simplest(bad, first, links, valid)
            if key > best[0]:
                best = (key, a + j, pi[j].copy(), int(first[j]))
        if not any_bad:
            return None
        ctx.shrink_adopt(level, arg, best[1])
        return self._adopted(cur, best[2], best[3])

    def shrink(self, c: Counterexample, max_steps: int = 64) -> Counterexample:
        """Shrink c while the violation persists (_shrink_plan), the candidates built on the host."""
        return self._shrink_plan(c, max_steps, self._shrink_step_host)

    def _shrink(self, c: Counterexample) -> Counterexample:
        """search(shrink=True): on the device when device_shrink is set and available."""
        if self.device_shrink and self.device_shrink_available():
            return self.shrink_device(c)
        return self.shrink(c)

    def device_shrink_available(self) -> bool:
        """Can shrink steps run on the GPU (psg_shrink_*)? The GPU evaluator (one device), integer
        inputs, not BenOr: its coins are keyed by the instance id, so its candidates run one by one."""
        return isinstance(self.evaluator, GpuEvaluator) and not self.alg.real and \
            self.alg.alg_id != abi.PSG_ALG_BENOR

    def shrink_device(self, c: Counterexample, max_steps: int = 64) -> Counterexample:
        """shrink() with the candidates of every step written on the device from a base schedule
        resident there: the same plan and selection, so the same counterexample bit for bit. In
        liveness mode every candidate of a list is evaluated and the ones with too few live rounds
        are then left out of the choice, where the host drops them before it evaluates:
        shrink_stats["candidates"] counts them, so it can exceed the host's count (the result does
        not change)."""
        if not self.device_shrink_available():
            raise ValueError("shrink_device needs the GPU evaluator, integer inputs and an algorithm other than BenOr")
        ctx = self.evaluator.gr._ctx
        ctx.shrink_begin(c.ho, c.crash, c.init)
        cur = self._shrink_plan(c, max_steps, self._shrink_step_device)
        if cur is c:  # nothing adopted
            return c
        ho, crash = ctx.shrink_read()
        return replace(cur, ho=ho, crash=crash, omitted_links=self._omitted(ho))


# ------------------------------------------------------------------ files

def save(path: str, adv: Adversary, cexs: Sequence[Counterexample], meta: Optional[dict] = None):
    """Write counterexamples as a .psgr record file (replay with records.replay)."""
    if not cexs:
        raise ValueError("no counterexamples to save")
    order = np.argsort([c.inst_id for c in cexs], kind="stable")
    cexs = [cexs[i] for i in order]
    cfg = adv.evaluator.cfg if hasattr(adv.evaluator, "cfg") else psync.make_config(adv.alg, adv.n, adv.R)
    summ = np.stack([np.asarray(c.summary, records.SUMMARY_DTYPE) for c in cexs])
    crash = None
    if any(c.crash is not None for c in cexs):
        crash = np.stack([c.crash if c.crash is not None else np.full(adv.n, -1, np.int32) for c in cexs])
    m = {"mode": adv.mode, "targets": [adv.names[t] for t in adv.targets], "family": adv.model.family,
         "violated": [c.violated for c in cexs], "check_point": [c.check_point for c in cexs],
         "omitted_links": [int(c.omitted_links) for c in cexs]}
    m.update(meta or {})
    rec = records.Records(cfg=cfg, slot_names=list(adv.names), ids=np.array([c.inst_id for c in cexs], np.uint64),
                          summary=summ, init=np.stack([c.init for c in cexs]), ho=np.stack([c.ho for c in cexs]),
                          crash=crash, meta=m, class_name=adv.alg.class_name)
    records.write(path, rec)
    return rec


def describe(c: Counterexample, n: int) -> str:
    """Human-readable rendering: the missing links per round up to the violation."""
    lines = [f"instance {c.inst_id}: {', '.join(c.violated)} violated at check point {c.check_point}; "
             f"{c.omitted_links} omitted link(s)", f"  init = {list(np.asarray(c.init).tolist())}"]
    R = c.ho.shape[0]
    last = R if c.check_point >= NEVER else min(R, c.check_point)
    for k in range(last):
        miss = []
        for p in range(n):
            for q in range(n):
                if not (int(c.ho[k, p, q >> 6]) >> (q & 63)) & 1:
                    miss.append(f"{q}->{p}")
        lines.append(f"  round {k}: " + ("all delivered" if not miss else "lost " + " ".join(miss[:40]) +
                                           (" ..." if len(miss) > 40 else "")))
    if c.crash is not None and (c.crash >= 0).any():
        lines.append("  crashed: " + ", ".join(f"{q}@{int(c.crash[q])}" for q in np.nonzero(c.crash >= 0)[0]))
    return "\n".join(lines)
