"""GPU parity over every kernel instantiation: W = ceil(n / 64) in 1..4 x launch mode.

Every round kernel is a template over W, and the host layer picks another kernel for the same
algorithm depending on how the batch is launched (`dispatch` below restates the rule). This module
runs every algorithm at both word-boundary shapes of every W > 1 (last mask word holds one
process: n = 65, 129, 193; last word full: n = 128, 192, 256) in every launch mode:

  seeded    built-in checks, against oracle.run / run_real (TwoPhaseCommit: py_tpc on the
            materialized schedule): summary, per-instance summaries, decisions(), fetched records.
  traced    psg_run_batch_spec with a bytecode program, so the group kernel runs with a.trace set.
            The run's own outputs (digest, n_decided, decisions) equal the oracle's run of the same
            config, and the Spec results equal oracle.vm_run over oracle.trace.
  explicit  psg_load_inputs + psg_load_schedule against oracle.run_schedule (py_tpc). The integer
            algorithms other than BenOr and TwoPhaseCommit get INT32_MIN, INT32_MAX, -1 and 0 in
            every instance, one of them in the last mask word.
  fused     the fused Spec module's round kernel, seeded and (fused-x) under a loaded schedule:
            rows equal the traced run's of the same context; the traced run under the loaded
            schedule is compared with the oracle in the same test.

Further parts: host inputs with the extremes on the lane-packed kernels (part 2: the X0 set's
sentinel INT32_MIN is itself an initial value), n = 1, 2, 3 (part 3), and the guards without a GPU
(part 4): every case's inputs make the oracle show deciders in the last mask word (process n - 1
for ragged n), non-constant decisions and a crash in the last word, and the case table covers
every cell of {10 algorithms} x {W = 1..4} x {the modes the algorithm has} (`required_cells`);
cells left to another module name the test (`DELEGATED`).

Findings written down while building the table:

* KSetAgreement once had a third, unsplit launch shape (one lane-packed kernel for all rounds) that
  could not be reached through the C ABI: psg_create allocates the hand-off buffer for every
  KSetAgreement context with W > 1 (psg_api.hip, `d_hand.grow`) and make_args always sets
  `hand_hdr` from it. That shape has been deleted; launch_w (psg_kset.hip) refuses a W > 1 seeded
  launch without the buffer. The two shapes are general rounds + loss-free tail
  (`drop_log2 == 0 && ho_min < 0`: rows "kset") and general rounds + general tail (rows
  "kset-loss" by drop_log2 > 0 and "kset-homin" by ho_min >= 0).
* The FloodMin mutant (variant 1: decides from round f - 1 on) and the KSetAgreement mutant
  (variant 1: `same > 1` instead of `same > n - k`) decide early, but still a value some process
  held, and every held value is a minimum of initial values: neither can decide a value that is not
  initial. So `X0Set::contains(kEmpty)` with `has_empty` false is asked by no run; part 2 includes
  the mutant rows and instances without INT32_MIN (the set then answers for the other extremes
  with empty slots left in the table), which is as close as the ABI gets.

That the cases can fail was measured once on an MI355X with scratch builds of the library (not
kept), each with a single value-only defect in an instantiation no test reached before. The fused
modules were the committed sources' (they compile from the sources, not from the library).

A. LastVoting, `vote = W == 4 ? v + 1 : v` where the coordinator takes its vote in slot 0 (lv_kernel
   <4, *>): fails test_seeded_matches_oracle, test_traced_matches_oracle and
   test_explicit_matches_oracle at lv-n193 and lv-n256, and the two fused tests at lv-n193 (the
   traced run they compare with is the library's). The other 46 LastVoting cases pass.
B. KSetAgreement group kernel, `kset_pick(...) + (W == 3 ? 1 : 0)` where a decider decides
   (kset_body, not the lane-packed kernel): fails test_traced_matches_oracle and
   test_explicit_matches_oracle at kset-n129 and kset-n192, and the two fused tests at kset-n129.
   The seeded kset rows at n = 129 and 192 pass: they run the lane-packed kernels.
C. `has_empty` always false in pk_x0_build, so X0Set::contains(kEmpty) answers false on the
   lane-packed path: fails all ten test_extreme_inputs_on_the_packed_kernels cases (FloodMin,
   KSetAgreement, KSetEarlyStopping and the two mutants at n = 65 and 256) and nothing else among
   the 125 FloodMin / KSet / KSES cases.

The GPU suite as it stood before this module ran under a library with the three defects together
(719 tests): 718 pass. One sees defect B, which the survey of the case tables had missed:
test_gpu_schedule.py::test_materialized_schedule_matches_oracle_and_replays[kset-crash-loss]
replays a seeded n = 130 run through psg_load_schedule and compares the two GPU runs' digests,
so kset_kernel<3, true> did run before, though never against the oracle. Nothing saw A or C.

Evaluating a Spec with the CPU interpreter is what the traced cases can least afford: see
`vm_sample` and `traced_program` for what is sampled and why, with the measured times.
"""
import collections
import functools
import importlib

import numpy as np
import pytest

from round_amd import abi, formula as F, lib, psync, schedules as S

import spec_cases
from gpu_support import (BEGIN, F64_ABS_TOL, assert_equal_to_restatement, assert_run_equals_oracle, cmp_instances,
                         cmp_summary, gpu_explicit, inst_tuple, np_inst_tuple, random_init, random_schedule, rec_tuple,
                         run_any, schedule_cfg, seeded_votes, spec_rows, tpc_seeded)
from restatement import M64, digest_of, ho_ints, py_tpc
from spec_cases import ALG_ID, FUSED_N, FUSED_X_N, spec_of

gpu = pytest.mark.gpu
H = psync.HOSchedule
I32MIN, I32MAX = -(1 << 31), (1 << 31) - 1

ALGS = ("otr", "otr2", "lv", "slv", "fm", "kset", "kses", "benor", "eps", "tpc")
WIDE = (65, 128, 129, 192, 193, 256)  # per W > 1: last word holds one process / is full
NARROW = (63, 64)


# ------------------------------------------------------------------------------------ the dispatch rule
def dispatch(alg, n, sched, mode):
    """(kernel family, W, flavour) the host layer launches: a restatement of the `launch_w`
    functions. `sched` is the config's psg_schedule; mode is seeded / traced / explicit / fused /
    fused-x. The six rules, first match wins:

    1. fused, fused-x: psg_run_batch_spec with a fused module launches the module's
       `psg_fused_a<alg>_w<W>`, or `psg_fused_x_a<alg>_w<W>` when a schedule is loaded
       (psg_api.hip:958-971).
    2. explicit (`a.ho_in != 0`): `*_kernel<W, true>` for every algorithm. The lane-packed branches
       test `!a.ho_in` first (psg_otr.hip:437, psg_lv.hip:429, psg_slv.hip:229, psg_tpc.hip:136,
       psg_epsilon.hip:525, psg_benor.hip:514, psg_kset_es.hip:326, psg_kset.hip:914,
       psg_floodmin.hip:375).
    3. traced (`a.trace != 0`): the group kernel `*_kernel<W, false>`; OTR / OTR2 / LastVoting /
       ShortLastVoting / TwoPhaseCommit have a branch of their own for it (psg_otr.hip:438,
       psg_lv.hip:430, psg_slv.hip:230, psg_tpc.hip:137), the others fall through their packed
       test `!a.trace` to the last line of launch_w.
    4. seeded, W > 1, BenOr / KSetEarlyStopping: the lane-packed kernel (psg_benor.hip:511-512,
       psg_kset_es.hip:323-324).
    5. seeded, W > 1, KSetAgreement: lane-packed general rounds, then the uniform-t tail, loss-free
       when `drop_log2 == 0 && ho_min < 0`, else general (psg_kset.hip:905-911; a context without
       the hand-off buffer gets hipErrorInvalidValue, line 907); FloodMin when the schedule is
       crash-only, `drop_log2 == 0 && good_p32 == 0 && ho_min < 0` (psg_floodmin.hip:371-373).
    6. everything else: the group kernel `*_kernel<W, false>` (the last line of every launch_w).
       For FloodMin and BenOr at W > 1 that is a lossy (FloodMin) or traced launch only, so those
       six kernels hold no built-in-check fast arm (floodmin_fast is W == 1; benor_fast is compiled
       for W == 1 and for the explicit-schedule kernels).
    """
    W = (n + 63) // 64
    if mode in ("fused", "fused-x"):
        return ("fused", W, mode)
    if mode == "explicit":
        return ("group", W, "xho")
    if mode == "traced":
        return ("group", W, "traced")
    assert mode == "seeded"
    if W > 1 and alg in ("benor", "kses"):
        return ("packed", W, "seeded")
    if W > 1 and alg == "kset":
        return ("packed", W, "lossfree-tail" if sched.drop_log2 == 0 and sched.ho_min < 0 else "general-tail")
    if W > 1 and alg == "fm" and sched.drop_log2 == 0 and sched.good_p32 == 0 and sched.ho_min < 0:
        return ("packed", W, "seeded")
    return ("group", W, "seeded")


def required_cells():
    """Every (algorithm, family, W, flavour) the dispatch rule can give."""
    cells = set()
    for alg in ALGS:
        for W in (1, 2, 3, 4):
            cells.add((alg, "group", W, "xho"))
            if alg != "eps":
                cells.add((alg, "group", W, "traced"))
            if ALG_ID[alg] in F.FUSED_KERNELS:
                cells |= {(alg, "fused", W, "fused"), (alg, "fused", W, "fused-x")}
            if W == 1 or alg in ("otr", "otr2", "lv", "slv", "fm", "eps", "tpc"):
                cells.add((alg, "group", W, "seeded"))
            if W > 1 and alg in ("benor", "kses", "fm"):
                cells.add((alg, "packed", W, "seeded"))
            if W > 1 and alg == "kset":
                cells |= {(alg, "packed", W, "lossfree-tail"), (alg, "packed", W, "general-tail")}
    return cells


# ------------------------------------------------------------------------------------ 1. the matrix
Row = collections.namedtuple("Row", "name alg make kw")


def _benor_kw(n):
    # the default schedule (links lost w.p. 1/4) lets 2 of 60 instances decide at n = 256
    return dict(schedule=H(drop_log2=3, good_round=0.0, ho_min=n // 2)) if n == 256 else {}


ROWS = [
    Row("otr", "otr", lambda n: psync.OTR(), lambda n: dict(value_range=8)),
    Row("otr2", "otr2", lambda n: psync.OTR2(), lambda n: dict(value_range=8)),
    Row("lv", "lv", lambda n: psync.LastVoting(), lambda n: {}),
    Row("slv", "slv", lambda n: psync.ShortLastVoting(), lambda n: {}),
    # crash-only: the lane-packed kernel when seeded, the group kernel's crash-stop branch when traced
    Row("fm", "fm", lambda n: psync.FloodMin(4), lambda n: dict(value_range=2 * n)),
    Row("fm-lossy", "fm", lambda n: psync.FloodMin(4),
        lambda n: dict(value_range=2 * n, schedule=H(drop_log2=2, good_round=0.0, crash_fmax=4))),
    Row("kset", "kset", lambda n: psync.KSetAgreement(2), lambda n: {}),
    # a link is lost w.p. 1/256: about n / 256 per receiver, so `same > n - k` still happens
    Row("kset-loss", "kset", lambda n: psync.KSetAgreement(3),
        lambda n: dict(rounds=5, schedule=H(drop_log2=8, good_round=0.0, crash_fmax=2))),
    # two or more crashed senders missing: the set is raised to everybody
    Row("kset-homin", "kset", lambda n: psync.KSetAgreement(2),
        lambda n: dict(schedule=H(drop_log2=0, good_round=0.0, crash_fmax=3, ho_min=n - 2))),
    Row("kses", "kses", lambda n: psync.KSetEarlyStopping(8, 2), lambda n: {}),
    Row("benor", "benor", lambda n: psync.BenOr(), _benor_kw),
    Row("eps", "eps", lambda n: psync.EpsilonConsensus(5, 0.05), lambda n: {}),
    # links lost w.p. 1/1024 (the default 1/64 leaves no commit at n = 256); coordinator in the last word
    Row("tpc", "tpc", lambda n: psync.TwoPhaseCommit(coord=n - 1), lambda n: dict(schedule=H(drop_log2=10,
                                                                                          good_round=0.0))),
]
ROW = {r.name: r for r in ROWS}
TRACED_ROWS = spec_cases.SPEC_ALGS
assert all(ROW[r].alg == r for r in TRACED_ROWS)  # spec_cases.fused_modules() names the modules by these

# Seeds: 3, except where the crash guard needs another one. With at most 1..4 crashes among n
# processes, process n - 1 of a ragged n crashes in few instances; these seeds are the first of
# 3, 4, 5, ... under which it does in some instance (scanned on the oracle's crash rounds).
SEEDS = {("fm", 193): 5, ("fm-lossy", 193): 5, ("kset", 129): 15, ("kset", 193): 38, ("kset-loss", 129): 12,
         ("kset-loss", 193): 5, ("kset-homin", 129): 11, ("kset-homin", 193): 5, ("kses", 193): 5}


def seed_of(row, n):
    return SEEDS.get((row, n), 3)


def count_of(row, n):
    return 200 if n <= 64 else 24 if ROW[row].alg == "kset" else 60


def case_cfg(row, n):
    r = ROW[row]
    return psync.make_config(r.make(n), n, seed=seed_of(row, n), batch_capacity=count_of(row, n), **r.kw(n))


Oracle = collections.namedtuple("Oracle", "cfg osum opi orec dec dround crash runs")
_ORACLE = {}


def oracle_case(oracle_mod, row, n):
    """The oracle's run of a seeded case (once per session, never modified). dec / dround are
    [count][n]; crash the schedule's crash rounds (None without crashes); runs the py_tpc runs (TwoPhaseCommit)."""
    if (row, n) not in _ORACLE:
        cfg, cnt = case_cfg(row, n), count_of(row, n)
        r = ROW[row]
        runs = osum = opi = None
        crash = None
        if cfg.sched.crash_fmax > 0:  # the generator reads n, R, the seed and the schedule only
            gen = schedule_cfg(cfg)
            crash = np.array([[oracle_mod.crash_round(gen, BEGIN + i, p) for p in range(n)] for i in range(cnt)],
                             np.int32)
        if r.alg == "tpc":
            ho, _ = oracle_mod.materialize_schedule(schedule_cfg(cfg), BEGIN, cnt)
            votes = seeded_votes(cfg, oracle_mod, BEGIN, cnt)
            runs = [py_tpc(n, cfg.param, votes[i], ho_ints(ho[i]), cfg.rounds) for i in range(cnt)]
            orec = None
            dec = np.array([[x[0] for x in run.rec] for run in runs], np.float64)
            dround = np.array([[x[1] for x in run.rec] for run in runs], np.int64)
        else:
            if r.alg == "eps":
                osum, opi, orec, odec, _ = oracle_mod.run_real(cfg, BEGIN, cnt, per_instance=True, records=True,
                                                               threads=8)
                dec = np.array(odec, np.float64).reshape(cnt, n)
            else:
                osum, opi, orec = oracle_mod.run(cfg, BEGIN, cnt, per_instance=True, records=True, threads=8)
                dec = np.array([x.decision for x in orec], np.float64).reshape(cnt, n)
            dround = np.array([x.decision_round for x in orec], np.int64).reshape(cnt, n)
        _ORACLE[(row, n)] = Oracle(cfg, osum, opi, orec, dec, dround, crash, runs)
    return _ORACLE[(row, n)]


def check_guards(name, n, dec, dround, crash):
    """What a case exists for, on the oracle's results alone (part 4)."""
    cnt = dround.shape[0]
    lo = 64 * ((n - 1) // 64)  # first pid of the last mask word
    decided = dround >= 0
    in_last = int(decided[:, lo:].any(axis=1).sum())
    assert 10 * in_last >= cnt, f"{name}: a process of the last mask word decides in {in_last} of {cnt} instances"
    if n % 64:
        last = int(decided[:, n - 1].sum())
        assert 10 * last >= cnt, f"{name}: process n - 1 decides in {last} of {cnt} instances"
    pairs = {(float(d), int(k)) for d, k in zip(dec[decided].tolist(), dround[decided].tolist())}
    assert len(pairs) >= 2, f"{name}: one (decision, round) pair in the whole batch: {pairs}"
    if crash is not None and (crash >= 0).any():
        assert (crash[:, lo:] >= 0).any(), f"{name}: no process of the last mask word crashes in any instance"


def sample_of(cnt):
    return [BEGIN + i for i in range(0, cnt, max(1, cnt // 19))]


SEEDED = [(r.name, n) for r in ROWS for n in WIDE]
TRACED = [(row, n) for row in TRACED_ROWS for n in NARROW + WIDE]
FUSED = [(row, n) for row in TRACED_ROWS for n in FUSED_N]


def _ids(cases):
    return [f"{a}-n{n}" for a, n in cases]


@gpu
@pytest.mark.parametrize("row,n", SEEDED, ids=_ids(SEEDED))
def test_seeded_matches_oracle(row, n, oracle_mod):
    """The built-in-checks kernel of the cell (`dispatch`): the group kernel `*_kernel<W, false>`,
    or the lane-packed one for BenOr, KSetAgreement, KSetEarlyStopping and crash-only FloodMin."""
    o = oracle_case(oracle_mod, row, n)
    r, cnt = ROW[row], count_of(row, n)
    check_guards(f"{row}-n{n}", n, o.dec, o.dround, o.crash)
    if r.alg == "tpc":
        runs, _ = tpc_seeded(n, o.cfg.rounds, n - 1, r.kw(n)["schedule"], cnt, seed_of(row, n), oracle_mod)
        assert [x.rec for x in runs] == [x.rec for x in o.runs]
        return
    with psync.GpuRound(r.make(n), n, seed=seed_of(row, n), batch_capacity=cnt, **r.kw(n)) as gr:
        assert bytes(gr.cfg) == bytes(o.cfg)
        if r.alg == "eps":
            run_any(gr, oracle_mod, cnt, sample_of(cnt))
        else:
            assert_run_equals_oracle(gr, cnt, o.osum, o.opi, o.orec, sample_of(cnt))


def traced_program(alg, n):
    """The program of a traced case: bytecode, so the interpreter evaluates the Spec over the trace
    the group kernel writes. LastVoting's reference Spec at W = 4 and BenOr's at n = 256 keep the
    device interpreter busy for 14 s and more per batch, whatever the instance count (two nested
    value quantifiers over n processes); there the same Spec runs as a non-fused native module, the
    other evaluator of the same trace (a.trace is set, the same fields are traced)."""
    spec = spec_of(alg)
    if (alg == "lv" and n >= 192) or (alg == "benor" and n == 256):
        return F.compile_native(spec, ALG_ID[alg])
    return F.compile_spec(spec, ALG_ID[alg])


def vm_sample(alg, cfg, cnt):
    """Instances whose oracle trace the CPU interpreter evaluates. oracle.vm_run is one thread of a
    plain interpreter: over all 60 instances it takes 59 s for LastVoting at n = 193, 76 s for BenOr
    at n = 256, 17 s for ShortLastVoting at n = 256 (measured, 0.8e6 process pairs x check points
    per second for LastVoting's Spec, 3e6 and more for the others). The sample is sized for about
    1.5 s and spread over the batch, at least two instances."""
    units = (cfg.rounds + 1) * cfg.n * cfg.n
    m = max(2, min(cnt, (1_200_000 if alg == "lv" else 5_000_000) // units))
    return sorted({(j * cnt) // m for j in range(m)})


def assert_traced_equals_oracle(alg, o, n, cnt, prog, sp, dec, dround, oracle_mod):
    """A psg_run_batch_spec run against the oracle: the run's own outputs, then the Spec results."""
    k = len(prog.slot_names)
    if o.runs is not None:  # TwoPhaseCommit: py_tpc restates both the run and the Spec's four slots
        want_pi = [(digest_of(x), x.n_decided) for x in o.runs]
        want_spec = [(tuple(x.first_fail), x.term_round) for x in o.runs]
        digest = sum(digest_of(x) for x in o.runs) & M64
        decided = sum(x.n_decided for x in o.runs)
    else:
        want_pi = [(s.digest, s.n_decided) for s in o.opi]
        want_spec = None
        digest, decided = o.osum.digest & M64, o.osum.decided_processes
    got_pi = [(s.digest, s.n_decided) for s in sp.per_instance]
    mism = [i for i in range(cnt) if got_pi[i] != want_pi[i]]
    assert not mism, f"{len(mism)} instances differ in (digest, n_decided), first {mism[:5]}"
    assert (sp.summary.digest & M64, sp.summary.decided_processes) == (digest, decided)
    bad = np.nonzero((np.array(dec, np.float64).reshape(cnt, n) != o.dec)
                     | (np.array(dround, np.int64).reshape(cnt, n) != o.dround))
    assert bad[0].size == 0, f"decisions differ, first (instance, process) {(int(bad[0][0]), int(bad[1][0]))}"
    got_spec = spec_rows(sp.per_instance, k)
    for s in range(k):  # counters agree with the per-instance view
        assert sp.summary.fail_count[s] == sum(1 for f, _ in got_spec if f[s] != abi.PSG_NEVER)
    if want_spec is not None:
        assert got_spec == want_spec
        return
    if ALG_ID[alg] in F.REFERENCE_SPECS:  # every instance: the oracle's own evaluation of the same Spec
        assert got_spec == [(tuple(s.first_fail)[:k], s.term_round) for s in o.opi]
    for i in vm_sample(alg, o.cfg, cnt):  # the CPU interpreter over the oracle's trace
        ff, tm = oracle_mod.vm_run(prog, oracle_mod.trace(o.cfg, BEGIN + i, 1), 1, n, o.cfg.rounds)
        assert got_spec[i] == (tuple(ff[0]), tm[0]), i


@gpu
@pytest.mark.parametrize("row,n", TRACED, ids=_ids(TRACED))
def test_traced_matches_oracle(row, n, oracle_mod):
    """The group kernel with a.trace set (the only seeded way into the n > 64 group kernels of
    BenOr, KSetAgreement, KSetEarlyStopping and crash-only FloodMin), under the interpreter."""
    o = oracle_case(oracle_mod, row, n)
    r, cnt = ROW[row], count_of(row, n)
    check_guards(f"{row}-n{n}", n, o.dec, o.dround, o.crash)
    prog = traced_program(r.alg, n)
    if ALG_ID[r.alg] in F.REFERENCE_SPECS:
        assert prog.slot_names == r.make(n).check_names[:len(prog.slot_names)]
    with psync.GpuRound(r.make(n), n, seed=seed_of(row, n), batch_capacity=cnt, **r.kw(n)) as gr:
        assert bytes(gr.cfg) == bytes(o.cfg)
        sp = gr.run_spec(BEGIN, cnt, prog, per_instance=True)
        dec, dround = gr.decisions()
    assert_traced_equals_oracle(r.alg, o, n, cnt, prog, sp, dec, dround, oracle_mod)


@gpu
def test_traced_epsilon_is_refused():
    """Spec programs need integer state: psg_run_batch_spec refuses EpsilonConsensus at every W."""
    prog = F.compile_spec(spec_cases.uniform_agreement())
    for n in (64, 129):
        with psync.GpuRound(psync.EpsilonConsensus(5, 0.05), n, batch_capacity=4) as gr:
            with pytest.raises(lib.PsgError) as e:
                gr.run_spec(BEGIN, 4, prog)
            assert e.value.rc == abi.PSG_EINVAL


# ------------------------------------------------------------------------------------ explicit schedules
# name -> (algorithm, R, schedule family of gpu_support.random_schedule)
EXPLICIT = {
    "otr": (lambda n: psync.OTR(), 8, "omission"),
    "otr2": (lambda n: psync.OTR2(), 8, "omission"),
    "lv": (lambda n: psync.LastVoting(), 12, "omission"),
    "slv": (lambda n: psync.ShortLastVoting(), 12, "omission"),
    "fm": (lambda n: psync.FloodMin(3), 5, "crash"),
    "kset": (lambda n: psync.KSetAgreement(3), 5, "crash"),
    "kses": (lambda n: psync.KSetEarlyStopping(4, 2), 5, "crash"),
    "benor": (lambda n: psync.BenOr(), 16, "omission"),
    "eps": (lambda n: psync.EpsilonConsensus(f=2, epsilon=1e-3), 8, "omission"),
    "tpc": (lambda n: psync.TwoPhaseCommit(coord=n - 1), 3, "omission"),
}
EXTREME_ALGS = ("otr", "otr2", "lv", "slv", "fm", "kset", "kses")
EXTREMES = (I32MIN, I32MAX, -1, 0)
POOL = (-7, 1, 2, 3, 5, 1 << 30)
# W = 1 under an explicit schedule: these three have no case elsewhere
EXPLICIT_CASES = [(a, n) for a in ALGS for n in ((NARROW if a in ("otr2", "kset", "kses") else ()) + WIDE)]


def silence_some_crashed(ho, crash, n):
    """A crash-stop schedule of gpu_support.random_schedule, changed in every second instance that
    has a crashed process: one of them crashes in round 0 instead and reaches nobody. Every
    fourth instance otherwise just names a crashed process. Returns the pid per instance (-1: none):
    extreme_rows puts INT32_MIN there, so the minimum is lost, or spreads only as far as the
    crashing process still reaches, and decisions differ among the instances."""
    I = ho.shape[0]
    at = np.full(I, -1, np.int64)
    for i in range(I):
        crashed = np.nonzero(crash[i] >= 0)[0]
        if i % 4 == 3 or not crashed.size:
            continue
        c = at[i] = int(crashed[i % crashed.size])
        if i % 2 == 0:
            crash[i, c] = 0
            keep = ho[i, :, c, c >> 6].copy()
            ho[i, :, :, c >> 6] &= ~np.uint64(1 << (c & 63))
            ho[i, :, c, c >> 6] = keep
    return at


def extreme_rows(rng, I, n, min_at=None, without_min_every=0):
    """[I][n] int32 from POOL (at most 6 values, so duplicates abound), and in every instance
    INT32_MIN, INT32_MAX, -1 and 0 once each, one of them (rotating) in the last mask word.
    min_at[i] >= 0 places INT32_MIN of instance i (silence_some_crashed).
    without_min_every = m: instance m - 1 of every m holds no INT32_MIN."""
    init = rng.choice(np.array(POOL, np.int64), size=(I, n)).astype(np.int32)
    lo = 64 * ((n - 1) // 64)
    for i in range(I):
        pos = [int(p) for p in rng.permutation(n)[:4]]
        if min_at is not None and min_at[i] >= 0:
            c = int(min_at[i])
            if c in pos:
                pos.remove(c)
            pos = [c] + pos[:3]
        if max(pos) < lo:
            pos[1 + i % 3] = lo + int(rng.integers(n - lo))
        for v, p in zip(EXTREMES, pos):
            init[i, p] = v
        if without_min_every and i % without_min_every == without_min_every - 1:
            init[i, pos[0]] = POOL[i % len(POOL)]
    return init


Explicit = collections.namedtuple("Explicit", "alg R I ho crash init")


@functools.lru_cache(maxsize=None)
def explicit_inputs(name, n):
    make, R, family = EXPLICIT[name]
    alg = make(n)
    # KSetAgreement under the family's 1 / 64 loss merges n maps of n entries per process and round
    # until somebody decides: 24 instances take the oracle 8 s at n = 256, which runs 8
    I = 200 if n <= 64 else 60 if name != "kset" else 24 if n < 256 else 8
    lo = 64 * ((n - 1) // 64)
    for salt in range(64):  # the first of a fixed sequence under which a process of the last word crashes
        rng = np.random.default_rng([ALGS.index(name), n, salt])
        if name == "tpc":  # as test_gpu_tpc._explicit_inputs: few omissions, P(no vote) = 0.5 / n
            ho, crash = S.random_omission(rng, I, R, n, 255 / 256), None
            init = (rng.random((I, n)) >= 0.5 / n).astype(np.int32)
        else:
            ho, crash = random_schedule(rng, alg, n, R, I, family)
            if crash is not None and not (crash[:, lo:] >= 0).any():
                continue
            min_at = None if crash is None else silence_some_crashed(ho, crash, n)
            init = extreme_rows(rng, I, n, min_at) if name in EXTREME_ALGS else random_init(rng, alg, I, n, 4)
        return Explicit(alg, R, I, ho, crash, init)
    raise AssertionError(f"{name}-n{n}: no schedule of the sequence crashes a process of the last mask word")


def explicit_cfg(name, n):
    x = explicit_inputs(name, n)
    return psync.make_config(x.alg, n, rounds=x.R, seed=5, value_range=4, batch_capacity=x.I)


_EXPLICIT_ORACLE = {}


def explicit_oracle(oracle_mod, name, n):
    """The oracle under the explicit inputs (TwoPhaseCommit: py_tpc), as oracle_case gives it."""
    if (name, n) not in _EXPLICIT_ORACLE:
        x, cfg = explicit_inputs(name, n), explicit_cfg(name, n)
        runs = osum = opi = orec = None
        if name == "tpc":
            runs = [py_tpc(n, n - 1, x.init[i], ho_ints(x.ho[i]), x.R) for i in range(x.I)]
            dec = np.array([[r[0] for r in run.rec] for run in runs], np.float64)
            dround = np.array([[r[1] for r in run.rec] for run in runs], np.int64)
        else:
            osum, opi, orec, odec, _ = oracle_mod.run_schedule(cfg, BEGIN, x.I, x.ho, x.crash, x.init,
                                                               per_instance=True, records=True)
            dec = (np.array(odec, np.float64) if name == "eps"
                   else np.array([r.decision for r in orec], np.float64)).reshape(x.I, n)
            dround = np.array([r.decision_round for r in orec], np.int64).reshape(x.I, n)
        _EXPLICIT_ORACLE[(name, n)] = Oracle(cfg, osum, opi, orec, dec, dround, x.crash, runs)
    return _EXPLICIT_ORACLE[(name, n)]


def check_extreme_rows(name, n):
    x = explicit_inputs(name, n)
    lo = 64 * ((n - 1) // 64)
    for i in range(x.I):
        row = x.init[i]
        assert all((row == v).sum() >= 1 for v in EXTREMES), (name, n, i)
        assert np.isin(row[lo:], EXTREMES).any(), (name, n, i)
        assert set(row.tolist()) <= set(EXTREMES) | set(POOL)


@gpu
@pytest.mark.parametrize("name,n", EXPLICIT_CASES, ids=_ids(EXPLICIT_CASES))
def test_explicit_matches_oracle(name, n, oracle_mod):
    """`*_kernel<W, true>`: loaded inputs and HO sets, the extremes among the initial values."""
    x, o = explicit_inputs(name, n), explicit_oracle(oracle_mod, name, n)
    check_guards(f"explicit-{name}-n{n}", n, o.dec, o.dround, x.crash)
    if name in EXTREME_ALGS:
        check_extreme_rows(name, n)
    if name == "tpc":
        s, pi, dec, dr, fs, fr = gpu_explicit(x.alg, n, x.R, x.init, x.ho)
        assert_equal_to_restatement(o.runs, pi, dec, dr, fs, fr)
        assert s.decided_processes == sum(r.n_decided for r in o.runs)
        assert s.digest & M64 == sum(digest_of(r) for r in o.runs) & M64
        return
    ids = [BEGIN + i for i in range(0, x.I, max(1, x.I // 19))]
    with psync.GpuRound(x.alg, n, x.R, seed=5, value_range=4, batch_capacity=x.I) as g:
        assert bytes(g.cfg) == bytes(o.cfg)
        ctx = g._ctx
        ctx.load_inputs(BEGIN, x.I, x.init)
        ctx.load_schedule(BEGIN, x.I, x.ho, x.crash)
        s, pi = ctx.run_batch_np(BEGIN, x.I)
        dec, dr = ctx.copy_decisions_np()
        fs, fr = ctx.fetch_np(ids)
    cmp_summary(s, o.osum, x.R)
    cmp_instances(pi, o.opi)
    assert (dr == o.dround).all()
    if name == "eps":
        assert np.allclose(dec, o.dec, atol=F64_ABS_TOL, rtol=0, equal_nan=True)
    else:
        assert (dec == o.dec).all()
    orr = np.array([rec_tuple(r) for r in o.orec], np.int64).reshape(x.I, n, 4)
    for j, inst in enumerate(ids):
        i = inst - BEGIN
        assert np_inst_tuple(fs[j]) == inst_tuple(o.opi[i]), inst
        fields = ("decision_round", "halt_round") if name == "eps" else ("decision", "decision_round", "halt_round",
                                                                          "final_x")
        cols = (1, 2) if name == "eps" else (0, 1, 2, 3)
        got = np.stack([fr[j][f] for f in fields], axis=1)
        assert (got == orr[i][:, cols]).all(), inst


# ------------------------------------------------------------------------------------ fused modules
def _assert_fused_equals_traced(gr, cnt, alg, n):
    """One context: the interpreter over the traced run, then the fused module's round kernel."""
    prog = traced_program(alg, n)
    fused = F.compile_native(spec_of(alg), ALG_ID[alg], fused=True, n=n)
    assert fused.slot_names == prog.slot_names
    k = len(prog.slot_names)
    tr = gr.run_spec(BEGIN, cnt, prog, per_instance=True)
    fu = gr.run_spec(BEGIN, cnt, fused, per_instance=True)
    assert spec_rows(fu.per_instance, k, digest=True) == spec_rows(tr.per_instance, k, digest=True)
    assert list(fu.summary.fail_count)[:k] == list(tr.summary.fail_count)[:k]
    assert (fu.summary.digest, fu.summary.decided_processes) == (tr.summary.digest, tr.summary.decided_processes)
    return tr


FUSED_X = [(a, n) for a in TRACED_ROWS for n in FUSED_X_N]


@gpu
@pytest.mark.parametrize("row,n", FUSED, ids=_ids(FUSED))
def test_fused_matches_traced(row, n):
    """`psg_fused_a<alg>_w<W>` == the traced run of the same config, which
    test_traced_matches_oracle[row-n] compares with the oracle."""
    r, cnt = ROW[row], count_of(row, n)
    with psync.GpuRound(r.make(n), n, seed=seed_of(row, n), batch_capacity=cnt, **r.kw(n)) as gr:
        _assert_fused_equals_traced(gr, cnt, r.alg, n)


@gpu
@pytest.mark.parametrize("name,n", FUSED_X, ids=_ids(FUSED_X))
def test_fused_matches_traced_under_a_loaded_schedule(name, n, oracle_mod):
    """`psg_fused_x_a<alg>_w<W>` == the traced explicit-schedule run, and that run's digests and
    decision counts are the oracle's under the same inputs."""
    alg = ROW[name].alg
    x, o = explicit_inputs(alg, n), explicit_oracle(oracle_mod, alg, n)
    with psync.GpuRound(x.alg, n, x.R, seed=5, value_range=4, batch_capacity=x.I) as gr:
        gr._ctx.load_inputs(BEGIN, x.I, x.init)
        gr._ctx.load_schedule(BEGIN, x.I, x.ho, x.crash)
        tr = _assert_fused_equals_traced(gr, x.I, alg, n)
    if o.runs is not None:
        want = [(digest_of(r), r.n_decided) for r in o.runs]
    else:
        want = [(s.digest, s.n_decided) for s in o.opi]
    assert [(s.digest, s.n_decided) for s in tr.per_instance] == want


# ------------------------------------------------------------------------------------ 2. extremes, lane-packed
PACKED_X = [(f"{name}-n{n}", name, alg, n)
            for name, alg in (("fm", psync.FloodMin(4)), ("fm-mutant", psync.FloodMin(4, variant=1)),
                              ("kset", psync.KSetAgreement(2)), ("kset-mutant", psync.KSetAgreement(2, variant=1)),
                              ("kses", psync.KSetEarlyStopping(8, 2)))
            for n in (65, 256)]


@functools.lru_cache(maxsize=None)
def packed_inputs(cid):
    _, name, alg, n = next(c for c in PACKED_X if c[0] == cid)
    cnt = 24 if name.startswith("kset") else 60
    rng = np.random.default_rng([77, n, len(name)])
    return alg, n, cnt, extreme_rows(rng, cnt, n, without_min_every=4)


def packed_oracle(oracle_mod, cid):
    if ("packed", cid) not in _ORACLE:
        alg, n, cnt, init = packed_inputs(cid)
        cfg = psync.make_config(alg, n, seed=32, batch_capacity=cnt)
        osum, opi, orec = oracle_mod.run(cfg, BEGIN, cnt, init=init.tolist(), per_instance=True, records=True,
                                         threads=8)
        _ORACLE[("packed", cid)] = (cfg, osum, opi, orec)
    return _ORACLE[("packed", cid)]


def check_packed_preconditions(oracle_mod, cid):
    alg, n, cnt, init = packed_inputs(cid)
    cfg, _, _, orec = packed_oracle(oracle_mod, cid)
    assert dispatch(cid.split("-")[0], n, cfg.sched, "seeded")[0] == "packed"
    dec = np.array([r.decision for r in orec], np.int64).reshape(cnt, n)
    dround = np.array([r.decision_round for r in orec], np.int64).reshape(cnt, n)
    decides_min = int(((dec == I32MIN) & (dround >= 0)).any(axis=1).sum())
    assert 2 * decides_min > cnt, f"{cid}: some process decides INT32_MIN in {decides_min} of {cnt} instances"
    no_min = ~(init == I32MIN).any(axis=1)
    assert no_min.any() and not ((dec[no_min] == I32MIN) & (dround[no_min] >= 0)).any()
    # every decision is an initial value of its instance, the mutants' too (module docstring)
    for i in range(cnt):
        assert set(dec[i][dround[i] >= 0].tolist()) <= set(init[i].tolist()), (cid, i)


@gpu
@pytest.mark.parametrize("cid", [c[0] for c in PACKED_X])
def test_extreme_inputs_on_the_packed_kernels(cid, oracle_mod):
    """Host inputs on the lane-packed kernels with INT32_MIN (the X0 set's empty-slot sentinel,
    tracked by has_empty), INT32_MAX, -1 and 0 among them. On the oracle first: in more than half
    of the instances some process decides INT32_MIN, and some instances hold no INT32_MIN. The
    mutant rows (variant 1) decide early but only initial values (module docstring), so no run
    asks the set for a sentinel that is not an initial value."""
    check_packed_preconditions(oracle_mod, cid)
    alg, n, cnt, init = packed_inputs(cid)
    cfg, osum, opi, orec = packed_oracle(oracle_mod, cid)
    with psync.GpuRound(alg, n, seed=32, batch_capacity=cnt) as gr:
        assert bytes(gr.cfg) == bytes(cfg)
        gr.load_inputs(BEGIN, cnt, init.tolist())
        assert_run_equals_oracle(gr, cnt, osum, opi, orec, sample_of(cnt))


# ------------------------------------------------------------------------------------ 3. tiny n
TINY = [(f"{name}-n{n}", alg, n)
        for name, alg in (("fm-f2", psync.FloodMin(2)), ("fm-f0", psync.FloodMin(0)), ("kset-k2", psync.KSetAgreement(2)),
                          ("kses-t2k2", psync.KSetEarlyStopping(2, 2)), ("benor", psync.BenOr()),
                          ("eps-f1", psync.EpsilonConsensus(1, 0.1)))
        for n in (1, 2, 3)]


def oracle_tiny(oracle_mod, alg, n, cnt=200):
    """The oracle's run of a tiny case, or None where it refuses the config."""
    cfg = psync.make_config(alg, n, seed=3, batch_capacity=cnt)
    try:
        if alg.real:
            oracle_mod.run_real(cfg, BEGIN, 1)
        else:
            oracle_mod.run(cfg, BEGIN, 1)
    except oracle_mod.OracleError:
        return None
    return cfg


@gpu
@pytest.mark.parametrize("cid,alg,n", TINY, ids=[c[0] for c in TINY])
def test_tiny_groups_match_oracle(cid, alg, n, oracle_mod):
    """n = 1, 2, 3 with f >= n, k >= n, t >= n among the shapes: the library and the oracle accept
    and refuse the same configs, and an accepted one runs as the oracle's."""
    cnt = 200
    cfg = oracle_tiny(oracle_mod, alg, n, cnt)
    try:
        gr = psync.GpuRound(alg, n, seed=3, batch_capacity=cnt)
    except lib.PsgError as e:
        assert e.rc == abi.PSG_EINVAL and cfg is None, f"{cid}: the library refuses, the oracle runs"
        return
    with gr:
        assert cfg is not None, f"{cid}: the oracle refuses, the library runs"
        run_any(gr, oracle_mod, cnt, sample_of(cnt))


# ------------------------------------------------------------------------------------ 4. guards, no GPU
@pytest.mark.parametrize("row,n", sorted(set(SEEDED) | set(TRACED)), ids=_ids(sorted(set(SEEDED) | set(TRACED))))
def test_guards_hold_on_the_oracle_seeded(row, n, oracle_mod):
    """Seeded, traced and fused cases share a config per (row, n)."""
    o = oracle_case(oracle_mod, row, n)
    check_guards(f"{row}-n{n}", n, o.dec, o.dround, o.crash)


EXPLICIT_ALL = sorted(set(EXPLICIT_CASES) | {(ROW[a].alg, n) for a, n in FUSED_X})


@pytest.mark.parametrize("name,n", EXPLICIT_ALL, ids=_ids(EXPLICIT_ALL))
def test_guards_hold_on_the_oracle_explicit(name, n, oracle_mod):
    x, o = explicit_inputs(name, n), explicit_oracle(oracle_mod, name, n)
    check_guards(f"explicit-{name}-n{n}", n, o.dec, o.dround, x.crash)
    if name in EXTREME_ALGS:
        check_extreme_rows(name, n)


@pytest.mark.parametrize("cid", [c[0] for c in PACKED_X])
def test_guards_hold_on_the_oracle_packed_extremes(cid, oracle_mod):
    check_packed_preconditions(oracle_mod, cid)


# Which tiny configs the oracle refuses (the library must refuse the same, test_tiny_groups_match_oracle)
TINY_REFUSED_BY_THE_ORACLE = set()


def test_tiny_configs_the_oracle_refuses(oracle_mod):
    refused = {cid for cid, alg, n in TINY if oracle_tiny(oracle_mod, alg, n) is None}
    assert refused == TINY_REFUSED_BY_THE_ORACLE


# Cells left to a test of another module: cell -> (module, test function, parametrize ids).
DELEGATED = {
    ("otr", "group", 1, "seeded"): ("test_gpu_parity", "test_gpu_matches_oracle", ("otr-n64-V64",)),
    ("otr2", "group", 1, "seeded"): ("test_gpu_parity", "test_gpu_matches_oracle", ("otr2-n64-V4",)),
    ("lv", "group", 1, "seeded"): ("test_gpu_parity", "test_gpu_matches_oracle", ("lv-n64-crash",)),
    ("slv", "group", 1, "seeded"): ("test_gpu_parity", "test_gpu_matches_oracle", ("slv-n64",)),
    ("fm", "group", 1, "seeded"): ("test_gpu_parity", "test_gpu_matches_oracle", ("fm-n64-f8",)),
    ("kset", "group", 1, "seeded"): ("test_gpu_parity", "test_gpu_matches_oracle", ("kset-n64-k3-crash",)),
    ("kses", "group", 1, "seeded"): ("test_gpu_parity", "test_gpu_matches_oracle", ("kses-n64-t8k2",)),
    ("benor", "group", 1, "seeded"): ("test_gpu_rounds", "test_long_live_run_matches_oracle", ("benor-n64",)),
    ("eps", "group", 1, "seeded"): ("test_gpu_parity", "test_gpu_epsilon_matches_oracle", ("eps-n64-f5",)),
    ("tpc", "group", 1, "seeded"): ("test_gpu_rounds", "test_tpc_seeded_families_equal_the_restatement",
                                    ("crash-n64-R3",)),
    ("otr", "group", 1, "xho"): ("test_gpu_schedule", "test_explicit_schedule_matches_oracle", ("otr-n64",)),
    ("lv", "group", 1, "xho"): ("test_gpu_schedule", "test_explicit_schedule_matches_oracle", ("lv-n64",)),
    ("slv", "group", 1, "xho"): ("test_gpu_schedule", "test_explicit_schedule_matches_oracle", ("slv-n64",)),
    ("fm", "group", 1, "xho"): ("test_gpu_schedule", "test_explicit_schedule_matches_oracle", ("fm-n64",)),
    ("benor", "group", 1, "xho"): ("test_gpu_schedule", "test_explicit_schedule_matches_oracle", ("benor-n8",)),
    ("eps", "group", 1, "xho"): ("test_gpu_schedule", "test_explicit_schedule_matches_oracle", ("eps-n40",)),
    ("tpc", "group", 1, "xho"): ("test_gpu_tpc", "test_explicit_schedules_equal_the_restatement", ()),
    ("otr", "fused", 1, "fused"): ("test_gpu_spec", "test_reference_spec_program_matches_builtin_checks",
                                   ("otr-n64", "fused")),
    ("otr2", "fused", 1, "fused"): ("test_gpu_spec", "test_reference_spec_program_matches_builtin_checks",
                                    ("otr2-n64", "fused")),
    ("lv", "fused", 1, "fused"): ("test_gpu_spec", "test_reference_spec_program_matches_builtin_checks",
                                  ("lv-n64", "fused")),
    ("benor", "fused", 1, "fused"): ("test_gpu_spec", "test_reference_spec_program_matches_builtin_checks",
                                     ("benor-n8", "fused")),
    ("slv", "fused", 1, "fused"): ("test_gpu_spec", "test_custom_spec_matches_cpu_interpreter", ("slv-n16", "fused")),
    ("fm", "fused", 1, "fused"): ("test_gpu_spec", "test_custom_spec_matches_cpu_interpreter", ("fm-n12", "fused")),
    ("kset", "fused", 1, "fused"): ("test_gpu_spec", "test_custom_spec_matches_cpu_interpreter", ("kset-n16", "fused")),
    ("kses", "fused", 1, "fused"): ("test_gpu_spec", "test_custom_spec_matches_cpu_interpreter", ("kses-n16", "fused")),
    ("tpc", "fused", 1, "fused"): ("test_gpu_tpc", "test_reference_spec_equals_the_builtin_checks", ("8", "fused")),
}


def covered_cells():
    """cell -> first test id of this module that runs it."""
    out = {}

    def add(alg, cell, test):
        out.setdefault((alg,) + cell, test)

    for row, n in SEEDED:
        add(ROW[row].alg, dispatch(ROW[row].alg, n, case_cfg(row, n).sched, "seeded"),
            f"test_seeded_matches_oracle[{row}-n{n}]")
    for row, n in TRACED:
        add(ROW[row].alg, dispatch(ROW[row].alg, n, case_cfg(row, n).sched, "traced"),
            f"test_traced_matches_oracle[{row}-n{n}]")
    for name, n in EXPLICIT_CASES:
        add(name, dispatch(name, n, explicit_cfg(name, n).sched, "explicit"), f"test_explicit_matches_oracle[{name}-n{n}]")
    for row, n in FUSED:
        add(ROW[row].alg, dispatch(ROW[row].alg, n, case_cfg(row, n).sched, "fused"),
            f"test_fused_matches_traced[{row}-n{n}]")
    for name, n in FUSED_X:
        add(ROW[name].alg, dispatch(ROW[name].alg, n, explicit_cfg(ROW[name].alg, n).sched, "fused-x"),
            f"test_fused_matches_traced_under_a_loaded_schedule[{name}-n{n}]")
    return out


def _parametrize_ids(fn):
    ids = set()
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        if m.kwargs.get("ids") is not None:
            ids |= {str(i) for i in m.kwargs["ids"]}
        else:
            for v in m.args[1]:
                ids.add("-".join(str(e) for e in v) if isinstance(v, (tuple, list)) else str(v))
    return ids


def test_every_cell_is_covered():
    """{10 algorithms} x {W = 1..4} x {the modes the algorithm has}: run by a case of this module,
    or left to a named test of another module that exists. The cells this module was written for
    (W > 1 everywhere, and W = 1 traced, fused-x and the explicit ones without a case) are its own."""
    own = covered_cells()
    need = required_cells()
    assert set(own) <= need and set(DELEGATED) <= need
    missing = sorted(need - set(own) - set(DELEGATED))
    assert not missing, f"{len(missing)} uncovered cells, first {missing[:8]}"
    assert all(c in own for c in need if c[2] > 1 or c[3] in ("traced", "fused-x"))
    for cell, (module, test, frags) in DELEGATED.items():
        fn = getattr(importlib.import_module(module), test)
        ids = _parametrize_ids(fn)
        assert all(f in ids for f in frags), (cell, module, test, frags)
    # the delegated W = 1 shapes are what their ids say
    assert all(c[2] == 1 for c in DELEGATED)


def coverage_table():
    """DESIGN.md's table of (algorithm, kernel, W) -> test, from the two tables above. A test without
    a module is one of this module; "-" marks a kernel the dispatch rule never gives at that W."""
    own, need = covered_cells(), required_cells()

    def test_of(cell):
        if cell not in need:
            return "-"
        if cell in own:
            return f"`{own[cell]}`"
        module, fn, frags = DELEGATED[cell]
        return f"`{module}.py::{fn}" + (f"[{'-'.join(frags)}]`" if frags else "`")

    lines = ["| algorithm | kernel | W = 1 | W = 2 | W = 3 | W = 4 |", "|---|---|---|---|---|---|"]
    kinds = sorted({(c[1], c[3]) for c in need})
    for alg in ALGS:
        for fam, flavour in kinds:
            if any((alg, fam, W, flavour) in need for W in (1, 2, 3, 4)):
                cells = " | ".join(test_of((alg, fam, W, flavour)) for W in (1, 2, 3, 4))
                lines.append(f"| {alg} | {fam}, {flavour} | {cells} |")
    return "\n".join(lines)


def test_design_table_is_the_generated_one():
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")
    with open(path) as f:
        text = f.read()
    begin, end = "<!-- instantiation-table:begin -->\n", "\n<!-- instantiation-table:end -->"
    assert begin in text and end in text
    assert text.split(begin)[1].split(end)[0] == coverage_table()
