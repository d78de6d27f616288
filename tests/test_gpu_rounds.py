"""GPU parity along the round-count axis: long live runs, R edges, coordinator rotation.

Everything is bit-exact against the CPU oracle (TwoPhaseCommit: against `py_tpc` on the
materialized schedule): batch summary, per-instance (digest, first_fail, term_round, n_checks,
n_decided), the decisions() arrays and fetched records.

1. Long live runs: seeded schedules that keep instances undecided past rounds 64 / 128 and let
   them decide late, so the 64-round refills of the good-round block (Sched::good_round) and of
   LastVoting's coordinator words (CoordWords::ho) run in instances whose results still depend
   on them. Each case's liveness is a precondition asserted on the oracle's records.
2. The same OTR / LastVoting runs through psg_run_batch_spec (trace + interpreter, fused hook),
   where the settled-round skip and the quiescent tail are off, incl. a Spec that reads |HO|.
3. R in {1, 2, phase - 1, phase + 1, 2 phase + 1} and PSG_MAX_ROUNDS for every algorithm.
4. Coordinator rotation past n (LastVoting, ShortLastVoting at n <= 3).
5. TwoPhaseCommit under every seeded schedule family (psg_tpc.hip's own HO assembly).

The `test_preconditions_hold_on_the_oracle_*` tests (no GPU) evaluate the preconditions of
parts 1, 2 and 4 on the oracle alone.

What the long runs can and cannot see was measured once with two scratch builds of the library:
`k - good_base >= 65` in Sched::good_round fails 9 of the 13 cases of part 1 (not lv-n64-crash,
lv-n3-V5, which has no good rounds, and the two FloodMin cases: a minimum that has flooded by
round 3 does not move with one misread round), `q - qbase >= 65` in CoordWords::ho fails
lv-n3-V5 alone (one misdrawn HO(coord), at k = 128, changes an n = 64 run only if that phase
would have succeeded). A refill that stays wrong after its first round is seen by every later
decision; the parity modules that existed before pass under both builds.
"""
import numpy as np
import pytest

from round_amd import abi, formula as F, psync, schedules as S

import spec_cases
from gpu_support import (BEGIN, assert_run_equals_oracle, cmp_instances, cmp_summary, rec_tuple, run_any, spec_rows,
                         tpc_seeded)
from restatement import tpc_outcomes

gpu = pytest.mark.gpu
H = psync.HOSchedule
LOSSY = H(drop_log2=1, good_round=0.02)  # links lost w.p. 1/2: progress only in the rare good rounds


# ------------------------------------------------------------------------------------ 1. long live runs
# (id, algorithm, n, R, instances, make_config kwargs). Oracle alone, shares of instances whose
# last decision round is >= 64 / >= 128 / >= 192:
#   otr-n64 120/44/14 of 200      otr2-n100 59/21/1 of 100      lv-n64-crash 44/24/6 of 200
#   lv-n130 16/10/1 of 60         lv-n3 127/53/18 of 300        slv-n64 65/39/19 of 200
#   slv-n5 84/41/24 of 300        benor-n64 82/36/7 of 200      benor-n200 16/8/2 of 60
#   fm-n64-f100 200/-/- of 200    fm-n256-f140 40/40/- of 40
#   kset-n40 11/0/0 of 60         kset-n66 3/0/0 of 30
LONG = [
    ("otr-n64-V64", psync.OTR(), 64, 250, 200, dict(value_range=64, schedule=LOSSY)),
    ("otr2-n100-W2", psync.OTR2(), 100, 200, 100, dict(value_range=8, schedule=LOSSY)),
    ("lv-n64-crash", psync.LastVoting(), 64, 250, 200, dict(schedule=H(drop_log2=1, good_round=0.02, crash_fmax=10))),
    ("lv-n130-W3", psync.LastVoting(), 130, 200, 60, dict(schedule=LOSSY)),
    # no good rounds: the coordinator rotates past n many times before a lucky phase. Pure HO: with
    # the self bit only 16 of 300 instances decide last at a round >= 64, below the 10 % asked
    ("lv-n3-V5", psync.LastVoting(), 3, 250, 300, dict(value_range=5, schedule=H(drop_log2=1, good_round=0.0,
                                                                                  self_bit=False))),
    ("slv-n64", psync.ShortLastVoting(), 64, 250, 200, dict(schedule=LOSSY)),
    ("slv-n5-V5", psync.ShortLastVoting(), 5, 250, 300, dict(value_range=5, schedule=H(drop_log2=1, good_round=0.01))),
    # BenOr without ho_min: its safety predicate is broken on purpose (the Safety slot fails, and
    # is compared like every other slot); the instances run on their coins alone
    ("benor-n64", psync.BenOr(), 64, 250, 200, dict(schedule=LOSSY)),
    ("benor-n200-W4", psync.BenOr(), 200, 200, 60, dict(schedule=H(drop_log2=1, good_round=0.01))),
    # FloodMin decides in round f + 1 only: every instance is live until then
    ("fm-n64-f100", psync.FloodMin(100), 64, 110, 200, dict(schedule=H(drop_log2=3, good_round=0.05, crash_fmax=30))),
    ("fm-n256-f140", psync.FloodMin(140), 256, 150, 40, dict(schedule=H(drop_log2=2, good_round=0.1, crash_fmax=64))),
    # KSet: sized for the Map-based oracle (about 2.5 s each). n = 40 is the group path (11 of 60
    # instances decide last at a round >= 64), n = 66 the lane-packed path (3 of 30, seed 2)
    ("kset-n40-k2", psync.KSetAgreement(2), 40, 130, 60, dict(schedule=H(drop_log2=1, good_round=0.02, crash_fmax=2))),
    ("kset-n66-k2", psync.KSetAgreement(2), 66, 80, 30, dict(seed=2, schedule=H(drop_log2=1, good_round=0.02,
                                                                                  crash_fmax=2))),
]
LONG_BY_ID = {c[0]: c for c in LONG}


def long_cfg(case):
    cid, alg, n, R, count, kw = case
    return psync.make_config(alg, n, rounds=R, batch_capacity=count, **kw)


_ORACLE = {}


def oracle_long(oracle_mod, cid):
    """The oracle's run of a LONG case (computed once per session, never modified):
    (cfg, summary, per-instance summaries, records, last decision round per instance)."""
    if cid not in _ORACLE:
        case = LONG_BY_ID[cid]
        cfg = long_cfg(case)
        osum, opi, orec = oracle_mod.run(cfg, BEGIN, case[4], per_instance=True, records=True, threads=8)
        last = np.array([r.decision_round for r in orec], np.int64).reshape(case[4], cfg.n).max(axis=1)
        _ORACLE[cid] = (cfg, osum, opi, orec, last)
    return _ORACLE[cid]


def has_late_good_round(oracle_mod, cfg, kmin=64, instances=4):
    """Some round k >= kmin of the first instances is good in the materialized schedule: the n HO
    sets, self bit aside, are one common set s. |s| is taken with the crashed senders put back
    (the generator removes them after drawing s) and must exceed good_min."""
    ho, cr = oracle_mod.materialize_schedule(cfg, BEGIN, instances)
    n, W = cfg.n, (cfg.n + 63) // 64
    good_min = cfg.sched.good_min if cfg.sched.good_min >= 0 else (2 * n) // 3
    notself = ~S.self_mask(n)  # [n][W]
    for i in range(instances):
        for k in range(kmin, cfg.rounds):
            common = np.bitwise_and.reduce(ho[i, k], axis=0)  # [W]
            if not ((ho[i, k] & notself) == (common[None] & notself)).all():
                continue
            size = sum(bin(int(common[w])).count("1") for w in range(W))
            size += int(((cr[i] >= 0) & (cr[i] <= k)).sum())
            if size > good_min:
                return True
    return False


def check_long_preconditions(oracle_mod, cid):
    """The liveness a LONG case exists for, on the oracle's records alone."""
    cid, alg, n, R, count, kw = LONG_BY_ID[cid]
    cfg, _, _, _, last = oracle_long(oracle_mod, cid)
    ge64, ge128 = int((last >= 64).sum()), int((last >= 128).sum())
    assert 10 * ge64 >= count, f"{cid}: {ge64} of {count} instances decide last at a round >= 64"
    if R >= 200:
        assert 20 * ge128 >= count, f"{cid}: {ge128} of {count} instances decide last at a round >= 128"
        # progress late: decisions both in [64, 128) and in [128, R)
        assert ge64 > ge128 >= 1
    if cid == "lv-n3-V5":  # the coordinator wrap: a decision in a phase >= n
        assert int((last // alg.phase_length >= n).sum()) >= 1
    if cid == "lv-n64-crash":
        # a decision at k >= 131 follows an instance-wide R0 at k >= 128 (coordinator round 64)
        assert int((last >= 131).sum()) >= 3
    if cfg.sched.good_p32:
        assert has_late_good_round(oracle_mod, cfg), f"{cid}: no good round at k >= 64 in the first instances"


def fetch_sample(count, last):
    """About 20 ids, the latest decider among them."""
    return sorted({BEGIN + i for i in range(0, count, max(1, count // 19))} | {BEGIN + int(np.argmax(last))})


@gpu
@pytest.mark.parametrize("cid", [c[0] for c in LONG])
def test_long_live_run_matches_oracle(cid, oracle_mod):
    """Instances still undecided after rounds 64 and 128 (precondition, on the oracle) decide as
    the oracle's do: the refills of the 64-round good-round block and of LastVoting's coordinator
    words, the partial phases' bookkeeping over many phases, check points up to R.
    KSet is sized for the Map-based oracle: at n = 40, R = 130 11 of 60 instances decide last at a
    round >= 64 (18 %), at n = 66, R = 80 (lane-packed) 3 of 30 (10 %, seed 2); none past 128."""
    cid, alg, n, R, count, kw = LONG_BY_ID[cid]
    check_long_preconditions(oracle_mod, cid)
    cfg, osum, opi, orec, last = oracle_long(oracle_mod, cid)
    with psync.GpuRound(alg, n, R, batch_capacity=count, **kw) as gr:
        assert bytes(gr.cfg) == bytes(cfg)
        assert_run_equals_oracle(gr, count, osum, opi, orec, fetch_sample(count, last))


# KSetEarlyStopping stops early by design (the oracle shows every decision by round 4 under these
# schedules), so these runs cover the frozen / check-only path at high check-point numbers and
# not the refill. EpsilonConsensus with epsilon = 1e-300 has maxR beyond R: no process decides,
# every instance stays live through all R rounds under good rounds and crashes, and the compared
# final values depend on every round's HO sets.
FROZEN = [(f"{name}-n{n}-R{R}", alg, n, R, sched(n))
          for name, alg, ns, sched in [
              ("kses", psync.KSetEarlyStopping(200, 1), (64, 130),
               lambda n: H(drop_log2=2, good_round=0.05, crash_fmax=20)),
              ("eps", psync.EpsilonConsensus(5, 1e-300), (64, 100),
               lambda n: H(drop_log2=3, good_round=0.05, crash_fmax=5, ho_min=n - 6))]
          for n in ns for R in (70, 250)]


@gpu
@pytest.mark.parametrize("cid,alg,n,R,sched", FROZEN, ids=[c[0] for c in FROZEN])
def test_high_check_point_numbers_match_oracle(cid, alg, n, R, sched, oracle_mod):
    """Parity at R = 70 and 250 under good rounds and crashes. KSetEarlyStopping: the frozen /
    check-only path at high check-point numbers, not the good-round refill (every decision falls by
    round 4). EpsilonConsensus: live to round R, but with no decision to compare past round 64."""
    count = 100
    with psync.GpuRound(alg, n, R, schedule=sched, batch_capacity=count) as gr:
        opi, orec = run_any(gr, oracle_mod, count, [BEGIN + i for i in range(0, count, 5)])
    if alg.real:
        assert all(r.decision_round < 0 for r in orec)  # live to the end: maxR > R


# ------------------------------------------------------------------------------------ 2. shortcuts off
@gpu
@pytest.mark.parametrize("mode", ["vm", "fused", "vm-ho", "fused-ho"])
@pytest.mark.parametrize("cid", ["otr-n64-V64", "lv-n64-crash"])
def test_long_live_run_under_a_spec_program(cid, mode, oracle_mod):
    """The trace-writing and fused-hook instantiations of the round kernels call good_round in
    every round: the reference Spec over the long live runs of part 1 gives the built-in run's
    first_fail, term_round and digest per instance, and that run is the oracle's."""
    cid, alg, n, R, count, kw = LONG_BY_ID[cid]
    check_long_preconditions(oracle_mod, cid)
    cfg, osum, opi, orec, last = oracle_long(oracle_mod, cid)
    spec = spec_cases.ref_with_ho_bound(alg.alg_id) if mode.endswith("-ho") else F.REFERENCE_SPECS[alg.alg_id]()
    if mode.startswith("vm"):
        prog = F.compile_spec(spec, alg.alg_id)
    else:
        prog = F.compile_native(spec, alg.alg_id, fused=True, n=n)
    ref_names = F.compile_spec(F.REFERENCE_SPECS[alg.alg_id](), alg.alg_id).slot_names
    k = len(ref_names)  # the built-in checks' slots, in their order
    assert prog.slot_names[:k] == ref_names == alg.check_names[:k]
    with psync.GpuRound(alg, n, R, batch_capacity=count, **kw) as gr:
        built = gr.run(BEGIN, count, per_instance=True)
        sp = gr.run_spec(BEGIN, count, prog, per_instance=True)
    cmp_instances(built.per_instance, opi)
    assert spec_rows(sp.per_instance, k, digest=True) == spec_rows(built.per_instance, k, digest=True)
    assert list(sp.summary.fail_count)[:k] == list(built.summary.fail_count)[:k]
    if mode.endswith("-ho"):  # |HO(p)| <= n holds at every check point
        assert all(s.first_fail[len(prog.slot_names) - 1] == abi.PSG_NEVER for s in sp.per_instance)


# ------------------------------------------------------------------------------------ 3. round-count edges
# (name, algorithm, n of the W = 1 shape, n > 64, extra R). FloodMin(4) decides in round k = f + 1,
# the (f + 2)-th: R <= f and R = f + 1 (nobody decides), f + 2, f + 3; KSetEarlyStopping(8, 2): t / k
# and t / k + 1.
EDGE_ALGS = [
    ("otr", psync.OTR(), 5, 130, ()),
    ("otr2", psync.OTR2(), 7, 65, ()),
    ("lv", psync.LastVoting(), 5, 130, ()),
    ("slv", psync.ShortLastVoting(), 7, 65, ()),
    ("benor", psync.BenOr(), 5, 130, ()),
    ("fm", psync.FloodMin(4), 7, 65, (4, 5, 6, 7)),
    ("kset", psync.KSetAgreement(2), 5, 130, ()),
    ("kses", psync.KSetEarlyStopping(8, 2), 7, 65, (4, 5)),
    ("eps", psync.EpsilonConsensus(1, 0.1), 7, 130, ()),
]


def edge_rounds(phase, extra=()):
    return sorted({R for R in (1, 2, phase - 1, phase + 1, 2 * phase + 1) if R >= 1} | set(extra))


EDGES = [(f"{name}-n{n}-R{R}", alg, n, R) for name, alg, n1, nw, extra in EDGE_ALGS for n in (n1, nw)
         for R in edge_rounds(alg.phase_length, extra)]


@gpu
@pytest.mark.parametrize("cid,alg,n,R", EDGES, ids=[c[0] for c in EDGES])
def test_round_count_edges_match_oracle(cid, alg, n, R, oracle_mod):
    """One round, a partial last phase, one round past a phase: the default schedule, the group
    kernel (W = 1) and the kernels for n > 64."""
    count = 300 if n <= 64 else 100
    with psync.GpuRound(alg, n, R, seed=3, batch_capacity=count) as gr:
        opi, orec = run_any(gr, oracle_mod, count, [BEGIN + i for i in range(0, count, max(1, count // 19))])
    if alg.alg_id == abi.PSG_ALG_FLOODMIN:  # decides in round k = f + 1 only
        assert {r.decision_round for r in orec} <= {-1, alg.param + 1}
        assert any(r.decision_round >= 0 for r in orec) == (R >= alg.param + 2)


@gpu
@pytest.mark.parametrize("R", edge_rounds(3))
def test_round_count_edges_tpc_wide(R, oracle_mod):
    """TwoPhaseCommit at n > 64, seeded (its explicit-schedule edges are in test_gpu_tpc.py)."""
    tpc_seeded(130, R, 129, None, 48, 3, oracle_mod)


MAXR = [
    ("otr2", psync.OTR2()), ("lv", psync.LastVoting()), ("slv", psync.ShortLastVoting()), ("benor", psync.BenOr()),
    ("fm", psync.FloodMin(2)), ("kset", psync.KSetAgreement(2)), ("kses", psync.KSetEarlyStopping(2, 2)),
    ("eps", psync.EpsilonConsensus(1, 0.1)),
]


@gpu
@pytest.mark.parametrize("name,alg", MAXR, ids=[c[0] for c in MAXR])
def test_max_rounds_match_oracle(name, alg, oracle_mod):
    """PSG_MAX_ROUNDS check points in each kernel's per-lane record and term_hist[R + 1]."""
    count, n = 100, 7 if alg.real else 5
    with psync.GpuRound(alg, n, abi.PSG_MAX_ROUNDS, seed=4, batch_capacity=count) as gr:
        run_any(gr, oracle_mod, count, [BEGIN + i for i in range(0, count, 5)])


@gpu
def test_max_rounds_tpc(oracle_mod):
    tpc_seeded(5, abi.PSG_MAX_ROUNDS, 4, None, 100, 4, oracle_mod)


# ------------------------------------------------------------------------------------ 4. coordinator rotation
ROTATION = [(f"{name}-n{n}-{'champ' if tb == abi.PSG_TIE_CHAMP else 'minpid'}", alg, n, tb)
            for name, alg in (("lv", psync.LastVoting()), ("slv", psync.ShortLastVoting()))
            for n, tbs in ((1, (abi.PSG_TIE_CHAMP,)), (2, (abi.PSG_TIE_CHAMP,)),
                           (3, (abi.PSG_TIE_CHAMP, abi.PSG_TIE_MIN_PID)))
            for tb in tbs]
ROT_R, ROT_COUNT = 40, 300
ROT_KW = dict(value_range=3, schedule=H(drop_log2=1, good_round=0.0))


def check_rotation_precondition(alg, n, orec, count):
    """Some instance decides in a phase >= n: its coordinator index has wrapped. A single process
    always hears itself and decides in phase 0 (all of them do, asserted), so n = 1 covers the
    wrap in the check points' coordinator only."""
    last = np.array([r.decision_round for r in orec], np.int64).reshape(count, n).max(axis=1)
    if n == 1:
        assert (last == alg.phase_length - 1).all()
    else:
        assert int((last // alg.phase_length >= n).sum()) >= 1


@gpu
@pytest.mark.parametrize("cid,alg,n,tb", ROTATION, ids=[c[0] for c in ROTATION])
def test_coordinator_rotation_matches_oracle(cid, alg, n, tb, oracle_mod):
    with psync.GpuRound(alg, n, ROT_R, tiebreak=tb, batch_capacity=ROT_COUNT, **ROT_KW) as gr:
        osum, opi, orec = oracle_mod.run(gr.cfg, BEGIN, ROT_COUNT, per_instance=True, records=True, threads=8)
        check_rotation_precondition(alg, n, orec, ROT_COUNT)
        assert_run_equals_oracle(gr, ROT_COUNT, osum, opi, orec, [BEGIN + i for i in range(0, ROT_COUNT, 15)])


def rotation_explicit_inputs():
    rng = np.random.default_rng(60)
    n, R, I = 3, 60, 300
    return n, R, I, S.random_omission(rng, I, R, n, 0.7), rng.integers(1, 4, (I, n), dtype=np.int32)


@gpu
def test_coordinator_rotation_explicit_schedule(oracle_mod):
    """LastVoting, n = 3, 15 phases through psg_load_schedule (the explicit-schedule kernel reads
    HO(coord) from the loaded sets, not from CoordWords)."""
    n, R, I, ho, init = rotation_explicit_inputs()
    alg = psync.LastVoting()
    with psync.GpuRound(alg, n, R, seed=5, value_range=3, batch_capacity=I) as g:
        ctx = g._ctx
        ctx.load_inputs(BEGIN, I, init)
        ctx.load_schedule(BEGIN, I, ho, None)
        s, pi = ctx.run_batch_np(BEGIN, I)
        dec, dr = ctx.copy_decisions_np()
        fs, fr = ctx.fetch_np(np.arange(BEGIN, BEGIN + I, 15, dtype=np.uint64))
    osum, opi, orec, _, _ = oracle_mod.run_schedule(g.cfg, BEGIN, I, ho, None, init, per_instance=True, records=True)
    check_rotation_precondition(alg, n, orec, I)
    cmp_summary(s, osum, R)
    cmp_instances(pi, opi)
    orr = np.array([rec_tuple(r) for r in orec], np.int64).reshape(I, n, 4)
    assert (dec == orr[:, :, 0]).all() and (dr == orr[:, :, 1]).all()
    for j, i in enumerate(range(0, I, 15)):
        assert int(fs[j]["digest"]) == opi[i].digest
        got = np.stack([fr[j][f] for f in ("decision", "decision_round", "halt_round", "final_x")], axis=1)
        assert (got == orr[i]).all(), i


# ------------------------------------------------------------------------------------ 5. TwoPhaseCommit, seeded
TPC_FAMILIES = [
    ("crash", lambda n: H(drop_log2=2, crash_fmax=n // 3)),
    ("good", lambda n: H(drop_log2=1, good_round=0.5)),
    ("homin", lambda n: H(drop_log2=1, ho_min=n // 2)),
    ("pureho", lambda n: H(drop_log2=3, self_bit=False, crash_fmax=2)),
    ("crashall", lambda n: H(drop_log2=0, crash_fmax=n - 1)),
]


def tpc_expected_outcomes(family, n):
    """Outcomes the instances of a case must hold. A commit needs the coordinator to hear all n
    votes in slot 1: under "good" (a good round's common set is everybody once it is not above
    good_min), "homin" (a set of at most n / 2 is raised to everybody) and "crashall" (no loss,
    sometimes no crash) that happens in many instances; under "crash" and "pureho" every link
    to the coordinator is lost independently w.p. 1/4 or 1/8, so at n >= 64 no instance commits
    ((7/8)^63 < 1e-3) and the case holds the other two outcomes."""
    if n >= 64 and family in ("crash", "pureho"):
        return {"abort", "suspect"}
    return {"commit", "abort", "suspect"}

TPC_SEEDED = [(f"{name}-n{n}-R{R}", name, n, R) for name, _ in TPC_FAMILIES for n in (5, 64, 130, 256) for R in (3, 5)]


@gpu
@pytest.mark.parametrize("cid,family,n,R", TPC_SEEDED, ids=[c[0] for c in TPC_SEEDED])
def test_tpc_seeded_families_equal_the_restatement(cid, family, n, R, oracle_mod):
    """psg_tpc.hip assembles its HO sets itself (tpc_ho, a copy of Sched::assemble): crash sets,
    ho_min, good rounds and the per-word self bit, with the coordinator in the last mask word.
    py_tpc knows nothing of crash rounds: the omissions are in the exported HO sets."""
    sched = dict(TPC_FAMILIES)[family](n)
    cnt = 64 if n <= 130 else 32
    runs, cr = tpc_seeded(n, R, n - 1, sched, cnt, 7, oracle_mod)
    assert tpc_outcomes(runs) == tpc_expected_outcomes(family, n)
    if family in ("crash", "crashall"):
        assert (cr[:, n - 1] >= 0).any(), "the coordinator crashes in no instance"
    else:  # at most 2 crashes among n: some process crashes, rarely the coordinator
        assert (cr >= 0).any() == (family == "pureho")


# ------------------------------------------------------------------------------------ CPU-side guard
@pytest.mark.parametrize("cid", [c[0] for c in LONG])
def test_preconditions_hold_on_the_oracle_long(cid, oracle_mod):
    """Parts 1 and 2 without a GPU: the inputs keep the instances live as the case table says."""
    check_long_preconditions(oracle_mod, cid)


def test_preconditions_hold_on_the_oracle_rotation(oracle_mod):
    """Part 4 without a GPU: decisions in phases >= n, seeded and under the explicit schedule."""
    for cid, alg, n, tb in ROTATION:
        cfg = psync.make_config(alg, n, rounds=ROT_R, tiebreak=tb, batch_capacity=ROT_COUNT, **ROT_KW)
        _, _, orec = oracle_mod.run(cfg, BEGIN, ROT_COUNT, records=True, threads=8)
        check_rotation_precondition(alg, n, orec, ROT_COUNT)
    n, R, I, ho, init = rotation_explicit_inputs()
    cfg = psync.make_config(psync.LastVoting(), n, rounds=R, seed=5, value_range=3, batch_capacity=I)
    _, _, orec, _, _ = oracle_mod.run_schedule(cfg, BEGIN, I, ho, None, init, records=True)
    check_rotation_precondition(psync.LastVoting(), n, orec, I)
