"""OTR / OTR2 check points on the GPU: the settled fast path's per-lane record, the
no-witness arm and the witness arm of otr_check (psg_otr.hip), bit-exact against the CPU
oracle on (digest, first_fail, term_round, n_checks, n_decided) per instance and on
the batch summary.

A frozen check point sees the state of the last live check point before it, so it can never
hold a slot's first failure: a frozen evaluation that misses a failure shows in no output,
only a false failure does. The live and the frozen settled check points are therefore one
function (otr_check_settled), and the first test drives the live one to a first failure at
the exact threshold.
"""
import numpy as np
import pytest

from round_amd import abi, psync

from gpu_support import cmp_instances, cmp_summary, inst_tuple, otr_alg

pytestmark = pytest.mark.gpu

H = psync.HOSchedule
NEVER = 0xFF


# --------------------------------------------------------------------------- 1. exact threshold
def _bits(lo, hi):
    return sum(1 << q for q in range(lo, hi))


def _scenario(n, ones, dev, R):
    """Initial values [1]*ones + [2]*twos. Round 0: pids < ones hear [0, ones), the rest nobody.
    Round 1: pids < dev hear [ones - m, n), the rest [0, ones). Later rounds: nobody hears
    anybody. With the mutant's quorum n // 2 every process has decided 1 after round 1 and dev
    of them hold x = 2, so check point 2 is settled with cnt = n - dev."""
    twos = n - ones
    m = n // 2 + 1 - twos
    init = [1] * ones + [2] * twos
    ho = [[0] * n for _ in range(R)]
    for p in range(ones):
        ho[0][p] = _bits(0, ones)
    for p in range(n):
        ho[1][p] = (_bits(ones - m, ones) | _bits(ones, n)) if p < dev else _bits(0, ones)
    return init, ho


def _reversed(n, init, ho):
    """The same instance with pid p renamed n - 1 - p (lane 0 then holds 2 and decides last)."""
    def rev(mask):
        return sum(1 << (n - 1 - q) for q in range(n) if (mask >> q) & 1)
    return init[::-1], [[rev(row[n - 1 - p]) for p in range(n)] for row in ho]


THRESHOLD_ROWS = [
    # (id, algorithm, (n, ones, dev), first_fail, term_round)
    ("otr-n24", psync.OTR(variant=1), (24, 17, 9), [255, 2, 0, 0, 255, 255, 255, 255], 2),
    ("otr-n64-cnt42", psync.OTR(variant=1), (64, 43, 22), [255, 2, 0, 0, 255, 255, 255, 255], 2),  # cnt = 2n/3
    ("otr-n64-cnt43", psync.OTR(variant=1), (64, 43, 21), [255, 255, 0, 0, 255, 255, 255, 255], 2),  # holds
    ("otr-n63", psync.OTR(variant=1), (63, 43, 21), [255, 2, 0, 0, 255, 255, 255, 255], 2),
    ("otr2-n64-cnt42", psync.OTR2(variant=1), (64, 43, 22), [255, 255, 0, 255, 255, 255, 255, 255], 2),
]


@pytest.mark.parametrize("cid,alg,shape,want_ff,want_term", THRESHOLD_ROWS, ids=[r[0] for r in THRESHOLD_ROWS])
def test_first_failure_through_settled_path_at_threshold(cid, alg, shape, want_ff, want_term, oracle_mod):
    """Slot 1 (Invariant0) first fails at a settled live check point, with the vote count
    exactly at, and one above, 2n/3; the pid-reversed copy puts the value 2 on lane 0."""
    n, ones, dev = shape
    R, begin = 6, 1000
    sched = H(drop_log2=0, good_round=0.0, self_bit=False)
    init, ho = _scenario(n, ones, dev, R)
    rinit, rho = _reversed(n, init, ho)
    cfg = psync.make_config(alg, n, rounds=R, seed=1, value_range=2, schedule=sched)
    rows = []
    for i_, h_ in ((init, ho), (rinit, rho)):
        s, _, tr = oracle_mod.run_explicit(cfg, i_, h_)
        rows.append(s)
        # the oracle's own output first, so that the comparison below is not vacuous
        assert list(s.first_fail)[:8] == want_ff and s.term_round == want_term
        x2, d2 = tr[2]
        assert all(d2) and sum(1 for v in x2 if v == 1) == n - dev  # settled at check point 2, cnt = n - dev
    assert inst_tuple(rows[0])[1:] == inst_tuple(rows[1])[1:]  # OTR is symmetric in pids
    slot1_fails = want_ff[1] != NEVER
    assert slot1_fails == (not isinstance(alg, psync.OTR2) and n - dev <= (2 * n) // 3)
    ho_np = np.array([ho, rho], dtype=np.uint64).reshape(2, R, n, 1)
    init_np = [init, rinit]
    with psync.GpuRound(alg, n, R, seed=1, value_range=2, schedule=sched, batch_capacity=2) as g:
        g.load_inputs(begin, 2, init_np)
        g.load_schedule(begin, 2, ho_np)
        res = g.run(begin, 2, per_instance=True)
    osum, opi, _, _, _ = oracle_mod.run_schedule(g.cfg, begin, 2, ho_np, None, init_np, per_instance=True)
    assert [inst_tuple(s)[1:] for s in opi] == [inst_tuple(s)[1:] for s in rows]
    cmp_instances(res.per_instance, opi)
    cmp_summary(res.summary, osum, R)


# --------------------------------------------------------------------------- 2. threshold shapes
SHAPES = [(a, n, V) for a in ("otr", "otr2") for n in (1, 2, 3, 4, 5, 63, 64) for V in (1, 2, 64)]


def _no_late_failures(opi):
    late = [k for k in range(8) if any(s.first_fail[k] not in (0, NEVER) for s in opi)]
    assert not late, f"the oracle fails slots {late} after check point 0"


@pytest.mark.parametrize("name,n,V", SHAPES, ids=[f"{a}-n{n}-V{V}" for a, n, V in SHAPES])
def test_threshold_shapes_seeded(name, n, V, oracle_mod):
    """Small and full waves, under the default schedule: no slot ever fails after check point
    0 on the oracle, so any difference is a false failure from the per-lane thresholds or from
    lanes past n."""
    begin, count = 1000, 400
    with psync.GpuRound(otr_alg(name), n, rounds=20, seed=11, value_range=V, batch_capacity=count) as g:
        res = g.run(begin, count, per_instance=True)
    osum, opi, _ = oracle_mod.run(g.cfg, begin, count, per_instance=True, threads=8)
    _no_late_failures(opi)
    if V == 1:  # every x is the same value from the start: OTR fails only Invariant2 (nobody decided yet)
        failing = [k for k in range(8) if osum.fail_count[k]]
        assert failing == ([] if name == "otr2" else [3])
    cmp_instances(res.per_instance, opi)
    cmp_summary(res.summary, osum, 20)


def test_threshold_shapes_max_rounds(oracle_mod):
    """rounds = PSG_MAX_ROUNDS: check-point numbers up to 250 in the per-lane record."""
    begin, count, R = 1000, 200, abi.PSG_MAX_ROUNDS
    with psync.GpuRound(psync.OTR(), 64, rounds=R, seed=12, value_range=64, batch_capacity=count) as g:
        res = g.run(begin, count, per_instance=True)
    osum, opi, _ = oracle_mod.run(g.cfg, begin, count, per_instance=True, threads=8)
    _no_late_failures(opi)
    cmp_instances(res.per_instance, opi)
    cmp_summary(res.summary, osum, R)


# --------------------------------------------------------------------------- 3. witness arm
@pytest.mark.parametrize("name", ["otr", "otr2"])
def test_witness_arm(name, oracle_mod):
    """The mutant under heavy loss: processes decide different values, so the exact arm resolves
    keepInit / Validity / Agreement / Irrevocability with a ballot each. OTR fails slots 0, 1, 4,
    6 and 7 on the oracle, with first failures spread over check points 1 to 9. Slot 5 (Validity)
    cannot fail with these inputs: every x, and so every decision, is some process's initial
    value. For OTR2 the oracle is the expectation, with no fixed counts."""
    begin, count = 1000, 3000
    with psync.GpuRound(otr_alg(name, variant=1), 5, rounds=20, seed=7, value_range=3,
                        schedule=H(drop_log2=1, good_round=0.0), batch_capacity=count) as g:
        res = g.run(begin, count, per_instance=True)
    osum, opi, _ = oracle_mod.run(g.cfg, begin, count, per_instance=True, threads=8)
    if name == "otr":
        for k in (0, 1, 4, 6, 7):
            assert osum.fail_count[k] >= 1, f"slot {k} never fails on the oracle"
    assert osum.fail_count[5] == 0
    cmp_instances(res.per_instance, opi)
    cmp_summary(res.summary, osum, 20)
