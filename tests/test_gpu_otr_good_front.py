"""The good rounds of the seeded W = 1 OTR / OTR2 kernels (psg_device.hpp GoodFront): rounds 0..3
of eight consecutive batch rows are drawn in one Philox pass (lane = row + 8 * round + 32 * call),
rounds 4 and later per instance, 32 rounds a pass (lanes 0..31 the first call of a round's global
stream, lanes 32..63 the second). Which lane draws a word does not change the word, so every
result equals the CPU oracle's: per-instance digest, first_fail, term_round, n_checks, n_decided,
the decisions and their rounds, and the batch summary.

Every case first asserts, on the oracle's own output, that the regime it names is reached.
"""
import numpy as np
import pytest

from round_amd import psync

from gpu_support import cmp_instances, cmp_summary, inst_tuple, otr_alg, rec_tuple

pytestmark = pytest.mark.gpu

H = psync.HOSchedule
# Copies of GoodFront::kRounds and GoodFront::kLate (psg_device.hpp): change them together with
# the kernel's, or the regime assertions below keep guarding the old block boundaries.
FRONT_ROUNDS, LATE_ROUNDS = 4, 32


def _cfg(alg, n, rounds, **kw):
    return psync.make_config(alg, n, rounds=rounds, **kw)


def _oracle(oracle_mod, cfg, begin, count):
    return oracle_mod.run(cfg, begin, count, per_instance=True, records=True, threads=8)


def _gpu_equals_oracle(alg, n, rounds, begin, count, ora, **kw):
    """Run [begin, begin + count) on the GPU and compare everything with the oracle's `ora`."""
    osum, opi, orec = ora
    with psync.GpuRound(alg, n, rounds=rounds, batch_capacity=count, **kw) as g:
        res = g.run(begin, count, per_instance=True)
        dec, dround = g.decisions()
    cmp_instances(res.per_instance, opi)
    assert list(dec) == [r.decision for r in orec]
    assert list(dround) == [r.decision_round for r in orec]
    cmp_summary(res.summary, osum, rounds)


def _common(oracle_mod, cfg, begin, count):
    """common[i][k]: every process of instance begin + i has the same HO set in round k, up to the
    self bits (the rows of a good round's common set differ only there), and full[i][k]: that set
    is all n processes."""
    n = cfg.n
    ho, _ = oracle_mod.materialize_schedule(cfg, begin, count)
    own = np.array([1 << p for p in range(n)], dtype=np.uint64).reshape(1, 1, n, 1)
    one = np.uint64(1)  # process 0's own bit, set in its row only
    common = ((ho | own | one) == (ho[:, :, :1, :] | own | one)).all(axis=(2, 3))
    full = (ho[:, :, :, 0] == np.uint64((1 << n) - 1)).all(axis=2)
    return common, full


# --------------------------------------------------------------------------- 1. block boundaries
@pytest.mark.parametrize("name", ["otr", "otr2"])
def test_block_boundaries_with_live_instances(name, oracle_mod):
    """The quorum mutant (variant = 1) at n = 5 under heavy loss keeps a fifth of the instances
    undecided to the last round, so good rounds are read on both sides of the front block's end
    (rounds 3 | 4) and of the later blocks' ends (35 | 36, 67 | 68). The ids start at 2^32 - 37:
    the low id word carries inside a front block of eight rows. drop_log2 = 1 at n = 5 also sends
    most common sets to at most good_min = 3 members, where they become the full set."""
    n, R, count, begin = 5, 70, 300, 2 ** 32 - 37
    alg = otr_alg(name, variant=1)
    kw = dict(seed=5, value_range=64, schedule=H(drop_log2=1, good_round=0.25))
    cfg = _cfg(alg, n, R, **kw)
    ora = _oracle(oracle_mod, cfg, begin, count)
    osum, opi, orec = ora
    assert begin % 8 != 0 and (begin + 37) == 2 ** 32 and 37 % 8 != 0  # the carry falls inside a block of rows
    live = []
    for i in range(count):
        recs = orec[i * n:(i + 1) * n]
        steps = max(r.halt_round + 1 if r.halt_round >= 0 else R for r in recs)
        if steps == R and any(r.decision_round < 0 for r in recs):
            live.append(i)
    assert len(live) >= 20, len(live)
    assert min(live) < 37 <= max(live)  # on both sides of the carry
    common, full = _common(oracle_mod, cfg, begin, count)
    edges = {FRONT_ROUNDS - 1, FRONT_ROUNDS}
    for b in range(FRONT_ROUNDS + LATE_ROUNDS, R, LATE_ROUNDS):
        edges |= {b - 1, b}
    assert edges >= {3, 4, 35, 36, 67, 68}
    per_round = {k: int(common[live, k].sum()) for k in sorted(edges)}
    print("live undecided instances", len(live), "with a common set at round", per_round)
    assert all(v >= 5 for v in per_round.values()), per_round
    # |s| <= good_min -> full: P(at most 3 of 5 kept at loss 1/2) = 26/32, so most common sets are full
    assert full.any() and 2 * int(full.sum()) > int(common.sum())
    _gpu_equals_oracle(alg, n, R, begin, count, ora, **kw)


# --------------------------------------------------------------------------- 2. drop words
@pytest.mark.parametrize("drop_log2", [0, 2, 3, 4, 6])
@pytest.mark.parametrize("name", ["otr", "otr2"])
def test_drop_words(name, drop_log2, oracle_mod):
    """drop_log2 = 0: no drop words; 2: words 1 and 2 (both calls); 3: words 1..3 (both calls in
    full); 4 and 6: words past the second call."""
    n, R, count, begin = 64, 20, 200, 1000
    kw = dict(seed=31, value_range=64, schedule=H(drop_log2=drop_log2, good_round=0.5))
    cfg = _cfg(otr_alg(name), n, R, **kw)
    common, _ = _common(oracle_mod, cfg, begin, 40)
    if drop_log2 == 0:  # no loss: every round has the common (full) set
        assert common.all()
    else:
        assert common[:, :FRONT_ROUNDS].any() and not common[:, :FRONT_ROUNDS].all()
        assert common[:, FRONT_ROUNDS:].any() and not common[:, FRONT_ROUNDS:].all()
    ora = _oracle(oracle_mod, cfg, begin, count)
    assert ora[0].decided_processes > 0
    _gpu_equals_oracle(otr_alg(name), n, R, begin, count, ora, **kw)


# --------------------------------------------------------------------------- 3. row grouping
def test_row_grouping_and_fetch(oracle_mod):
    """One batch of 37 rows == its parts [B, B+5), [B+5, B+18), [B+18, B+37) (front blocks of eight
    rows at three alignments to the ids, the last ones cut short) == the fetch path on a shuffled,
    non-consecutive subset of the ids plus one id >= 2^64 - 2 (a front block's rows past the id
    list, and an id whose consecutive successors would wrap)."""
    n, R, B, count = 64, 20, 1003, 37
    kw = dict(seed=32, value_range=64)
    assert H().good_round == 0.25 and H().drop_log2 == 3
    cfg = _cfg(psync.OTR(), n, R, **kw)
    osum, opi, orec = _oracle(oracle_mod, cfg, B, count)
    common, _ = _common(oracle_mod, cfg, B, count)
    assert common[:, :FRONT_ROUNDS].any() and sum(1 for v in list(osum.term_hist)[:R + 2] if v) >= 2
    rng = np.random.default_rng(7)
    ids = [B + int(j) for j in rng.permutation(count)[:14]] + [2 ** 64 - 2]
    rng.shuffle(ids)
    assert sorted(ids) != ids and any(b - a > 1 for a, b in zip(sorted(ids), sorted(ids)[1:]))
    _, fpi, frec = oracle_mod.run(cfg, ids=ids, per_instance=True, records=True, threads=4)
    with psync.GpuRound(psync.OTR(), n, rounds=R, batch_capacity=count, **kw) as g:
        res = g.run(B, count, per_instance=True)
        dec, dround = g.decisions()
        cmp_instances(res.per_instance, opi)
        cmp_summary(res.summary, osum, R)
        assert list(dec) == [r.decision for r in orec]
        assert list(dround) == [r.decision_round for r in orec]
        for lo, hi in ((0, 5), (5, 18), (18, 37)):
            part = g.run(B + lo, hi - lo, per_instance=True)
            pdec, pdround = g.decisions()
            assert [inst_tuple(s) for s in part.per_instance] == [inst_tuple(s) for s in res.per_instance[lo:hi]]
            assert list(pdec) == list(dec[lo * n:hi * n]) and list(pdround) == list(dround[lo * n:hi * n])
        fsums, frecs = g.fetch(ids)
    for j, inst in enumerate(ids):
        assert inst_tuple(fsums[j]) == inst_tuple(fpi[j]), inst
        assert [rec_tuple(r) for r in frecs[j * n:(j + 1) * n]] == [rec_tuple(r) for r in frec[j * n:(j + 1) * n]], inst
        if inst < B + count:
            assert inst_tuple(fsums[j]) == inst_tuple(res.per_instance[inst - B]), inst


# --------------------------------------------------------------------------- 4. lanes past n, small R
SMALL = [(n, 20) for n in (1, 33, 63)] + [(64, R) for R in (1, 3, 4, 5)]
SMALL_CASES = [(a, n, R, p) for a in ("otr", "otr2") for n, R in SMALL for p in (1.0, 0.25)]


@pytest.mark.parametrize("name,n,R,p", SMALL_CASES, ids=[f"{a}-n{n}-R{R}-good{p}" for a, n, R, p in SMALL_CASES])
def test_lanes_past_n_and_small_round_counts(name, n, R, p, oracle_mod):
    """n below 64: the common set is cut to n processes and measured against 2n/3. R below, at and
    just past the front block's four rounds: rounds past R are never good."""
    count, begin = 200, 1000
    kw = dict(seed=33, value_range=64, schedule=H(drop_log2=3, good_round=p))
    cfg = _cfg(otr_alg(name), n, R, **kw)
    common, _ = _common(oracle_mod, cfg, begin, 40)
    if p == 1.0 or n == 1:  # (one process: its row is the set)
        assert common.all()
    else:
        assert common.any() and not common.all()
    ora = _oracle(oracle_mod, cfg, begin, count)
    assert ora[0].instances == count
    _gpu_equals_oracle(otr_alg(name), n, R, begin, count, ora, **kw)
