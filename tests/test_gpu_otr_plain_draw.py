"""The plain-schedule form of the seeded W = 1 OTR / OTR2 kernels (psg_otr.hip PLAIN, psg_device.hpp
Sched::ho_plain): a launch whose schedule has no crashes and no ho_min draws HO(p) = full & ~(AND of
words 0 .. drop_log2 - 1 of p's stream), or the round's common set, with the self bit on either —
the same Philox calls and words as the general draw, written straight-line: one call for
drop_log2 <= 2, calls 0 and 1 as an interleaved pair for 3 and 4, a loop of whole calls past that.
Every result equals the CPU oracle's: per-instance digest, first_fail, term_round, n_checks,
n_decided, the decisions and their rounds, the fetched process records and the batch summary.

Every case first asserts, on the oracle's own output, that the regime it names is reached.
"""
import numpy as np
import pytest

from round_amd import psync

from gpu_support import BEGIN, assert_run_equals_oracle, cmp_instances, cmp_summary, inst_tuple, otr_alg, rec_tuple

pytestmark = pytest.mark.gpu

H = psync.HOSchedule
ALGS = ["otr", "otr2"]


def _cfg(alg, n, rounds, **kw):
    return psync.make_config(alg, n, rounds=rounds, **kw)


def _oracle(oracle_mod, cfg, begin, count, init=None):
    return oracle_mod.run(cfg, begin, count, init=init, per_instance=True, records=True, threads=8)


def _gpu_equals_oracle(alg, n, rounds, begin, count, ora, init=None, **kw):
    """Run [begin, begin + count) on the GPU and compare everything with the oracle's `ora`. A batch
    at gpu_support's BEGIN goes through its assert_run_equals_oracle, which also fetches a sample of
    the ids (the id-list launch of the same kernel) and compares summaries and process records."""
    osum, opi, orec = ora
    with psync.GpuRound(alg, n, rounds=rounds, batch_capacity=count, **kw) as g:
        if init is not None:
            g.load_inputs(begin, count, init)
        if begin == BEGIN:
            sample = [BEGIN + count - 1, BEGIN, BEGIN + count // 2, BEGIN + 9, BEGIN + 8]
            assert_run_equals_oracle(g, count, osum, opi, orec, sample)
            return
        res = g.run(begin, count, per_instance=True)
        dec, dround = g.decisions()
    cmp_instances(res.per_instance, opi)
    assert list(dec) == [r.decision for r in orec]
    assert list(dround) == [r.decision_round for r in orec]
    cmp_summary(res.summary, osum, rounds)


def _unsettled_rounds(orec, n, R, count):
    """Per instance, the rounds the kernel executes with HO sets drawn: a round is settled (not
    drawn) only once every live process has decided, so rounds 0 .. (last first-decision round)
    are drawn, all R of them where some process never decides."""
    out = []
    for i in range(count):
        recs = orec[i * n:(i + 1) * n]
        out.append(max(r.decision_round + 1 if r.decision_round >= 0 else R for r in recs))
    return out


def _ho(oracle_mod, cfg, begin, count):
    """The seeded HO sets [count][R][n] (n <= 64) as the oracle's generator gives them."""
    return oracle_mod.materialize_schedule(cfg, begin, count)[0][:, :, :, 0]


def _common(ho, n):
    """common[i][k]: every process of instance i has the same HO set in round k, up to the self bits."""
    own = np.array([1 << p for p in range(n)], dtype=np.uint64).reshape(1, 1, n)
    one = np.uint64(1)
    return ((ho | own | one) == (ho[:, :, :1] | own | one)).all(axis=2)


# --------------------------------------------------------------------------- 1. drop words x self bit
@pytest.mark.parametrize("self_bit", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("drop_log2", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("name", ALGS)
def test_drop_words_and_self_bit(name, drop_log2, self_bit, oracle_mod):
    """drop_log2 = 0: no draw; 1, 2: one call (one word, both words); 3: two calls, the last word
    unused; 4: two calls in full; 5, 6: the loop of whole calls (an odd and an even word count).
    At n = 64 the self bit of lane 63 is bit 63. The oracle's own HO sets show the loss rate the
    case names (a drop word too many or too few halves or doubles it) and the self bit on every
    set or, without it, missing from some."""
    n, R, count, begin = 64, 20, 400, 1000
    kw = dict(seed=41, value_range=64, schedule=H(drop_log2=drop_log2, good_round=0.25, self_bit=self_bit))
    alg = otr_alg(name)
    cfg = _cfg(alg, n, R, **kw)
    ho = _ho(oracle_mod, cfg, begin, 40)
    own = np.array([1 << p for p in range(n)], dtype=np.uint64).reshape(1, 1, n)
    has_self = (ho & own) != 0
    if self_bit or drop_log2 == 0:
        assert has_self.all()
    else:
        assert not has_self.all()
    bad = ~_common(ho, n)  # rounds that are not good: every other process is dropped with 2^-drop_log2
    if drop_log2 == 0:
        assert not bad.any()
    else:
        others = np.ascontiguousarray((ho & ~own)[bad])  # [rounds][n]: the other processes heard
        heard = np.unpackbits(others.view(np.uint8)).sum() / others.size
        lost = 1.0 - heard / (n - 1)
        assert 0.7 * 2.0 ** -drop_log2 < lost < 1.4 * 2.0 ** -drop_log2, lost
    ora = _oracle(oracle_mod, cfg, begin, count)
    drawn = _unsettled_rounds(ora[2], n, R, count)
    assert min(drawn) >= 1 and ora[0].decided_processes > 0
    if drop_log2 in (1, 2):  # heavy loss: undecided well past the front rounds
        assert max(drawn) >= 5, max(drawn)
    _gpu_equals_oracle(alg, n, R, begin, count, ora, **kw)


@pytest.mark.parametrize("R", [20, 70])
@pytest.mark.parametrize("drop_log2", [5, 6])
@pytest.mark.parametrize("name", ALGS)
def test_loop_of_calls_in_late_rounds(name, drop_log2, R, oracle_mod):
    """The path past the written-out cases in late rounds. At a loss of 1/32 or 1/64 most instances
    decide by round 2, but at n = 3 (quorum: all three heard) a process that misses its quorum in
    the two rounds before the others halt never hears a quorum again and stays undecided: the
    oracle leaves 23 (drop_log2 = 5) and 5 (drop_log2 = 6) of these 2000 instances with such a
    process, and those are drawn in every round through R - 1 — past round 64 at R = 70."""
    n, count, begin = 3, 2000, 1000
    kw = dict(seed=41, value_range=64, schedule=H(drop_log2=drop_log2, good_round=0.0))
    alg = otr_alg(name)
    cfg = _cfg(alg, n, R, **kw)
    ora = _oracle(oracle_mod, cfg, begin, count)
    drawn = _unsettled_rounds(ora[2], n, R, count)
    late = sum(1 for d in drawn if d == R)
    print("instances drawn through round", R - 1, ":", late, "of", count)
    assert late >= 4, late
    _gpu_equals_oracle(alg, n, R, begin, count, ora, **kw)


# --------------------------------------------------------------------------- 2. n and the lanes past it
@pytest.mark.parametrize("self_bit", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("n", [1, 2, 5, 33, 63, 64])
@pytest.mark.parametrize("name", ALGS)
def test_process_counts(name, n, self_bit, oracle_mod):
    """n = 1, 2, 5, 33, 63: lanes past n, `full` without bit 63, the self bit below it; n = 64:
    `full` with bit 63. The default loss (drop_log2 = 3: the interleaved pair)."""
    R, count, begin = 20, 300, 1000
    kw = dict(seed=43, value_range=64, schedule=H(drop_log2=3, good_round=0.25, self_bit=self_bit))
    alg = otr_alg(name)
    cfg = _cfg(alg, n, R, **kw)
    ho = _ho(oracle_mod, cfg, begin, 40)
    assert (ho >> np.uint64(n) == 0).all() if n < 64 else (ho >> np.uint64(63)).any()
    ora = _oracle(oracle_mod, cfg, begin, count)
    assert ora[0].instances == count and min(_unsettled_rounds(ora[2], n, R, count)) >= 1
    _gpu_equals_oracle(alg, n, R, begin, count, ora, **kw)


# --------------------------------------------------------------------------- 3. good rounds
@pytest.mark.parametrize("self_bit", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("good,good_min", [(0.0, None), (0.25, None), (1.0, None), (0.5, 60), (0.5, 20)])
@pytest.mark.parametrize("name", ALGS)
def test_good_rounds(name, good, good_min, self_bit, oracle_mod):
    """No good round, the default rate, every round good, and an explicit good_min above and below
    the default 2n/3 (60: most common sets fall to at most good_min members and become full).
    The self bit goes on a good round's common set as on a drawn one. The oracle's HO sets show
    that good rounds are executed unsettled: round 0 is drawn in every instance."""
    n, R, count, begin = 64, 20, 300, 1000
    kw = dict(seed=44, value_range=64, schedule=H(drop_log2=2, good_round=good, good_min=good_min, self_bit=self_bit))
    alg = otr_alg(name)
    cfg = _cfg(alg, n, R, **kw)
    ora = _oracle(oracle_mod, cfg, begin, count)
    drawn = _unsettled_rounds(ora[2], n, R, count)
    ho = _ho(oracle_mod, cfg, begin, 60)
    common = _common(ho, n)
    unsettled = np.array([[k < drawn[i] for k in range(R)] for i in range(60)])
    good_unsettled = int((common & unsettled).sum())
    print("good rounds executed unsettled:", good_unsettled, "of", int(unsettled.sum()), "unsettled rounds")
    if good == 0.0:
        assert good_unsettled == 0
    elif good == 1.0:
        assert common.all() and good_unsettled == int(unsettled.sum()) > 0
    else:
        assert 0 < good_unsettled < int(unsettled.sum())
    if good_min is not None:
        full = (ho == np.uint64(2 ** 64 - 1)).all(axis=2)
        assert full[common].mean() > 0.5 if good_min == 60 else full[common].mean() < 0.5
    # a common set without some process's own bit is left without it (good_min = 60: the sets are full)
    if not self_bit and good > 0.0 and good_min != 60:
        own = np.array([1 << p for p in range(n)], dtype=np.uint64).reshape(1, 1, n)
        assert ((ho & own) == 0)[common].any()
    _gpu_equals_oracle(alg, n, R, begin, count, ora, **kw)


# --------------------------------------------------------------------------- 4. instance ids, long runs
@pytest.mark.parametrize("R", [1, 20, 70])
@pytest.mark.parametrize("name", ALGS)
def test_high_id_words_and_long_runs(name, R, oracle_mod):
    """The quorum mutant (variant = 1) at n = 5 under heavy loss keeps instances undecided to the
    last round (R = 70: draws past round 64). The batch straddles 2^32: the low id word carries
    and the high word — a wave-uniform Philox input — is 0 on one side and 1 on the other."""
    n, count, begin = 5, 300, 2 ** 32 - 37
    alg = otr_alg(name, variant=1)
    kw = dict(seed=5, value_range=64, schedule=H(drop_log2=1, good_round=0.25))
    cfg = _cfg(alg, n, R, **kw)
    ora = _oracle(oracle_mod, cfg, begin, count)
    drawn = _unsettled_rounds(ora[2], n, R, count)
    live = [i for i in range(count) if drawn[i] == R]
    print("instances drawn through the last round:", len(live))
    assert len(live) >= 20 and min(live) < 37 <= max(live)  # on both sides of the carry
    _gpu_equals_oracle(alg, n, R, begin, count, ora, **kw)


@pytest.mark.parametrize("name", ALGS)
def test_id_list_with_high_words(name, oracle_mod):
    """The fetch path (an explicit id list): shuffled ids with high words 0, 1, 0x12345678 and
    2^32 - 1, next to a batch that starts at a non-zero high word."""
    n, R, count = 64, 20, 40
    begin = (0x12345678 << 32) + 0xFFFFFFF0  # the batch itself carries into the high word
    kw = dict(seed=45, value_range=64)
    assert H().crash_fmax is None and H().ho_min is None  # the default schedule is a plain one
    alg = otr_alg(name)
    cfg = _cfg(alg, n, R, **kw)
    ora = _oracle(oracle_mod, cfg, begin, count)
    ids = [7, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 9, begin + 3, begin + 20, 2 ** 64 - 2, (2 ** 32 - 1) << 32, 2 ** 63 + 5]
    np.random.default_rng(3).shuffle(ids)
    _, fpi, frec = oracle_mod.run(cfg, ids=ids, per_instance=True, records=True, threads=4)
    assert len({inst_tuple(s) for s in fpi}) > 1
    with psync.GpuRound(alg, n, rounds=R, batch_capacity=count, **kw) as g:
        res = g.run(begin, count, per_instance=True)
        dec, dround = g.decisions()
        fsums, frecs = g.fetch(ids)
    cmp_instances(res.per_instance, ora[1])
    cmp_summary(res.summary, ora[0], R)
    assert list(dec) == [r.decision for r in ora[2]] and list(dround) == [r.decision_round for r in ora[2]]
    for j, inst in enumerate(ids):
        assert inst_tuple(fsums[j]) == inst_tuple(fpi[j]), inst
        assert [rec_tuple(r) for r in frecs[j * n:(j + 1) * n]] == [rec_tuple(r) for r in frec[j * n:(j + 1) * n]], inst


# --------------------------------------------------------------------------- 5. the dispatch
@pytest.mark.parametrize("sched", ["plain", "crash", "ho_min", "crash0"])
@pytest.mark.parametrize("name", ALGS)
def test_dispatch_by_schedule(name, sched, oracle_mod):
    """The same seeds under the plain schedule, with crash_fmax = 2 and with ho_min = n // 2 (both
    through the general kernel), and with crash_fmax = 0 (nobody can crash: a plain launch). The
    crash and ho_min schedules change the oracle's results, so a launch sent to the wrong kernel
    cannot pass."""
    n, R, count, begin = 64, 20, 400, 1000
    extra = {"plain": {}, "crash": dict(crash_fmax=2), "ho_min": dict(ho_min=n // 2), "crash0": dict(crash_fmax=0)}[sched]
    # loss 1/2: HO sets of about n / 2 members, so ho_min = n // 2 raises many of them
    kw = dict(seed=46, value_range=64, schedule=H(drop_log2=1, good_round=0.25, **extra))
    base = dict(seed=46, value_range=64, schedule=H(drop_log2=1, good_round=0.25))
    alg = otr_alg(name)
    ora = _oracle(oracle_mod, _cfg(alg, n, R, **kw), begin, count)
    plain = _oracle(oracle_mod, _cfg(alg, n, R, **base), begin, count)
    same = [inst_tuple(a) for a in ora[1]] == [inst_tuple(b) for b in plain[1]]
    assert same == (sched in ("plain", "crash0"))
    _gpu_equals_oracle(alg, n, R, begin, count, ora, **kw)


# --------------------------------------------------------------------------- 6. mmor's inputs
@pytest.mark.parametrize("V", [1, 2, 64, 1000])
@pytest.mark.parametrize("name", ALGS)
def test_value_ranges(name, V, oracle_mod):
    """Seeded initial values: V = 1 all equal, V = 2 and 64 inside a 64-value window (bitmap mode),
    V = 1000 outside one."""
    n, R, count, begin = 64, 20, 300, 1000
    kw = dict(seed=47, value_range=V, schedule=H(drop_log2=2, good_round=0.25))
    alg = otr_alg(name)
    cfg = _cfg(alg, n, R, **kw)
    inits = {oracle_mod.init_value(cfg, begin + i, p) for i in range(20) for p in range(n)}
    assert len(inits) == 1 if V == 1 else (max(inits) - min(inits) >= 64) == (V == 1000)
    ora = _oracle(oracle_mod, cfg, begin, count)
    _gpu_equals_oracle(alg, n, R, begin, count, ora, **kw)


@pytest.mark.parametrize("kind", ["distinct", "pairs", "equal", "wide"])
@pytest.mark.parametrize("name", ALGS)
def test_host_supplied_values(name, kind, oracle_mod):
    """n = 64 with host-supplied values: 64 distinct values of one 64-value window (every holder
    class of mmor's round 0 is walked down to the single holders), 32 values held twice, all
    equal, and 64 distinct values spread past a window."""
    n, R, count, begin = 64, 20, 200, 1000
    rng = np.random.default_rng(11)
    rows = []
    for _ in range(count):
        if kind == "distinct":
            row = 100 + rng.permutation(64)
        elif kind == "pairs":
            row = 100 + rng.permutation(np.repeat(np.arange(32), 2))
        elif kind == "equal":
            row = np.full(64, 7)
        else:
            row = 1 + 1000 * rng.permutation(64)
        rows.append(row.astype(np.int32))
    init = np.stack(rows)
    assert {len(set(r.tolist())) for r in init} == {dict(distinct=64, pairs=32, equal=1, wide=64)[kind]}
    kw = dict(seed=48, value_range=2 ** 20, schedule=H(drop_log2=2, good_round=0.25))
    alg = otr_alg(name)
    ora = _oracle(oracle_mod, _cfg(alg, n, R, **kw), begin, count, init=init)
    assert ora[0].decided_processes > 0
    _gpu_equals_oracle(alg, n, R, begin, count, ora, init=init, **kw)
