"""OTR / OTR2 per-instance setup and finish on the GPU (psg_otr.hip, W = 1): the X0 window
test and its LDS bitmap (X0Set::build_window), check point 0 from the initial state
(otr_check_initial), the summary record packed into one store and the per-wave counter sums
(finish_instance_w1, WaveTally). Exact against the CPU oracle on (digest, first_fail,
term_round, n_checks, n_decided) per instance, on the decisions and on the batch summary.

Every case first asserts, on its inputs and on the oracle's own output, that the regime it
names is reached.
"""
import numpy as np
import pytest

from round_amd import psync

from gpu_support import BEGIN, cmp_instances, cmp_summary, otr_alg

pytestmark = pytest.mark.gpu

H = psync.HOSchedule
NEVER = 0xFF
INT32_MIN = -(2 ** 31)


def _oracle(oracle_mod, cfg, count, init=None):
    return oracle_mod.run(cfg, BEGIN, count, init=init, per_instance=True, records=True, threads=8)


def _gpu_equals_oracle(alg, n, rounds, count, ora, init=None, **kw):
    """Run [BEGIN, BEGIN + count) on the GPU and compare everything with the oracle's `ora`."""
    osum, opi, orec = ora
    with psync.GpuRound(alg, n, rounds=rounds, batch_capacity=count, **kw) as g:
        g.load_inputs(BEGIN, count, init)
        res = g.run(BEGIN, count, per_instance=True)
        dec, dround = g.decisions()
    cmp_instances(res.per_instance, opi)
    assert list(dec) == [r.decision for r in orec]
    assert list(dround) == [r.decision_round for r in orec]
    cmp_summary(res.summary, osum, rounds)


def _cfg(alg, n, rounds, **kw):
    return psync.make_config(alg, n, rounds=rounds, **kw)


# --------------------------------------------------------------------------- 1. seeded shapes
SHAPES = [(a, n) for a in ("otr", "otr2") for n in (1, 2, 3, 5, 63, 64)]


@pytest.mark.parametrize("name,n", SHAPES, ids=[f"{a}-n{n}" for a, n in SHAPES])
def test_seeded_shapes_default_schedule(name, n, oracle_mod):
    """Seeded values in {1..64} (the window hits) under the default schedule (good_round = 0.25):
    small and full waves. Slot 2 (Invariant1) fails at check point 0 wherever two processes start
    with different values, and Termination first holds at several different check points."""
    count, kw = 300, dict(seed=21, value_range=64)
    ora = _oracle(oracle_mod, _cfg(otr_alg(name), n, 20, **kw), count)
    osum, opi, _ = ora
    assert H().good_round == 0.25 and H().drop_log2 == 3
    if n >= 2:
        assert sum(1 for s in opi if s.first_fail[2] == 0) > count // 2
    else:
        assert osum.fail_count[2] == 0  # one process: cnt == n
    if n >= 3:
        assert sum(1 for v in list(osum.term_hist)[:22] if v) >= 2
    _gpu_equals_oracle(otr_alg(name), n, 20, count, ora, **kw)


# --------------------------------------------------------------------------- 2. X0 regimes
def _regime_rows(regime, count, n, rng):
    """Host-supplied initial values [count][n] of one X0 regime."""
    if regime == "window":  # all in [1, 64], both ends present
        a = rng.integers(1, 65, size=(count, n))
        a[:, 0], a[:, -1] = 1, 64
    elif regime == "miss-low":  # contains 0, spread < 64: the bitmap comes through min / max
        a = rng.integers(0, 64, size=(count, n))
        a[:, 0] = 0
    elif regime == "miss-high":  # contains 65, spread < 64
        a = rng.integers(2, 66, size=(count, n))
        a[:, -1] = 65
    elif regime == "hash":  # spread >= 64, negative values and INT32_MIN: the hash table
        a = rng.integers(-1000, 1000, size=(count, n))
        a[:, 0] = INT32_MIN
        a[:, -1] = 2 ** 31 - 1
        a[::2, n // 2] = -1
    elif regime == "equal":  # V = 1: every process starts with the same value
        a = np.repeat(rng.integers(1, 65, size=(count, 1)), n, axis=1)
    else:
        raise ValueError(regime)
    return a.astype(np.int64)


def _in_regime(regime, a):
    lo, hi = a.min(axis=1), a.max(axis=1)
    if regime in ("window", "equal"):
        return bool(((lo >= 1) & (hi <= 64)).all())
    if regime in ("miss-low", "miss-high"):
        return bool((((lo < 1) | (hi > 64)) & (hi - lo < 64)).all())
    return bool((hi - lo >= 64).all() and (lo == INT32_MIN).all() and (a < 0).any())


REGIMES = ["window", "miss-low", "miss-high", "hash", "equal", "mixed"]
X0_CASES = [(a, n, r) for a in ("otr", "otr2") for n in (5, 64) for r in REGIMES]


@pytest.mark.parametrize("name,n,regime", X0_CASES, ids=[f"{a}-n{n}-{r}" for a, n, r in X0_CASES])
def test_host_initial_values_in_each_x0_regime(name, n, regime, oracle_mod):
    """Host-supplied initial values once in each regime of the X0 set, and all regimes interleaved
    instance by instance in one batch (a wave then changes regime between instances and reuses
    its LDS table)."""
    count, kw = 240, dict(seed=22, value_range=64)
    rng = np.random.default_rng(1234 + n)
    if regime == "mixed":
        parts = ["window", "hash", "miss-low", "equal", "miss-high"]
        blocks = {p: _regime_rows(p, count, n, rng) for p in parts}
        init = np.stack([blocks[parts[i % len(parts)]][i] for i in range(count)])
        for j, p in enumerate(parts):
            assert _in_regime(p, init[j::len(parts)])
    else:
        init = _regime_rows(regime, count, n, rng)
        assert _in_regime(regime, init)
    init = init.astype(np.int32)
    ora = _oracle(oracle_mod, _cfg(otr_alg(name), n, 20, **kw), count, init=init.tolist())
    osum, opi, orec = ora
    if regime == "equal":
        # nobody differs: Invariant1 holds at check point 0; OTR fails only Invariant2 there
        assert osum.fail_count[2] == 0
        assert [k for k in range(8) if osum.fail_count[k]] == ([] if name == "otr2" else [3])
    else:
        assert sum(1 for s in opi if s.first_fail[2] == 0) >= count // 2
    assert osum.decided_processes > 0 and osum.fail_count[5] == 0  # decisions are initial values
    _gpu_equals_oracle(otr_alg(name), n, 20, count, ora, init=init, **kw)


def test_seeded_value_range_above_window(oracle_mod):
    """value_range = 1000: the launch does not try the window at all."""
    count, kw = 200, dict(seed=23, value_range=1000)
    ora = _oracle(oracle_mod, _cfg(psync.OTR(), 64, 20, **kw), count)
    vals = [[oracle_mod.init_value(_cfg(psync.OTR(), 64, 20, **kw), BEGIN + i, p) for p in range(64)] for i in (0, 1)]
    assert all(max(v) > 64 for v in vals)
    _gpu_equals_oracle(psync.OTR(), 64, 20, count, ora, **kw)


# --------------------------------------------------------------------------- 3. the good rounds' common set
def _common_set_rounds(oracle_mod, cfg, count):
    ho, _ = oracle_mod.materialize_schedule(cfg, BEGIN, count)
    same = (ho == ho[:, :, :1, :]).all(axis=(2, 3))
    return int(same.sum()), int(same.size)


@pytest.mark.parametrize("name", ["otr", "otr2"])
def test_every_round_good(name, oracle_mod):
    """good_round = 1.0 with drop_log2 = 3: every executed round reads the common HO set, round 0
    included, and every instance terminates at check point 2."""
    count, kw = 300, dict(seed=24, value_range=64, schedule=H(drop_log2=3, good_round=1.0, self_bit=False))
    cfg = _cfg(otr_alg(name), 64, 20, **kw)
    good, total = _common_set_rounds(oracle_mod, cfg, 40)
    assert good == total
    ora = _oracle(oracle_mod, cfg, count)
    assert ora[0].term_hist[2] == count and ora[0].decided_processes == count * 64
    _gpu_equals_oracle(otr_alg(name), 64, 20, count, ora, **kw)


def test_no_round_good(oracle_mod):
    """good_round = 0.0: no round has a common HO set, so the set is never formed or read."""
    count, kw = 300, dict(seed=25, value_range=64, schedule=H(drop_log2=3, good_round=0.0, self_bit=False))
    cfg = _cfg(psync.OTR(), 64, 20, **kw)
    good, _ = _common_set_rounds(oracle_mod, cfg, 40)
    assert good == 0
    ora = _oracle(oracle_mod, cfg, count)
    assert sum(1 for v in list(ora[0].term_hist)[:22] if v) >= 2
    _gpu_equals_oracle(psync.OTR(), 64, 20, count, ora, **kw)


@pytest.mark.parametrize("name", ["otr", "otr2"])
def test_good_rounds_past_the_64_round_block(name, oracle_mod):
    """rounds = 70 with good_round = 0.25 and value_range = 64: the good-round flags and common
    sets are drawn in blocks of 64 rounds, and instances must still execute unsettled rounds in
    the second block. Under the plain seeded schedules every instance has halted long before
    round 64 (the default one terminates by check point 3), so this case uses the quorum mutant
    (variant = 1) at n = 5 under heavy loss, where a fifth of the instances keeps an undecided
    process to the end."""
    n, R, count = 5, 70, 300
    alg = otr_alg(name, variant=1)
    kw = dict(seed=5, value_range=64, schedule=H(drop_log2=1, good_round=0.25))
    cfg = _cfg(alg, n, R, **kw)
    ora = _oracle(oracle_mod, cfg, count)
    osum, opi, orec = ora
    live_undecided = 0
    for i in range(count):
        recs = orec[i * n:(i + 1) * n]
        steps = max(r.halt_round + 1 if r.halt_round >= 0 else R for r in recs)
        live_undecided += steps > 65 and any(r.decision_round < 0 for r in recs)
    assert live_undecided >= 20, live_undecided
    ho, _ = oracle_mod.materialize_schedule(cfg, BEGIN, 40)
    own = np.array([1 << p for p in range(n)], dtype=np.uint64).reshape(1, 1, n, 1)
    one = np.uint64(1)  # rows of a common set differ only in the self bits: compare with those set
    common = ((ho | own | one) == (ho[:, :, :1, :] | own | one)).all(axis=(2, 3))
    assert common[:, 64:].any() and not common[:, 64:].all()
    _gpu_equals_oracle(alg, n, R, count, ora, **kw)


# --------------------------------------------------------------------------- 4. partial queue chunk
@pytest.mark.parametrize("count", [1, 3, 11])
def test_count_below_one_block_and_off_the_queue_chunk(count, oracle_mod):
    """Fewer instances than one block's four waves (1, 3) and a count that is no multiple of the
    queue chunk of 8 (3, 11): idle waves flush empty per-wave sums, a last chunk is cut short."""
    kw = dict(seed=26, value_range=64)
    ora = _oracle(oracle_mod, _cfg(psync.OTR(), 64, 20, **kw), count)
    assert ora[0].decided_processes > 0 and ora[0].fail_count[2] == count
    _gpu_equals_oracle(psync.OTR(), 64, 20, count, ora, **kw)
