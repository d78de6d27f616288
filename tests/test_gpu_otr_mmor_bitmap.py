"""mmor of the seeded, trace-free W = 1 OTR / OTR2 kernels in bitmap mode (psg_otr.hip
otr_mmor_bitmap), and the order in which the one-instance-ahead load of the initial values is used.

When every initial value of an instance lies in a window [lo, lo + 64), a value is named by its slot
in the window, the running best is one 32-bit key (count << 6 | 63 - slot), round 0 walks the bits
of the value bitmap — by holder classes (>= 3, 2, 1 holders) when there are more than 8 values —
and the later rounds walk the alive lanes' values with the same key. Instances whose values spread
over 64 or more keep the 64-bit-key loop over a hash table.

Every result equals the CPU oracle's: per-instance digest, first_fail, term_round, n_checks,
n_decided, the decisions and their rounds, the fetched process records (the id-list launch) and the
batch summary. Every case first asserts on the CPU, from its inputs or from the oracle's own output,
that the regime it names is reached.
"""
import numpy as np
import pytest

from round_amd import psync

from gpu_support import BEGIN, assert_run_equals_oracle, otr_alg

pytestmark = pytest.mark.gpu

H = psync.HOSchedule
ALGS = ["otr", "otr2"]
I32_MAX, I32_MIN = 2 ** 31 - 1, -(2 ** 31)
LOSSLESS = H(drop_log2=0, good_round=0.0)  # every mailbox holds all n values: every process updates


def _oracle(oracle_mod, cfg, count, init=None):
    return oracle_mod.run(cfg, BEGIN, count, init=init, per_instance=True, records=True, threads=8)


def _sample(count):
    return sorted({BEGIN, BEGIN + count - 1, BEGIN + count // 2, BEGIN + min(7, count - 1), BEGIN + min(8, count - 1)})


def _run(oracle_mod, alg, n, count, init=None, load=False, rounds=20, **kw):
    """One oracle run and one GPU run of [BEGIN, BEGIN + count), compared; returns the oracle's."""
    ora = _oracle(oracle_mod, psync.make_config(alg, n, rounds=rounds, **kw), count, init=init)
    with psync.GpuRound(alg, n, rounds=rounds, batch_capacity=count, **kw) as g:
        if init is not None:
            g.load_inputs(BEGIN, count, init)
        elif load:
            g.load_inputs(BEGIN, count)
        assert_run_equals_oracle(g, count, *ora, _sample(count))
    return ora


def _mode(row, V):
    """The X0 set of a row of initial values at value range V: 'window' (the fixed window [1, 65)),
    'bitmap' (spread below 64 at another lo) or 'hash'."""
    lo, hi = int(row.min()), int(row.max())
    if V <= 64 and lo >= 1 and hi <= 64:
        return "window"
    return "bitmap" if hi - lo < 64 else "hash"


def _classes(row):
    """(values held by >= 3 processes, by exactly 2, by exactly 1) of a row."""
    _, c = np.unique(row, return_counts=True)
    return int((c >= 3).sum()), int((c == 2).sum()), int((c == 1).sum())


def _seeded_values(oracle_mod, cfg, count, n):
    return np.array([[oracle_mod.init_value(cfg, BEGIN + i, p) for p in range(n)] for i in range(count)], np.int64)


def _later_mmor(orec):
    """Processes that decided in a round after round 0: mmor ran in a later round."""
    return sum(1 for r in orec if r.decision_round >= 1)


# --------------------------------------------------------------------------- 1. seeded values: n x V
@pytest.mark.parametrize("n", [1, 2, 3, 5, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("name", ALGS)
def test_seeded_n_by_value_range(name, n, oracle_mod):
    """Seeded values {1..V}: V = 1, 2, 8 never stage the holder classes (at most 8 values), V = 9
    and 64 do from n = 31 on (asserted on the seeded values themselves: some instance has more than
    8 distinct ones, and at V = 64 some instance an odd and some an even number of them)."""
    count = 300
    alg = otr_alg(name)
    for V in (1, 2, 8, 9, 64):
        kw = dict(seed=61 + V, value_range=V)
        cfg = psync.make_config(alg, n, rounds=20, **kw)
        vals = _seeded_values(oracle_mod, cfg, 60, n)
        assert vals.min() >= 1 and vals.max() <= V
        distinct = [len(set(r.tolist())) for r in vals]
        if V <= 8 or n <= 8:
            assert max(distinct) <= 8
        elif n >= 31:
            assert max(distinct) > 8, sorted(set(distinct))
            assert V == 9 or len({d % 2 for d in distinct}) == 2, sorted(set(distinct))
        ora = _run(oracle_mod, alg, n, count, **kw)
        assert ora[0].decided_processes > 0


# --------------------------------------------------------------------------- 2. schedules
@pytest.mark.parametrize("drop", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ALGS)
def test_loss_and_good_rounds(name, drop, oracle_mod):
    """A loss of 2^-drop with no, some and only good rounds at n = 64 and n = 33, V = 64 (round 0
    stages the classes; under loss the lanes' mailboxes differ, so the cut-off between classes falls
    differently from instance to instance). Without good rounds at a high loss processes decide in
    later rounds or never: the lane walk of rounds k > 0 runs (asserted on the oracle's records)."""
    alg = otr_alg(name)
    later = 0
    for n in (64, 33):
        for good in (0.0, 0.25, 1.0):
            ora = _run(oracle_mod, alg, n, 300, seed=70 + drop, value_range=64, schedule=H(drop_log2=drop, good_round=good))
            later += _later_mmor(ora[2])
    assert later > 0


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", ALGS)
def test_crash_schedule(name, variant, oracle_mod):
    """A schedule with crashes goes to the general seeded kernel (not the plain-schedule one), with
    the standard quorum and with the n / 2 quorum mutant; a crashed sender's value is still a value
    of round 0's bitmap and counts in no mailbox. The crashes change the results (asserted against
    the oracle's run without them)."""
    alg = otr_alg(name, variant=variant)
    for n, V in ((64, 64), (33, 9), (5, 64)):
        base = dict(seed=81, value_range=V)
        sched = dict(drop_log2=2, good_round=0.25)
        ora = _run(oracle_mod, alg, n, 400, schedule=H(crash_fmax=max(1, n // 8), **sched), **base)
        plain = _oracle(oracle_mod, psync.make_config(alg, n, rounds=20, schedule=H(**sched), **base), 400)
        assert [s.digest for s in ora[1]] != [s.digest for s in plain[1]]


@pytest.mark.parametrize("n", [2, 3, 32, 64])
@pytest.mark.parametrize("name", ALGS)
def test_half_quorum_mutant(name, n, oracle_mod):
    """variant = 1 (n / 2 in place of 2n / 3) under a loss of 1/2: more lanes update on smaller
    mailboxes, and processes decide different values (asserted: some instance fails Agreement)."""
    alg = otr_alg(name, variant=1)
    ora = _run(oracle_mod, alg, n, 600, seed=9, value_range=64, schedule=H(drop_log2=1, good_round=0.25))
    if n == 3:
        assert ora[0].fail_count[4] > 0  # Agreement


# --------------------------------------------------------------------------- 3. host-supplied values
def _rows(kind, rng, count, n):
    """Rows of host-supplied values of one kind (value range 64)."""
    if kind == "window":
        return rng.integers(1, 65, (count, n)).astype(np.int32)
    if kind == "equal":
        return np.repeat(rng.integers(-1000, 1000, (count, 1)), n, axis=1).astype(np.int32)
    if kind == "hash":  # a spread of 64 or more: 1000 apart, the row's smallest moves with the row
        return np.stack([(1 + i + 1000 * rng.integers(0, 40, n)) for i in range(count)]).astype(np.int32)
    if kind == "hash64":  # a spread of exactly 64: the first that does not fit the window
        r = rng.integers(0, 65, (count, n))
        r[:, 0], r[:, n - 1] = 0, 64
        return (r + 7).astype(np.int32)
    lo = {"lo100": 100, "neg": -50, "zero": 0, "top": I32_MAX - 63, "bottom": I32_MIN, "spread63": -31}[kind]
    r = rng.integers(0, 64, (count, n)).astype(np.int64)
    if n > 1:
        r[:, 0], r[:, n - 1] = 0, 63  # the whole window: lo and lo + 63 are values
    return (r + lo).astype(np.int32)


HOST_KINDS = ["window", "lo100", "neg", "zero", "top", "bottom", "spread63", "equal", "hash", "hash64"]
EXPECT = {"window": "window", "equal": None, "hash": "hash", "hash64": "hash"}


@pytest.mark.parametrize("kind", HOST_KINDS + ["mixed"])
@pytest.mark.parametrize("name", ALGS)
def test_host_supplied_values(name, kind, oracle_mod):
    """Host-supplied rows at n = 64 and n = 33 under a loss of 1/4: a window hit; spreads below 64
    at lo = 100, negative lo, lo = 0, lo + 63 = INT32_MAX and lo = INT32_MIN (bitmap mode away from
    the fixed window, with lo and lo + 63 both present); all values equal; spreads of 64 or more
    (hash mode, the 64-bit-key loop); and all of these interleaved row by row in one batch."""
    count, V = 300, 64
    alg = otr_alg(name)
    rng = np.random.default_rng(5)
    for n in (64, 33):
        if kind == "mixed":
            per = [_rows(k, rng, count, n) for k in HOST_KINDS]
            init = np.stack([per[i % len(per)][i] for i in range(count)])
            modes = {_mode(r, V) for r in init}
            assert modes == {"window", "bitmap", "hash"}
        else:
            init = _rows(kind, rng, count, n)
            modes = {_mode(r, V) for r in init}
            want = EXPECT.get(kind, "bitmap")
            assert want is None or modes == {want}, modes
            if kind == "equal":
                assert all(len(set(r.tolist())) == 1 for r in init) and "hash" not in modes
            if kind in ("top", "bottom"):
                assert int(init.max()) == I32_MAX if kind == "top" else int(init.min()) == I32_MIN
        ora = _run(oracle_mod, alg, n, count, init=init, seed=48, value_range=V, schedule=H(drop_log2=2, good_round=0.25))
        assert ora[0].decided_processes > 0


# --------------------------------------------------------------------------- 4. class cut-offs
def _class_row(rng, n, a, b, s, lo):
    """A row of n values in [lo, lo + 64) with a values held by >= 3 processes, b by two and s by
    one, in random lane order."""
    assert 3 * a + 2 * b + s <= n and a + b + s <= 64 and (a > 0 or 2 * b + s == n)
    vals = lo + rng.permutation(64)[: a + b + s]
    held = [3] * a + [2] * b + [1] * s
    for _ in range(n - sum(held)):
        held[int(rng.integers(0, a))] += 1
    row = np.repeat(vals, held)
    return row[rng.permutation(n)].astype(np.int32)


# (a, b, s): odd and even numbers of values in each class, empty classes among them
CLASS_SHAPES = {
    "first": [(1, 4, 5), (2, 3, 6), (3, 0, 9), (4, 5, 0), (7, 2, 1)],       # some value held by >= 3
    "second": [(0, 1, 62), (0, 2, 60), (0, 7, 50), (0, 32, 0), (0, 31, 2)],  # pairs at the most
    "third": [(0, 0, 64)],                                                   # 64 distinct values
}


@pytest.mark.parametrize("stop", ["first", "second", "third"])
@pytest.mark.parametrize("name", ALGS)
def test_round0_class_cutoffs(name, stop, oracle_mod):
    """Rows built so that, with lossless mailboxes (every process receives all n values, so a
    value's count is its holders), round 0 stops after the first class (a value held by >= 3:
    every lane's best count is then >= 3), after the second (no such value, pairs: every best is
    2) or runs all three (64 distinct values), with odd and even numbers of values per class; the
    same rows under a loss of 1/2, where a lane may miss a class's values and the walk goes on.
    Lossless, every process takes the most-held value, the smaller on a tie (asserted on the
    oracle's records against the rows)."""
    n, per = 64, 60
    alg = otr_alg(name)
    rng = np.random.default_rng(23)
    shapes = CLASS_SHAPES[stop]
    for lo in (1, -40):
        init = np.stack([_class_row(rng, n, *shapes[i % len(shapes)], lo) for i in range(per * len(shapes))])
        for i, row in enumerate(init):
            a, b, s = _classes(row)
            assert (a, b, s) == shapes[i % len(shapes)] and a + b + s > 8
            assert {"first": a > 0, "second": a == 0 and b > 0, "third": a == 0 and b == 0}[stop]
        assert _mode(init[0], 64) == ("window" if lo == 1 else "bitmap")
        count = len(init)
        ora = _run(oracle_mod, alg, n, count, init=init, seed=3, value_range=64, schedule=LOSSLESS)
        for i, row in enumerate(init):
            v, c = np.unique(row, return_counts=True)
            winner = int(v[c == c.max()].min())
            assert all(r.final_x == winner for r in ora[2][i * n:(i + 1) * n]), i
        _run(oracle_mod, alg, n, count, init=init, seed=3, value_range=64, schedule=H(drop_log2=1, good_round=0.0))


# --------------------------------------------------------------------------- 5. ties
@pytest.mark.parametrize("n", [2, 32, 64])
@pytest.mark.parametrize("name", ALGS)
def test_ties_go_to_the_smaller_value(name, n, oracle_mod):
    """Two values held by n / 2 processes each (no staging), and from n = 32 on four values held by
    n / 4 each in a third of the rows; the larger values sit on the lower lanes in half of the
    rows, and half of the rows are shuffled. Lossless, the counts are equal in every mailbox and
    the oracle's records show every process on the smallest value; the same rows under loss."""
    alg = otr_alg(name)
    rng = np.random.default_rng(31)
    rows = []
    for i in range(120):
        lo = int(rng.integers(-60, 60))
        k = 4 if (n >= 32 and i % 3 == 2) else 2
        vals = lo + np.sort(rng.permutation(64)[:k])
        row = np.repeat(vals if i % 2 else vals[::-1], n // k)
        rows.append(row if i % 4 < 2 else row[rng.permutation(n)])
    init = np.stack(rows).astype(np.int32)
    for row in init:
        _, c = np.unique(row, return_counts=True)
        assert len(set(c.tolist())) == 1 and len(c) in (2, 4)
    ora = _run(oracle_mod, alg, n, len(init), init=init, seed=4, value_range=2 ** 20, schedule=LOSSLESS)
    for i, row in enumerate(init):
        assert all(r.final_x == int(row.min()) for r in ora[2][i * n:(i + 1) * n]), i
    _run(oracle_mod, alg, n, len(init), init=init, seed=4, value_range=2 ** 20, schedule=H(drop_log2=2, good_round=0.25))


# --------------------------------------------------------------------------- 6. the prefetch
@pytest.mark.parametrize("inputs", ["seeded", "staged", "host"])
@pytest.mark.parametrize("name", ALGS)
def test_prefetch_order_and_counts(name, inputs, oracle_mod):
    """Batches of 1, 7, 8, 9, 3 (below one block) and 200 instances as consecutive runs on one
    context: without staged values (no load to prefetch), with the seeded values staged in device
    memory (load_inputs) and with host-supplied rows that differ from instance to instance, so a
    value consumed an instance early or late changes the results. After every run the same
    instances are fetched through an id list of 1, 7, 8 and 9 ids in descending order (the launch
    with an id list, whose rows are found by id)."""
    n, V = 64, 64
    alg = otr_alg(name)
    kw = dict(seed=12, value_range=V, schedule=H(drop_log2=2, good_round=0.25))
    cfg = psync.make_config(alg, n, rounds=20, **kw)
    rng = np.random.default_rng(17)
    with psync.GpuRound(alg, n, rounds=20, batch_capacity=200, **kw) as g:
        for count in (1, 7, 8, 9, 3, 200, 8):
            init = None
            if inputs == "host":
                init = (rng.integers(0, 64, (count, n)) + rng.integers(-500, 500, (count, 1))).astype(np.int32)
                assert count == 1 or len({tuple(r.tolist()) for r in init}) == count
                g.load_inputs(BEGIN, count, init)
            elif inputs == "staged":
                g.load_inputs(BEGIN, count)
            ora = _oracle(oracle_mod, cfg, count, init=init)
            for k in (1, 7, 8, 9):
                ids = [BEGIN + j for j in range(min(k, count))][::-1]
                assert_run_equals_oracle(g, count, *ora, ids)
