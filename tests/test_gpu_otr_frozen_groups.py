"""The frozen tail of the W = 1 OTR / OTR2 kernels in groups of U check points (psg_otr.hip
otr_check_frozen_group): once every process has halted, check points kf + 1 .. R are evaluated U at
a time while U are left and the state is settled (every process decided, one decision, no
witness); the remainder, and the whole tail of an instance whose frozen state is not settled, go
through the one-at-a-time loop. Traced launches, the fused modules and W > 1 keep that loop alone.
Every result equals the CPU oracle's: per-instance digest, first_fail, term_round, n_checks,
n_decided, the decisions and their rounds, the fetched process records and the batch summary.

A frozen check point can never hold a first failure or the Termination round (its state is that of
check point kf), so the check-point numbers a group records are not observable: what these cases
pin is that grouping neither skips the general path where it is needed nor disturbs the first
failures, the counters and the decide results.

Every case first asserts, on the oracle's own output, that the regime it names is reached.
"""
import numpy as np
import pytest

from round_amd import abi, psync

from gpu_support import BEGIN, assert_run_equals_oracle, inst_tuple, otr_alg

pytestmark = pytest.mark.gpu

H = psync.HOSchedule
ALGS = ["otr", "otr2"]
U = 8  # the group size compiled into psg_otr.hip (kFrozenGroup)
AGREEMENT = 4  # slot of first_fail


def _cfg(alg, n, rounds, **kw):
    return psync.make_config(alg, n, rounds=rounds, **kw)


def _oracle(oracle_mod, cfg, count, init=None):
    return oracle_mod.run(cfg, BEGIN, count, init=init, per_instance=True, records=True, threads=8)


def _tails(orec, n, R, count):
    """Per instance, the number of frozen check points: with every process halted, kf = the last
    halt round + 1 and the tail is R - kf; an instance with a process that never halts has none."""
    out = []
    for i in range(count):
        halts = [r.halt_round for r in orec[i * n:(i + 1) * n]]
        out.append(R - (max(halts) + 1) if min(halts) >= 0 else 0)
    return out


def _never_halts(orec, n, count):
    """Instances with a process that never halts."""
    return sum(1 for i in range(count) if min(r.halt_round for r in orec[i * n:(i + 1) * n]) < 0)


def _gpu_equals_oracle(alg, n, rounds, count, ora, init=None, ho=None, **kw):
    """Run [BEGIN, BEGIN + count) on the GPU and compare everything with the oracle's `ora`, through
    gpu_support.assert_run_equals_oracle (which also fetches a sample of the ids). With `ho`, the
    launch reads these HO sets (the explicit-schedule kernel) instead of drawing them."""
    osum, opi, orec = ora
    with psync.GpuRound(alg, n, rounds=rounds, batch_capacity=count, **kw) as g:
        if init is not None:
            g.load_inputs(BEGIN, count, init)
        if ho is not None:
            g.load_schedule(BEGIN, count, ho)
        sample = sorted({BEGIN + count - 1, BEGIN, BEGIN + count // 2, BEGIN + min(9, count - 1), BEGIN + min(8, count - 1)})
        assert_run_equals_oracle(g, count, osum, opi, orec, sample)


# --------------------------------------------------------------------------- 1. tail lengths
TAIL_ROUNDS = list(range(4, 2 * U + 6))  # (R = 20, the headline shape, among them)
_TAIL_ORACLE = {}


def _tail_oracle(oracle_mod, name, R):
    """The oracle's run of the default schedule at n = 64 with R rounds (once per session)."""
    if (name, R) not in _TAIL_ORACLE:
        kw = dict(seed=51, value_range=64)
        ora = _oracle(oracle_mod, _cfg(otr_alg(name), 64, R, **kw), 300)
        _TAIL_ORACLE[(name, R)] = (kw, ora, _tails(ora[2], 64, R, 300))
    return _TAIL_ORACLE[(name, R)]


@pytest.mark.parametrize("R", TAIL_ROUNDS)
@pytest.mark.parametrize("name", ALGS)
def test_tail_lengths(name, R, oracle_mod):
    """n = 64 under the default schedule halts every process by round 3 or 4, so R = 4 .. 2U + 5
    gives every tail length 0 .. 2U + 1 between them: no group, one and two groups, a remainder of
    every size 0 .. U - 1 after one group; R = 20, the headline shape, is one of them."""
    seen = set()
    for r in TAIL_ROUNDS:
        seen |= set(_tail_oracle(oracle_mod, name, r)[2])
    assert seen >= set(range(2 * U + 2)), sorted(seen)
    kw, ora, tails = _tail_oracle(oracle_mod, name, R)
    print("R", R, "tails", sorted(set(tails)))
    assert len(set(tails)) >= 2
    _gpu_equals_oracle(otr_alg(name), 64, R, 300, ora, **kw)


@pytest.mark.parametrize("R", [20, 70])
@pytest.mark.parametrize("name", ALGS)
def test_no_tail_because_a_process_never_halts(name, R, oracle_mod):
    """n = 3 without good rounds at a loss of 1/32: a process that misses its quorum (all three)
    before the others halt never decides and never halts, so those instances have no frozen tail
    at all, next to instances with a tail of more than two groups."""
    n, count = 3, 2000
    kw = dict(seed=41, value_range=64, schedule=H(drop_log2=5, good_round=0.0))
    alg = otr_alg(name)
    ora = _oracle(oracle_mod, _cfg(alg, n, R, **kw), count)
    tails = _tails(ora[2], n, R, count)
    never = _never_halts(ora[2], n, count)
    print("instances with a process that never halts:", never, "of", count)
    assert never >= 4 and tails.count(0) >= never
    assert sum(1 for t in tails if t > 2 * U) >= count // 2
    _gpu_equals_oracle(alg, n, R, count, ora, **kw)


@pytest.mark.parametrize("name", ALGS)
def test_groups_at_check_points_above_64(name, oracle_mod):
    """R = 70 at n = 64: every instance has a tail of 65 or more check points, so groups run at
    check-point numbers above 64."""
    n, R, count = 64, 70, 300
    kw = dict(seed=51, value_range=64)
    alg = otr_alg(name)
    ora = _oracle(oracle_mod, _cfg(alg, n, R, **kw), count)
    tails = _tails(ora[2], n, R, count)
    assert min(tails) >= 65 and len({t % U for t in tails}) >= 2, sorted(set(tails))
    _gpu_equals_oracle(alg, n, R, count, ora, **kw)


# --------------------------------------------------------------------------- 2. lanes past n
@pytest.mark.parametrize("n", [1, 2, 5, 63, 64])
@pytest.mark.parametrize("name", ALGS)
def test_lanes_past_n(name, n, oracle_mod):
    """n = 1, 2, 5, 63: the lanes past n carry decided = 0 and must stay out of the group's witness
    and count ballots (an unmasked witness ballot would refuse every group, an unmasked count
    would not change a result the tests can see, so the oracle parity of the whole run is the
    check); n = 64: no such lane."""
    R, count = 20, 300
    kw = dict(seed=43, value_range=64)
    alg = otr_alg(name)
    ora = _oracle(oracle_mod, _cfg(alg, n, R, **kw), count)
    tails = _tails(ora[2], n, R, count)
    assert sum(1 for t in tails if t >= 2 * U) >= count // 2, sorted(set(tails))
    assert ora[0].decided_processes > 0
    _gpu_equals_oracle(alg, n, R, count, ora, **kw)


# --------------------------------------------------------------------------- 3. frozen, not settled
@pytest.mark.parametrize("name", ALGS)
def test_frozen_with_two_decisions(name, oracle_mod):
    """The quorum mutant (variant = 1: n / 2 instead of 2n / 3) at n = 3 under a loss of 1/2 lets
    two processes decide different values. In at least 10 instances the oracle shows an Agreement
    first failure with every process halted at least U rounds before R: a frozen tail of a group
    or more whose state is not settled, so the group must refuse and every check point of the tail
    go through the general path."""
    n, R, count = 3, 20, 600
    alg = otr_alg(name, variant=1)
    kw = dict(seed=9, value_range=64, schedule=H(drop_log2=1, good_round=0.25))
    ora = _oracle(oracle_mod, _cfg(alg, n, R, **kw), count)
    tails = _tails(ora[2], n, R, count)
    split = [i for i in range(count) if tails[i] >= U and ora[1][i].first_fail[AGREEMENT] != abi.PSG_NEVER]
    print("frozen and split instances:", len(split), "tails", sorted({tails[i] for i in split}))
    assert len(split) >= 10
    for i in split:  # two decisions in the final state
        assert len({r.decision for r in ora[2][i * n:(i + 1) * n] if r.decision_round >= 0}) >= 2
    assert sum(1 for i in range(count) if tails[i] >= U and i not in set(split)) >= 10  # and settled ones
    _gpu_equals_oracle(alg, n, R, count, ora, **kw)


@pytest.mark.parametrize("name", ALGS)
def test_frozen_with_values_past_the_window(name, oracle_mod):
    """Host-supplied rows of 64 distinct values spread over 63000 (the `wide` rows of
    test_gpu_otr_plain_draw.py, each row shifted by its index so that the decided value — the
    row's smallest under this loss — differs from instance to instance): the X0 set is a hash
    table, not a 64-value window, and the memoized "maybe not initial" bit of a value stays set in
    the frozen state when the value sits outside its two home slots. Where the table put a value is
    not the oracle's to see; what it shows is the hash-table regime (a spread past the window), a
    tail of a group or more in most instances and 150 or more different decided values, each with
    its own place in the table. A group must refuse where the bit is set, and the general path
    resolve the probe exactly."""
    n, R, count = 64, 20, 200
    rng = np.random.default_rng(11)
    init = np.stack([(1 + i + 1000 * rng.permutation(64)).astype(np.int32) for i in range(count)])
    assert all(int(r.max()) - int(r.min()) >= 64 and len(set(r.tolist())) == 64 for r in init)
    kw = dict(seed=48, value_range=2 ** 20, schedule=H(drop_log2=2, good_round=0.25))
    alg = otr_alg(name)
    ora = _oracle(oracle_mod, _cfg(alg, n, R, **kw), count, init=init)
    tails = _tails(ora[2], n, R, count)
    assert sum(1 for t in tails if t >= U) >= count // 2, sorted(set(tails))
    decided = {r.decision for r in ora[2] if r.decision_round >= 0}
    print("decided values:", len(decided))
    assert len(decided) >= 150
    _gpu_equals_oracle(alg, n, R, count, ora, init=init, **kw)


# --------------------------------------------------------------------------- 4. the three launch forms
@pytest.mark.parametrize("form", ["plain", "crash", "explicit"])
@pytest.mark.parametrize("name", ALGS)
def test_launch_forms(name, form, oracle_mod):
    """The same seeds through each kernel that groups its frozen tail: the plain-schedule kernel,
    the general seeded kernel (crash_fmax = 2) and the explicit-schedule kernel, fed the oracle's
    materialized HO sets and initial values of the plain schedule (so its results are the plain
    run's)."""
    n, R, count = 64, 20, 300
    alg = otr_alg(name)
    base = dict(seed=46, value_range=64, schedule=H(drop_log2=2, good_round=0.25))
    kw = dict(base, schedule=H(drop_log2=2, good_round=0.25, crash_fmax=2)) if form == "crash" else base
    cfg = _cfg(alg, n, R, **kw)
    ora = _oracle(oracle_mod, cfg, count)
    tails = _tails(ora[2], n, R, count)
    print(form, "tails", sorted(set(tails)))
    assert sum(1 for t in tails if t >= 2 * U) >= count // 4, sorted(set(tails))
    if form == "crash":
        plain = _oracle(oracle_mod, _cfg(alg, n, R, **base), count)
        assert [inst_tuple(a) for a in ora[1]] != [inst_tuple(b) for b in plain[1]]
    init = ho = None
    if form == "explicit":
        ho = oracle_mod.materialize_schedule(cfg, BEGIN, count)[0]
        init = np.array([[oracle_mod.init_value(cfg, BEGIN + i, p) for p in range(n)] for i in range(count)], np.int32)
        again = _oracle(oracle_mod, cfg, count, init=init)
        assert [inst_tuple(a) for a in again[1]] == [inst_tuple(b) for b in ora[1]]
    _gpu_equals_oracle(alg, n, R, count, ora, init=init, ho=ho, **kw)
