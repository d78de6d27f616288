"""LatticeAgreement pinned to the reference: a literal restatement and hand KATs.

`py_lattice` restates `LatticeAgreementProcess` (example/LatticeAgreement.scala:39-65) in pure
Python under explicit HO sets, with send / mailbox / update as the source writes them on Python
sets, and evaluates the six check slots of DESIGN.md §2 after every round by direct set
arithmetic. It is the reference side of the GPU tests (tests/test_gpu_lattice.py): the oracle
library has no LatticeAgreement and the reference's spec is `TrivialSpec //TODO` (:74).

Sets cross the C ABI as int32 bit masks (bit e = element e of {0..30}); inputs are taken
`& 0x7FFFFFFF`. The KATs below were worked from the Scala source line by line.
"""
import numpy as np
import pytest

from round_amd import abi, psync

NEVER = abi.PSG_NEVER
NONE32 = -(1 << 31)
LATTICE = 11
SLOTS = ["Safety", "Invariant0", "Comparability", "DownwardValidity", "UpwardValidity", "Irrevocability"]
VIOLATION_SLOTS = [0, 2, 3, 4, 5]


def to_set(mask):
    mask = int(mask) & 0x7FFFFFFF
    return frozenset(e for e in range(31) if (mask >> e) & 1)


def to_mask(s):
    return sum(1 << e for e in s)


class LatticeRun:
    """Result of py_lattice: per-process records, the slots' verdicts, the states of every check point."""

    def __init__(self, n, R):
        self.n, self.R = n, R
        self.rec = []         # per p: (decision, decision_round, halt_round, final_x) as the C ABI reports them
        self.states = []      # per check point: list of (proposed mask, decided, decision mask or NONE32, hosize)
        self.first_fail = [NEVER] * 6
        self.term_round = NEVER
        self.n_decided = 0


def py_lattice(n, init, ho, R, variant=0):
    """LatticeAgreementProcess under explicit HO sets ho[k][p] (bit q: p hears q in round k), R
    rounds. variant 1: the threshold is n/4 instead of n/2 (:54)."""
    init = [to_set(v) for v in init]
    J = frozenset().union(*init)
    proposed = list(init)                    # init(io), :39-43
    active = [True] * n
    decision = [None] * n
    halted = [False] * n
    cb = [None] * n                          # (value passed to callback.decide, round), :55
    out = LatticeRun(n, R)
    thr = n // 4 if variant == 1 else n // 2

    def check(c, old, hosize):
        defined = [d for d in decision if d is not None]
        comparable = all(a <= b or b <= a for a in defined for b in defined)
        down = all(decision[p] is None or init[p] <= decision[p] for p in range(n))
        up = all(d <= J for d in defined)
        irrev = old is None or all(old[p] is None or (decision[p] is not None and decision[p] == old[p])
                                   for p in range(n))
        inv = all(init[p] <= proposed[p] <= J and (decision[p] is None or decision[p] == proposed[p])
                  for p in range(n)) and comparable
        for s, ok in enumerate((inv, inv, comparable, down, up, irrev)):
            if not ok and out.first_fail[s] == NEVER:
                out.first_fail[s] = c
        if out.term_round == NEVER and len(defined) == n:
            out.term_round = c
        out.states.append([(to_mask(proposed[p]), int(decision[p] is not None),
                            NONE32 if decision[p] is None else to_mask(decision[p]), hosize[p]) for p in range(n)])

    check(0, None, [n] * n)
    for k in range(R):
        old = list(decision)
        senders = [q for q in range(n) if not halted[q]]
        sent = {q: proposed[q] for q in senders}                                  # :48-50 broadcast(proposed)
        new_proposed = list(proposed)
        hosize = [n] * n
        exits = []
        for p in senders:
            mailbox = {q: v for q, v in sent.items() if (ho[k][p] >> q) & 1}
            hosize[p] = len(mailbox)
            if active[p]:                                                         # :53
                if sum(1 for v in mailbox.values() if v == proposed[p]) > thr:    # :54
                    cb[p] = (proposed[p], k)                                      # :55
                    decision[p] = proposed[p]                                     # :56
                    active[p] = False                                             # :57
                    exits.append(p)                                               # :58
                else:
                    x = proposed[p]
                    for v in mailbox.values():                                    # :60 join(proposed, mailbox values)
                        x = x | v
                    new_proposed[p] = x
        proposed = new_proposed
        for p in exits:
            halted[p] = True
        check(k + 1, old, hosize)
    for p in range(n):
        if cb[p] is None:
            out.rec.append((0, -1, -1, to_mask(proposed[p])))
        else:
            out.rec.append((to_mask(cb[p][0]), cb[p][1], cb[p][1], to_mask(proposed[p])))
    out.n_decided = sum(1 for r in out.rec if r[1] >= 0)
    return out


def ho_ints(ho_arr):
    """uint64 [R][n][W] -> Python ints [R][n]."""
    R, n, W = ho_arr.shape
    return [[sum(int(ho_arr[k, p, w]) << (64 * w) for w in range(W)) for p in range(n)] for k in range(R)]


def full_ho(n, R):
    return [[(1 << n) - 1] * n for _ in range(R)]


# ------------------------------------------------------------------------------------ 1. hand KATs
def kat_three_singletons():
    """Round 0: nobody has two equal values (cnt = 1, not > 1), everyone joins to {0,1,2} = 7.
    Round 1: cnt = 3 > 1: all decide 7."""
    return 3, (1, 2, 4), full_ho(3, 2), 2


def kat_two_comparable_decisions():
    """Round 0: p0, p1 hear {0,1,2}, all {0}: cnt = 3 > 2, decide {0}. p2 hears {2,3}: values
    {0}, {0,1}, cnt = 1: joins to {0,1}. p3, p4 hear {3,4}: cnt = 2, not > 2: stay {0,1}.
    Round 1: p2..p4 hear {2,3,4}, all {0,1}: cnt = 3 > 2, decide {0,1}."""
    ho = [[0b00111, 0b00111, 0b01100, 0b11000, 0b11000], [0b11100] * 5]
    return 5, (1, 1, 1, 3, 3), ho, 2


def kat_mutant_n5():
    """variant 1 (cnt > n/4 = 1): p0, p1 hear each other: cnt = 2, decide {0}; p2, p3 likewise
    decide {1}; p4 hears itself: cnt = 1, stays. {0} and {1} are incomparable."""
    return 5, (1, 1, 2, 2, 2), [[0b00011, 0b00011, 0b01100, 0b01100, 0b10000]], 1


def kat_single_self():
    return 1, (5,), [[1]], 1      # cnt = 1 > 0: decides its input in round 0


def kat_single_deaf():
    return 1, (5,), [[0], [0]], 2  # empty mailbox: cnt = 0, join of nothing: never decides


def kat_bottom_and_high_bits():
    """p0..p2 hold bottom (0) and hear each other: cnt = 3 > 2, they decide the empty set (decision
    0 with decision_round 0). p3, p4 hold -1 = every bit: bit 31 is dropped on input (0x7FFFFFFF);
    they hear only themselves (cnt = 1) in round 0 and p0..p4 minus the halted in round 1 (cnt = 2)."""
    ho = [[0b00111, 0b00111, 0b00111, 0b01000, 0b10000], [0b11111] * 5]
    return 5, (0, 0, 0, -1, -1), ho, 2


H = 0x7FFFFFFF
# (kat, variant, per process (decision, decision_round, halt_round, final_x), first_fail, term_round, n_decided)
KATS = [
    (kat_three_singletons, 0, [(7, 1, 1, 7)] * 3, [NEVER] * 6, 2, 3),
    (kat_two_comparable_decisions, 0, [(1, 0, 0, 1)] * 2 + [(3, 1, 1, 3)] * 3, [NEVER] * 6, 2, 5),
    (kat_mutant_n5, 1, [(1, 0, 0, 1)] * 2 + [(2, 0, 0, 2)] * 2 + [(0, -1, -1, 2)], [1, 1, 1, NEVER, NEVER, NEVER], NEVER, 4),
    (kat_mutant_n5, 0, [(0, -1, -1, 1)] * 2 + [(0, -1, -1, 2)] * 3, [NEVER] * 6, NEVER, 0),
    (kat_single_self, 0, [(5, 0, 0, 5)], [NEVER] * 6, 1, 1),
    (kat_single_deaf, 0, [(0, -1, -1, 5)], [NEVER] * 6, NEVER, 0),
    (kat_bottom_and_high_bits, 0, [(0, 0, 0, 0)] * 3 + [(0, -1, -1, H)] * 2, [NEVER] * 6, NEVER, 3),
]
KAT_IDS = [f"{k[0].__name__}-v{k[1]}" for k in KATS]


@pytest.mark.parametrize("kat,variant,recs,ff,term,nd", KATS, ids=KAT_IDS)
def test_hand_kats(kat, variant, recs, ff, term, nd):
    n, init, ho, R = kat()
    run = py_lattice(n, init, ho, R, variant)
    assert run.rec == recs
    assert (run.first_fail, run.term_round, run.n_decided) == (ff, term, nd)


def test_kat_states_round_by_round():
    """The three-singleton KAT's states: everyone holds 7 after round 0 and is undecided there."""
    n, init, ho, R = kat_three_singletons()
    run = py_lattice(n, init, ho, R)
    assert [s[:3] for s in run.states[0]] == [(1, 0, NONE32), (2, 0, NONE32), (4, 0, NONE32)]
    assert [s[:3] for s in run.states[1]] == [(7, 0, NONE32)] * 3
    assert [s[:3] for s in run.states[2]] == [(7, 1, 7)] * 3


def test_halted_majority_blocks_later_decisions():
    """Once more than n/2 processes have halted nobody else can decide: the instance stays
    undecided to R and Termination is reported as never, not as a violation."""
    ho = [[0b00111, 0b00111, 0b00111, 0b01000, 0b10000]] + [[0b11111] * 5] * 5
    run = py_lattice(5, (1, 1, 1, 2, 2), ho, 6)
    assert [r[1] for r in run.rec] == [0, 0, 0, -1, -1]
    assert run.term_round == NEVER and run.first_fail == [NEVER] * 6
    assert run.rec[3][3] == 2 and run.rec[4][3] == 2   # p3, p4 hear only each other's {1} afterwards


# ------------------------------------------------------------------------------------ 2. properties
def sparse_case(rng, n, R=4):
    """A random sparse schedule: every link kept with a per-instance probability in [0.3, 0.9]."""
    keep = rng.uniform(0.3, 0.9)
    ho = [[sum(1 << q for q in range(n) if q == p or rng.random() < keep) for p in range(n)] for _ in range(R)]
    U = int(rng.integers(2, 5))
    v = rng.integers(0, U * U, n)
    init = [(1 << (int(x) // U)) | (1 << (int(x) % U)) for x in v]
    return init, ho, R


def test_reference_holds_and_mutant_breaks_comparability_on_random_schedules():
    rng = np.random.default_rng(11)
    ref_bad = mut_bad = total = 0
    for t in range(300):
        n = 5 + t % 5
        init, ho, R = sparse_case(rng, n)
        ref = py_lattice(n, init, ho, R)
        mut = py_lattice(n, init, ho, R, variant=1)
        total += 1
        ref_bad += any(ref.first_fail[s] != NEVER for s in VIOLATION_SLOTS)
        mut_bad += mut.first_fail[2] != NEVER
        # the mutant changes only the threshold: validity and irrevocability still hold
        assert [mut.first_fail[s] for s in (3, 4, 5)] == [NEVER] * 3
        assert mut.first_fail[0] == mut.first_fail[1] == mut.first_fail[2]
    assert total >= 200
    assert ref_bad == 0
    assert mut_bad > 0


# ------------------------------------------------------------------------------------ 3. the layers' tables
def test_abi_rows():
    assert abi.PSG_ALG_LATTICE == LATTICE
    assert abi.CLASS_TO_ALG["example.LatticeAgreement"] == LATTICE
    assert abi.CHECK_NAMES[LATTICE] == SLOTS
    assert abi.VIOLATION_SLOTS[LATTICE] == VIOLATION_SLOTS
    alg = psync.ALGORITHMS["example.LatticeAgreement"]()
    assert (alg.alg_id, alg.phase_length, alg.default_rounds(64), alg.default_value_range(64)) == (LATTICE, 1, 8, 16)
    s = alg.default_schedule(64)
    assert (s.drop_log2, s.good_round, s.crash_fmax, s.ho_min, s.self_bit) == (2, 0.0, None, None, True)
