"""LatticeAgreement pinned to the reference: a literal restatement and hand KATs.

`py_lattice` (tests/restatement.py) restates `LatticeAgreementProcess`
(example/LatticeAgreement.scala:39-65) in pure Python under explicit HO sets, with send / mailbox /
update as the source writes them on Python sets, and evaluates the six check slots of DESIGN.md §2
after every round by direct set arithmetic. It is the reference side of the GPU tests
(tests/test_gpu_lattice.py): the oracle library has no LatticeAgreement and the reference's spec is
`TrivialSpec //TODO` (:74).

Sets cross the C ABI as int32 bit masks (bit e = element e of {0..30}); inputs are taken
`& 0x7FFFFFFF`. The KATs (beside py_lattice) were worked from the Scala source line by line.
"""
import numpy as np
import pytest

from round_amd import abi, psync

from restatement import LATTICE_KAT_IDS, LATTICE_KATS, NEVER, NONE32, py_lattice
from restatement import lattice_kat_three_singletons as kat_three_singletons

LATTICE = 11
SLOTS = ["Safety", "Invariant0", "Comparability", "DownwardValidity", "UpwardValidity", "Irrevocability"]
VIOLATION_SLOTS = [0, 2, 3, 4, 5]


# ------------------------------------------------------------------------------------ 1. hand KATs
@pytest.mark.parametrize("kat,variant,recs,ff,term,nd", LATTICE_KATS, ids=LATTICE_KAT_IDS)
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
    assert len(py_lattice(*kat_three_singletons()).first_fail) == len(SLOTS) == 6
    assert abi.VIOLATION_SLOTS[LATTICE] == VIOLATION_SLOTS
    alg = psync.ALGORITHMS["example.LatticeAgreement"]()
    assert (alg.alg_id, alg.phase_length, alg.default_rounds(64), alg.default_value_range(64)) == (LATTICE, 1, 8, 16)
    s = alg.default_schedule(64)
    assert (s.drop_log2, s.good_round, s.crash_fmax, s.ho_min, s.self_bit) == (2, 0.0, None, None, True)
