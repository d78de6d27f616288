"""TwoPhaseCommit pinned to the reference: a literal restatement, the formal model, the Spec.

`py_tpc` (tests/restatement.py) restates `TpcProcess` (example/TwoPhaseCommit.scala:15-79) in pure
Python under explicit HO sets, with send / mailbox / update per round as the source writes them, and
evaluates the Spec (:93-105) on the state variable `decision` after every round. It is the reference
side of the GPU tests (tests/test_gpu_tpc.py): the oracle library has no TwoPhaseCommit.

The reference also holds a formal model of the algorithm, psync/logic/TpcExample.scala. Its
transition relations `round1a` (:45-60) and `round2a` (:90-101) and its `invariant1`, `agreement`
and `validity` (:36-37, 120-123) are restated below as Python predicates and checked on the
restatement's runs over random schedules. The model's symbols map to the process state as
    data0(j)   = vote of j (io.canCommit)
    vote(i)    = i is the coordinator and its decision is Some(true)   (the coordinator's verdict)
    decided(i) = i took round 2's update and its decision is defined
    data(i)    = decided(i) and decision(i) == Some(true)
What the pin covers: the slot-1 and slot-2 transitions (round2a for the coordinator only under
self delivery: without it the coordinator keeps its slot-1 decision, which the model calls
undecided) and the invariant. What it does not cover: the coordinator's early Some(_) between
slots 1 and 2 (the model's decided(coord) is false there, the Spec's decision.isDefined true) and
the decide(None) callback, which the model does not have.
"""
import ctypes as C

import numpy as np
import pytest

from round_amd import abi, formula as F, lib, psync, schedules as S

import formula_ref
from restatement import NEVER, NONE32, TPC_KAT_IDS, TPC_KATS, full_ho, ho_ints, py_tpc
from restatement import tpc_kat_full, tpc_kat_mutant_n5 as kat_mutant_n5, tpc_kat_two_rounds as kat_two_rounds

TPC = abi.PSG_ALG_TPC


# ------------------------------------------------------------------------------------ 1. hand KATs
@pytest.mark.parametrize("kat,recs,ff,term,nd", TPC_KATS, ids=TPC_KAT_IDS)
def test_hand_kats(kat, recs, ff, term, nd):
    n, coord, votes, ho, R = kat()
    run = py_tpc(n, coord, votes, ho, R)
    assert [r[:3] for r in run.rec] == recs
    assert [r[3] for r in run.rec] == list(votes)
    assert (run.first_fail, run.term_round, run.n_decided) == (ff, term, nd)


def test_two_rounds_leave_only_the_coordinator_defined():
    n, coord, votes, ho, R = kat_two_rounds()
    run = py_tpc(n, coord, votes, ho, R)
    assert run.states[2] == [True, None, None]


def test_mutant_kat_breaks_validity():
    n, coord, votes, ho, R = kat_mutant_n5()
    ok = py_tpc(n, coord, votes, ho, R)
    assert [r[:3] for r in ok.rec] == [(0, 2, 2)] * n and ok.first_fail == [NEVER] * 4  # aborts, no violation
    bad = py_tpc(n, coord, votes, ho, R, mutant=True)
    assert [r[0] for r in bad.rec] == [1] * n
    assert bad.first_fail == [2, 2, NEVER, 2]  # Safety, Invariant0 and Validity from check point 2


# ------------------------------------------------------------------------------------ 2. the TpcExample pin
class Model:
    """The symbols of TpcExample.scala over a py_tpc state (see the module docstring)."""

    def __init__(self, run, coord, votes, c):
        d = run.states[c]
        n = run.n
        self.n, self.coord = n, coord
        self.data0 = [bool(v) for v in votes]
        self.vote = [i == coord and d[i] is True for i in range(n)]
        self.decided = [c >= 3 and d[i] is not None for i in range(n)]
        self.data = [self.decided[i] and d[i] is True for i in range(n)]


def round1a(m, m1, ho_k, i):
    """TpcExample.scala:45-60 for process i; ho_k[i]: HO(i) in the round."""
    n, coord = m.n, m.coord
    card = sum(1 for j in range(n) if (ho_k[i] >> j) & 1 and m.data0[j])
    return ((not (i == coord and card == n) or m1.vote[i])
            and (not (i == coord and card != n) or not m1.vote[i])
            and (i == coord or m.vote[i] == m1.vote[i])
            and m.data[i] == m1.data[i] and m.decided[i] == m1.decided[i])


def round2a(m, m1, ho_k, i):
    """TpcExample.scala:90-101 for process i."""
    heard = bool((ho_k[i] >> m.coord) & 1)
    return ((not heard or (m1.decided[i] and m1.data[i] == m.vote[m.coord]))
            and (heard or (not m1.decided[i] and m1.data[i] == m.data[i]))
            and m.vote[i] == m1.vote[i])


def invariant1(m):
    """TpcExample.scala:120-123."""
    vc = m.vote[m.coord]
    return all((not vc or m.data0[i]) and (not m.decided[i] or m.data[i] == vc) for i in range(m.n))


def agreement(m):
    """TpcExample.scala:36."""
    return all(not (m.decided[i] and m.decided[j]) or m.data[i] == m.data[j] for i in range(m.n) for j in range(m.n))


def validity(m):
    """TpcExample.scala:37, as written: forall i. exists j. decided(i) && data(i) ==> data0(j)."""
    return all(any(not (m.decided[i] and m.data[i]) or m.data0[j] for j in range(m.n)) for i in range(m.n))


@pytest.mark.parametrize("n,self_bit", [(3, True), (3, False), (5, True), (8, False), (70, True)])
def test_tpcexample_model_holds_on_random_schedules(n, self_bit):
    rng = np.random.default_rng(100 + n)
    I, R = 200 if n < 64 else 40, 4
    hos = S.random_omission(rng, I, R, n, 0.9 if n < 64 else 255 / 256, self_bit)
    seen = set()
    for i in range(I):
        coord = int(rng.integers(0, n))
        votes = (rng.random(n) >= 0.5 / n).astype(int)
        ho = ho_ints(hos[i])
        run = py_tpc(n, coord, votes, ho, R)
        ms = [Model(run, coord, votes, c) for c in range(R + 1)]
        assert ms[0].vote == [False] * n and ms[0].decided == [False] * n            # initialState (:39)
        for p in range(n):
            assert round1a(ms[1], ms[2], ho[1], p)
            if p != coord or (ho[2][p] >> coord) & 1:
                assert round2a(ms[2], ms[3], ho[2], p)
        for c in range(R + 1):
            assert invariant1(ms[c]) and agreement(ms[c]) and validity(ms[c])
        assert run.first_fail == [NEVER] * 4
        seen.add((run.states[R][coord], any(d is None for d in run.states[R])))
    if n < 64:
        assert len(seen) >= 3  # commits, aborts and suspected coordinators all occur


def test_tpcexample_model_rejects_the_mutant():
    """A lost no-vote: the mutant's slot-1 step is not round1a's, and invariant1 and the Spec's
    Validity break. The model's own `validity` is the weak exists-j form: it breaks only when
    nobody votes yes (then the mutant commits on an empty mailbox)."""
    n, coord, votes, ho, R = kat_mutant_n5()
    run = py_tpc(n, coord, votes, ho, R, mutant=True)
    ms = [Model(run, coord, votes, c) for c in range(R + 1)]
    assert not round1a(ms[1], ms[2], ho[1], coord)
    assert not invariant1(ms[2]) and not invariant1(ms[3])
    assert run.first_fail[3] == 2
    votes0 = (0, 0, 0)
    ho0 = full_ho(3, 3)
    ho0[1][0] = 0  # pure HO: the coordinator hears no vote at all
    run0 = py_tpc(3, 0, votes0, ho0, 3, mutant=True)
    ms0 = [Model(run0, 0, votes0, c) for c in range(4)]
    assert not round1a(ms0[1], ms0[2], ho0[1], 0)
    assert not validity(ms0[3]) and run0.first_fail[3] == 2
    good = py_tpc(3, 0, votes0, ho0, 3)
    assert validity(Model(good, 0, votes0, 3)) and good.first_fail == [NEVER] * 4


# ------------------------------------------------------------------------------------ 3. Spec parity
def trace_of(runs, votes_of):
    """The state trace psg_run_batch_spec writes, [count][R+1][9][n] int32, from py_tpc states."""
    n, R = runs[0].n, runs[0].R
    tr = np.zeros((len(runs), R + 1, 9, n), np.int32)
    for i, run in enumerate(runs):
        for c in range(R + 1):
            for p in range(n):
                d = run.states[c][p]
                tr[i, c, F.FIELD_X, p] = tr[i, c, F.FIELD_VOTE, p] = int(bool(votes_of[i][p]))
                tr[i, c, F.FIELD_DECIDED, p] = int(d is not None)
                tr[i, c, F.FIELD_DECISION, p] = NONE32 if d is None else int(d)
                tr[i, c, F.FIELD_HOSIZE, p] = n
    return tr


def _spec_cases():
    rng = np.random.default_rng(9)
    n, R, I = 6, 4, 60
    hos = S.random_omission(rng, I, R, n, 0.85, False)
    runs, votes = [], []
    for i in range(I):
        v = (rng.random(n) >= 0.15).astype(int)
        runs.append(py_tpc(n, int(rng.integers(0, n)), v, ho_ints(hos[i]), R, mutant=i % 2 == 1))
        votes.append(v)
    return n, R, runs, votes


def test_reference_spec_equals_the_restatements_checks(oracle_mod):
    n, R, runs, votes = _spec_cases()
    assert any(r.first_fail[3] != NEVER for r in runs) and any(r.first_fail == [NEVER] * 4 for r in runs)
    spec = F.REFERENCE_SPECS[TPC]()
    prog = F.compile_spec(spec, TPC)
    assert prog.slot_names == abi.CHECK_NAMES[TPC]
    tr = trace_of(runs, votes)
    flat = (C.c_int32 * tr.size)(*[int(v) for v in tr.ravel()])
    want = ([r.first_fail for r in runs], [r.term_round for r in runs])
    assert tuple(oracle_mod.vm_run(prog, flat, len(runs), n, R)) == want          # CPU Spec interpreter
    assert tuple(formula_ref.evaluate(spec, flat, len(runs), n, R)) == want       # direct evaluation
    assert tuple(oracle_mod.vm_run(lib.spec_from_text(F.to_text(spec), TPC), flat, len(runs), n, R)) == want


# ------------------------------------------------------------------------------------ 4. ABI
def test_abi_row():
    L = lib.load()
    assert L.psg_alg_from_class(b"example.TwoPhaseCommit") == 10 == TPC
    assert L.psg_check_count(TPC) == 4 == len(py_tpc(*tpc_kat_full()).first_fail)
    assert lib.check_names(TPC) == ["Safety", "Invariant0", "UniformAgreement", "Validity"]
    assert L.psg_check_name(TPC, 4) is None
    assert psync.ALGORITHMS["example.TwoPhaseCommit"]().violation_slots == [0, 2, 3]
    c = abi.Config()
    assert L.psg_config_default(C.byref(c), TPC, 64) == 0
    assert (c.rounds, c.value_range, c.param, c.sched.drop_log2, c.sched.good_p32) == (3, 128, 0, 6, 0)


@pytest.mark.parametrize("coord", [-1, 8])
def test_create_rejects_a_coordinator_outside_the_group(coord):
    L = lib.load()
    cfg = psync.make_config(psync.TwoPhaseCommit(coord=coord), 8, batch_capacity=16)
    h = C.c_void_p()
    assert L.psg_create(C.byref(h), C.byref(cfg)) == abi.PSG_EINVAL
    assert h.value is None and b"coord" in L.psg_create_error()


def test_fixed_coord_live_predicate():
    """schedules.fixed_coord_live against the livenessPredicate read per round (:90-92), and: under
    it every process gets Some(_), Some(true) when everyone votes yes."""
    rng = np.random.default_rng(4)
    n, R, I, coord = 7, 3, 300, 4
    hos = S.random_omission(rng, I, R, n, 0.93, True)
    live = S.fixed_coord_live(hos, n, coord)
    assert live[:, 0].all() and 0 < live[:, 1:].all(1).sum() < I
    for i in range(I):
        ho = ho_ints(hos[i])
        assert live[i, 1] == (ho[1][coord] == (1 << n) - 1)
        assert live[i, 2] == all((ho[2][q] >> coord) & 1 for q in range(n))
        if live[i].all():
            run = py_tpc(n, coord, [1] * n, ho, R)
            assert [r[:2] for r in run.rec] == [(1, 2)] * n and run.term_round == 3
