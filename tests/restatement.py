"""Pure-Python restatements of the reference, shared by the CPU and GPU tests (no GPU needed).

`py_tpc` restates `TpcProcess` (example/TwoPhaseCommit.scala:15-79) and `py_lattice`
`LatticeAgreementProcess` (example/LatticeAgreement.scala:39-65) under explicit HO sets, with send /
mailbox / update per round as the sources write them; each evaluates its check slots after every
round. They are the reference side of the GPU tests of the two algorithms (the oracle library has
neither), with the hand KATs worked from the Scala sources line by line and the per-instance digest
of DESIGN.md §4 over their records. tests/test_reference_tpc.py and tests/test_reference_lattice.py
pin them.

Also here, because more than one test module reads them: the HO-set conversions, `mmor`
(OtrExample.scala:67-75), the Scala Map iteration order (`py_champ`) and the symbols of
LvExample.scala over an oracle trace (tests/test_reference_lv.py has the four rounds).
"""
import numpy as np

from round_amd import abi, psync

NEVER = abi.PSG_NEVER
NONE32 = -(1 << 31)
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------ HO sets, digest
def ho_ints(ho_arr):
    """uint64 [R][n][W] -> Python ints [R][n]."""
    R, n, W = ho_arr.shape
    return [[sum(int(ho_arr[k, p, w]) << (64 * w) for w in range(W)) for p in range(n)] for k in range(R)]


def ho_array(hos, n):
    """Python ints [I][R][n] -> uint64 [I][R][n][W]."""
    W = (n + 63) // 64
    out = np.zeros((len(hos), len(hos[0]), n, W), np.uint64)
    for i, h in enumerate(hos):
        for k, row in enumerate(h):
            for p, m in enumerate(row):
                for w in range(W):
                    out[i, k, p, w] = (m >> (64 * w)) & M64
    return out


def full_ho(n, R):
    return [[(1 << n) - 1] * n for _ in range(R)]


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def digest_of(run):
    """The per-instance digest of a py_tpc / py_lattice run, over its rec rows
    (decision, decision_round, halt_round, final_x)."""
    d = 0
    for pid, (dec, dr, hr, x) in enumerate(run.rec):
        y = (pid << 32) | ((dr & 0xFFFF) << 16) | (hr & 0xFFFF)
        z = ((dec & 0xFFFFFFFF) << 32) | (x & 0xFFFFFFFF)
        d = (d + splitmix64(z ^ splitmix64(y))) & M64
    return d


# ------------------------------------------------------------------------------------ TwoPhaseCommit
class TpcRun:
    """Result of py_tpc: per-process records, the Spec's verdicts, the states of every check point."""

    def __init__(self, n, R):
        self.n, self.R = n, R
        self.rec = []         # per p: (decision, decision_round, halt_round, vote) as the C ABI reports them
        self.states = []      # per check point: list of decision (None / False / True) per p
        self.first_fail = [NEVER] * 4   # Safety, Invariant0, UniformAgreement, Validity
        self.term_round = NEVER
        self.n_decided = 0


def py_tpc(n, coord, votes, ho, R, mutant=False):
    """TpcProcess under explicit HO sets ho[k][p] (bit q: p hears q in round k), R rounds.
    mutant: the coordinator drops `mailbox.size == n` (:51)."""
    vote = [bool(v) for v in votes]          # init(io), :22-27: vote = io.canCommit
    decision = [None] * n                    # decision = None
    halted = [False] * n
    cb = [None] * n                          # (value passed to callback.decide, round), :73
    out = TpcRun(n, R)

    def check(c):
        defined = [d for d in decision if d is not None]
        validity = (not any(d is True for d in decision)) or all(vote)            # :104
        agreement = all(a == b for a in defined for b in defined)                 # :102
        inv = validity and agreement                                              # :94-95
        for s, ok in enumerate((inv, inv, agreement, validity)):
            if not ok and out.first_fail[s] == NEVER:
                out.first_fail[s] = c
        if out.term_round == NEVER and len(defined) == n:
            out.term_round = c
        out.states.append(list(decision))

    check(0)
    for k in range(R):
        slot = k % 3
        senders = [q for q in range(n) if not halted[q]]
        # send(): Map[destination -> payload] of every non-halted process
        sent = {}
        for q in senders:
            if slot == 0:
                sent[q] = {p: True for p in range(n)} if q == coord else {}       # :31-34 broadcast(true)
            elif slot == 1:
                sent[q] = {coord: vote[q]}                                        # :43-45
            else:
                if q == coord:
                    assert decision[q] is not None  # decision.get (:63): slot 1 of this phase ran first
                    sent[q] = {p: decision[q] for p in range(n)}
                else:
                    sent[q] = {}
        inbox = [{} for _ in range(n)]  # what was sent to p (sender -> payload), before the HO filter
        for q in senders:
            for p, v in sent[q].items():
                inbox[p][q] = v
        new = list(decision)
        exits = []
        for p in senders:
            mailbox = {q: v for q, v in inbox[p].items() if (ho[k][p] >> q) & 1}
            if slot == 1:
                if p == coord:                                                    # :50-56
                    if (mutant or len(mailbox) == n) and all(mailbox.values()):
                        new[p] = True
                    else:
                        new[p] = False
            elif slot == 2:
                if len(mailbox) > 0:                                              # :70-72
                    new[p] = next(iter(mailbox.values()))                         # mailbox.head._2
                cb[p] = (new[p], k)                                               # callback.decide(decision)
                exits.append(p)                                                   # exitAtEndOfRound()
        decision = new
        for p in exits:
            halted[p] = True
        check(k + 1)
    for p in range(n):
        if cb[p] is None:
            out.rec.append((NONE32, -1, -1, int(vote[p])))
        elif cb[p][0] is None:                       # decide(None): coordinator suspected, not a decision
            out.rec.append((NONE32, -1, cb[p][1], int(vote[p])))
        else:
            out.rec.append((int(cb[p][0]), cb[p][1], cb[p][1], int(vote[p])))
    out.n_decided = sum(1 for r in out.rec if r[1] >= 0)
    return out


def tpc_outcomes(runs):
    got = set()
    for run in runs:
        decs = [r[0] for r in run.rec]
        if all(d == 1 for d in decs):
            got.add("commit")
        if any(d == 0 for d in decs):
            got.add("abort")
        if any(d == NONE32 for d in decs):
            got.add("suspect")
    return got


# hand KATs: (n, coord, votes, ho, R)
def tpc_kat_full():
    return 3, 0, (1, 1, 1), full_ho(3, 3), 3


def tpc_kat_coord_misses_vote():
    ho = full_ho(3, 3)
    ho[1][0] = 0b011  # the coordinator does not hear p2's vote
    return 3, 0, (1, 1, 1), ho, 3


def tpc_kat_receiver_misses_coord():
    ho = full_ho(3, 3)
    ho[2][1] = 0b110  # p1 does not hear the coordinator's decision
    return 3, 0, (1, 1, 1), ho, 3


def tpc_kat_coord_deaf_to_itself_slot1():
    ho = full_ho(3, 3)
    ho[1][0] = 0b110  # pure HO: the coordinator's own vote is not delivered
    return 3, 0, (1, 1, 1), ho, 3


def tpc_kat_coord_deaf_to_itself_slot2():
    ho = full_ho(3, 3)
    ho[2][0] = 0b110  # pure HO: the coordinator does not hear its own broadcast
    return 3, 0, (1, 1, 1), ho, 3


def tpc_kat_two_rounds():
    return 3, 0, (1, 1, 1), full_ho(3, 2), 2


def tpc_kat_mutant_n5():
    """n = 5, coord = 0, p3 votes no and its slot-1 link to the coordinator is dropped."""
    ho = full_ho(5, 3)
    ho[1][0] = 0b10111
    return 5, 0, (1, 1, 1, 0, 1), ho, 3


def tpc_kat_coord_crashed_from_round2():
    """The coordinator crashes by send omission from round 2: nobody else hears its decision."""
    n = 5
    ho = full_ho(n, 3)
    for p in range(1, n):
        ho[2][p] = ((1 << n) - 1) & ~1
    return n, 0, (1, 1, 1, 1, 1), ho, 3


# (kat, per-process (decision, decision_round, halt_round), first_fail, term_round, n_decided)
TPC_KATS = [
    (tpc_kat_full, [(1, 2, 2)] * 3, [NEVER] * 4, 3, 3),
    (tpc_kat_coord_misses_vote, [(0, 2, 2)] * 3, [NEVER] * 4, 3, 3),
    (tpc_kat_receiver_misses_coord, [(1, 2, 2), (NONE32, -1, 2), (1, 2, 2)], [NEVER] * 4, NEVER, 2),
    (tpc_kat_coord_deaf_to_itself_slot1, [(0, 2, 2)] * 3, [NEVER] * 4, 3, 3),
    (tpc_kat_coord_deaf_to_itself_slot2, [(1, 2, 2)] * 3, [NEVER] * 4, 3, 3),
    (tpc_kat_two_rounds, [(NONE32, -1, -1)] * 3, [NEVER] * 4, NEVER, 0),
    (tpc_kat_coord_crashed_from_round2, [(1, 2, 2)] + [(NONE32, -1, 2)] * 4, [NEVER] * 4, NEVER, 1),
]
TPC_KAT_IDS = [k[0].__name__[len("tpc_"):] for k in TPC_KATS]


# ------------------------------------------------------------------------------------ LatticeAgreement
# Sets cross the C ABI as int32 bit masks (bit e = element e of {0..30}); inputs are taken & 0x7FFFFFFF.
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


# hand KATs: (n, initial masks, ho, R)
def lattice_kat_three_singletons():
    """Round 0: nobody has two equal values (cnt = 1, not > 1), everyone joins to {0,1,2} = 7.
    Round 1: cnt = 3 > 1: all decide 7."""
    return 3, (1, 2, 4), full_ho(3, 2), 2


def lattice_kat_two_comparable_decisions():
    """Round 0: p0, p1 hear {0,1,2}, all {0}: cnt = 3 > 2, decide {0}. p2 hears {2,3}: values
    {0}, {0,1}, cnt = 1: joins to {0,1}. p3, p4 hear {3,4}: cnt = 2, not > 2: stay {0,1}.
    Round 1: p2..p4 hear {2,3,4}, all {0,1}: cnt = 3 > 2, decide {0,1}."""
    ho = [[0b00111, 0b00111, 0b01100, 0b11000, 0b11000], [0b11100] * 5]
    return 5, (1, 1, 1, 3, 3), ho, 2


def lattice_kat_mutant_n5():
    """variant 1 (cnt > n/4 = 1): p0, p1 hear each other: cnt = 2, decide {0}; p2, p3 likewise
    decide {1}; p4 hears itself: cnt = 1, stays. {0} and {1} are incomparable."""
    return 5, (1, 1, 2, 2, 2), [[0b00011, 0b00011, 0b01100, 0b01100, 0b10000]], 1


def lattice_kat_single_self():
    return 1, (5,), [[1]], 1      # cnt = 1 > 0: decides its input in round 0


def lattice_kat_single_deaf():
    return 1, (5,), [[0], [0]], 2  # empty mailbox: cnt = 0, join of nothing: never decides


def lattice_kat_bottom_and_high_bits():
    """p0..p2 hold bottom (0) and hear each other: cnt = 3 > 2, they decide the empty set (decision
    0 with decision_round 0). p3, p4 hold -1 = every bit: bit 31 is dropped on input (0x7FFFFFFF);
    they hear only themselves (cnt = 1) in round 0 and p0..p4 minus the halted in round 1 (cnt = 2)."""
    ho = [[0b00111, 0b00111, 0b00111, 0b01000, 0b10000], [0b11111] * 5]
    return 5, (0, 0, 0, -1, -1), ho, 2


_H = 0x7FFFFFFF
# (kat, variant, per process (decision, decision_round, halt_round, final_x), first_fail, term_round, n_decided)
LATTICE_KATS = [
    (lattice_kat_three_singletons, 0, [(7, 1, 1, 7)] * 3, [NEVER] * 6, 2, 3),
    (lattice_kat_two_comparable_decisions, 0, [(1, 0, 0, 1)] * 2 + [(3, 1, 1, 3)] * 3, [NEVER] * 6, 2, 5),
    (lattice_kat_mutant_n5, 1, [(1, 0, 0, 1)] * 2 + [(2, 0, 0, 2)] * 2 + [(0, -1, -1, 2)],
     [1, 1, 1, NEVER, NEVER, NEVER], NEVER, 4),
    (lattice_kat_mutant_n5, 0, [(0, -1, -1, 1)] * 2 + [(0, -1, -1, 2)] * 3, [NEVER] * 6, NEVER, 0),
    (lattice_kat_single_self, 0, [(5, 0, 0, 5)], [NEVER] * 6, 1, 1),
    (lattice_kat_single_deaf, 0, [(0, -1, -1, 5)], [NEVER] * 6, NEVER, 0),
    (lattice_kat_bottom_and_high_bits, 0, [(0, 0, 0, 0)] * 3 + [(0, -1, -1, _H)] * 2, [NEVER] * 6, NEVER, 3),
]
LATTICE_KAT_IDS = [f"{k[0].__name__[len('lattice_'):]}-v{k[1]}" for k in LATTICE_KATS]


# ------------------------------------------------------------------------------------ OTR's mmor
def mmor(mailbox_vals):
    """OtrExample.scala:67-75 defs, literally: the value with card >= 1 whose card is
    maximal and which is Leq every other value of maximal card."""
    best = None
    for v in set(mailbox_vals):
        c = mailbox_vals.count(v)
        if c < 1:
            continue
        ok = all(mailbox_vals.count(p) <= c for p in set(mailbox_vals))
        ok = ok and all(v <= p for p in set(mailbox_vals) if mailbox_vals.count(p) == c)
        if ok:
            assert best is None, "defs determine mmor uniquely"
            best = v
    return best


# ------------------------------------------------------------------------------------ Scala Map order
def py_improve(h):
    m = 0xFFFFFFFF
    x = (h + (~(h << 9) & m)) & m
    x ^= x >> 14
    x = (x + (x << 4)) & m
    x ^= x >> 10
    return x


def py_champ(keys, shift=0):
    groups = {}
    for k in keys:
        groups.setdefault((py_improve(k) >> shift) & 31, []).append(k)
    out = [g[0] for f, g in sorted(groups.items()) if len(g) == 1]
    for f, g in sorted(groups.items()):
        if len(g) > 1:
            out += py_champ(g, shift + 5)
    return out


# ------------------------------------------------------------------------------------ LvExample's symbols
# trace fields (include/psg.h enum psg_field)
NF = 9
X, DECIDED, DECISION, TS, READY, COMMIT, VOTE = 0, 1, 2, 3, 4, 5, 6


def lv_maxts_ok(box, val):
    """maxTSdef (LvExample.scala:78-97) for one non-empty map box = {pid: (value, ts)}."""
    return any(box[j][0] == val and all(box[i][0] == val or box[i][1] <= box[j][1] for i in box) for j in box)


def lv_state(row, n):
    d = {f: [int(v) for v in row[f]] for f in (X, DECIDED, DECISION, TS, READY, COMMIT, VOTE)}
    return {
        "data": [d[DECISION][i] if d[DECIDED][i] else d[X][i] for i in range(n)],
        "decided": [bool(v) for v in d[DECIDED]],
        "ts": d[TS], "ready": [bool(v) for v in d[READY]], "commit": [bool(v) for v in d[COMMIT]],
        "vote": d[VOTE],
    }


def lv_frame(pre, post, names, n):
    for f in names:
        for i in range(n):
            if pre[f][i] != post[f][i]:
                return f"frame {f} of p{i}: {pre[f][i]} -> {post[f][i]}"
    return None


def lv_invariant1(n, r, s, data0):
    """LvExample.scala:221-238, V and the phase type finitized exactly: v ranges over the
    data values (A is a non-empty majority), t over the timestamps (A = {i : t <= ts(i)}
    only changes at a timestamp, and every ts <= r)."""
    co = r % n
    no_dec = all(not s["decided"][i] and not s["ready"][i] for i in range(n))
    maj = False
    if not no_dec:
        for t in sorted(set(s["ts"])):
            if t > r:
                continue
            A = [i for i in range(n) if t <= s["ts"][i]]
            if not n < 2 * len(A):
                continue
            for v in set(s["data"][i] for i in A):
                if all((i not in A or s["data"][i] == v) and (not s["decided"][i] or s["data"][i] == v) and
                       (not s["commit"][i] or s["vote"][i] == v) and (not s["ready"][i] or s["vote"][i] == v) and
                       (s["ts"][i] != r or s["commit"][co]) for i in range(n)):
                    maj = True
                    break
            if maj:
                break
    valid = all(s["data"][i] in data0 for i in range(n))
    return (no_dec or maj) and valid


def lv_agreement(n, s):
    """LvExample.scala:60."""
    return len({s["data"][i] for i in range(n) if s["decided"][i]}) <= 1


# (n, count, schedule, tiebreak, value_range) of the LastVoting model pins
_S = psync.HOSchedule
LV_MODEL_CASES = [
    (4, 300, _S(drop_log2=2, good_round=0.0), abi.PSG_TIE_CHAMP, 3),
    (5, 300, _S(drop_log2=1, good_round=0.0, crash_fmax=2), abi.PSG_TIE_CHAMP, 4),
    (7, 300, _S(drop_log2=2, good_round=0.0, self_bit=False), abi.PSG_TIE_CHAMP, 3),
    (16, 200, _S(drop_log2=3, good_round=0.0, crash_fmax=7), abi.PSG_TIE_CHAMP, 5),
    (16, 200, _S(drop_log2=1, good_round=0.0), abi.PSG_TIE_MIN_PID, 5),
    (64, 60, _S(drop_log2=4, good_round=0.0, crash_fmax=31), abi.PSG_TIE_CHAMP, 32767),
    (64, 60, _S(drop_log2=2, good_round=0.0), abi.PSG_TIE_CHAMP, 3),
    (64, 60, _S(drop_log2=2, good_round=0.0, crash_fmax=20), abi.PSG_TIE_MIN_PID, 6),
]
