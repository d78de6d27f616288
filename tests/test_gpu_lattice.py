"""GPU: LatticeAgreement (psg_lattice.hip) against the pure-Python restatement of the reference.

The oracle library has no LatticeAgreement, so the reference side is `py_lattice`
(tests/restatement.py, written from example/LatticeAgreement.scala). Explicit and
seeded schedules, hand KATs, sharding and fetch, a custom Spec in its three forms, the adversary.
"""
import functools

import numpy as np
import pytest

from round_amd import abi, adversary as A, formula as F, psync, records, schedules as S

import spec_cases
from gpu_support import (assert_equal_to_restatement, assert_multi_device_equals_one_device, gpu_explicit, seeded_inits,
                         sharding_and_fetch)
from restatement import (LATTICE_KAT_IDS, LATTICE_KATS, M64, NEVER, digest_of, ho_array, ho_ints, lattice_kat_mutant_n5,
                         py_lattice)

pytestmark = pytest.mark.gpu
LATTICE = abi.PSG_ALG_LATTICE
NS = [1, 2, 3, 5, 63, 64, 65, 128, 129, 192, 193, 256]  # every W and both sides of each wave edge


def ending(run):
    return "all" if run.n_decided == run.n else ("none" if run.n_decided == 0 else "partly")


# ------------------------------------------------------------------------------------ 1. explicit schedules
def _cases_random():
    """Family (a): per n two cases over U x R x keep x self_bit, rotated so that every n, U in
    {1, 2, 31}, R in {1, 2, 8}, keep in {1/2, 3/4} and both self_bit values occur."""
    out = []
    Us, Rs = [1, 2, 31], [1, 2, 8]
    for a, n in enumerate(NS):
        out.append((n, Us[a % 3], Rs[(a + 1) % 3], 0.5, a % 2 == 0))
        out.append((n, Us[(a + 1) % 3], Rs[(a + a // 3) % 3], 0.75, a % 2 == 1))
    return out


def _count(n):
    return 40 if n <= 65 else 12


@functools.lru_cache(maxsize=None)
def _random_inputs(n, U, R, keep, self_bit):
    """Random links kept with probability `keep`; initial sets: one or two elements of {0..U-1}
    for even instances, a uniform subset for odd ones (many disagreeing elements: the general path
    stays live for several rounds, with partial batches of the W > 1 exchange)."""
    I = _count(n)
    rng = np.random.default_rng([n, U, R, int(keep * 4), int(self_bit)])
    ho = S.random_omission(rng, I, R, n, keep, self_bit)
    v = rng.integers(0, U * U, (I, n))
    inits = ((1 << (v // U)) | (1 << (v % U))).astype(np.int64)
    inits[1::2] = rng.integers(0, 1 << U, inits[1::2].shape)
    inits = inits.astype(np.int32)
    runs = [py_lattice(n, inits[i], ho_ints(ho[i]), R) for i in range(I)]
    return ho, inits, runs


@pytest.mark.parametrize("n,U,R,keep,self_bit", _cases_random())
def test_random_schedules_equal_the_restatement(n, U, R, keep, self_bit):
    ho, inits, runs = _random_inputs(n, U, R, keep, self_bit)
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.LatticeAgreement(), n, R, inits, ho, value_range=U)
    assert_equal_to_restatement(runs, pi, dec, dr, fs, fr)
    assert s.decided_processes == sum(r.n_decided for r in runs)
    assert list(s.fail_count)[:6] == [0] * 6


def staggered(rng, n, R, self_bit):
    """Family (b): every initial set is {0}, except max(1, n/8) outliers holding one extra element.
    In round 0 about a fifth of the rest hear all non-outliers and decide {0}; everyone else hears
    the outliers plus at most n/2 of the rest (no decision, the extras are joined in). Later
    rounds are full: the processes still live then decide the larger set."""
    m = max(1, n // 8)
    out = [int(q) for q in rng.choice(n, m, replace=False)]
    inits = [1] * n
    for j, q in enumerate(out):
        inits[q] = 1 | (2 << (j % 3))
    rest = [p for p in range(n) if p not in out]
    early = [p for p in rest if rng.random() < 0.2]
    restm, outm, full = sum(1 << q for q in rest), sum(1 << q for q in out), (1 << n) - 1
    ho = [[full] * n for _ in range(R)]
    for p in range(n):
        if p in early:
            ho[0][p] = restm
        else:
            others = [q for q in rest if q != p]
            size = int(rng.integers(0, max(0, min(len(others), n // 2 - 1)) + 1))
            sub = rng.choice(others, size, replace=False) if size else []
            ho[0][p] = outm | sum(1 << int(q) for q in sub) | (1 << p)
    if not self_bit:
        ho = [[h & ~(1 << p) for p, h in enumerate(row)] for row in ho]
    return inits, ho


@functools.lru_cache(maxsize=None)
def _staggered_inputs(n, R, self_bit):
    I = _count(n)
    rng = np.random.default_rng([n, R, int(self_bit), 7])
    cases = [staggered(rng, n, R, self_bit) for _ in range(I)]
    inits = np.array([c[0] for c in cases], np.int32)
    runs = [py_lattice(n, c[0], c[1], R) for c in cases]
    return ho_array([c[1] for c in cases], n), inits, runs


def _cases_staggered():
    return [(n, [2, 8, 3][a % 3], a % 2 == 0) for a, n in enumerate(x for x in NS if x >= 5)]


@pytest.mark.parametrize("n,R,self_bit", _cases_staggered())
def test_staggered_schedules_equal_the_restatement(n, R, self_bit):
    ho, inits, runs = _staggered_inputs(n, R, self_bit)
    # (on the restatement alone) some instance ends with two distinct, comparable decisions
    two = sum(1 for r in runs if len({x[0] for x in r.rec if x[1] >= 0}) > 1)
    assert two >= 1
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.LatticeAgreement(), n, R, inits, ho, value_range=4)
    assert_equal_to_restatement(runs, pi, dec, dr, fs, fr)
    assert list(s.fail_count)[:6] == [0] * 6


def test_the_cases_hold_every_ending():
    """On the restatement's runs alone: some instance of the file's cases ends all decided, some
    partly decided, some undecided, so that the comparisons above cannot pass vacuously."""
    got = set()
    for c in _cases_random():
        got |= {ending(r) for r in _random_inputs(*c)[2]}
    for c in _cases_staggered():
        got |= {ending(r) for r in _staggered_inputs(*c)[2]}
    assert got == {"all", "partly", "none"}


# ------------------------------------------------------------------------------------ 2. hand KATs
@pytest.mark.parametrize("kat,variant,recs,ff,term,nd", LATTICE_KATS, ids=LATTICE_KAT_IDS)
def test_hand_kats_on_the_gpu(kat, variant, recs, ff, term, nd):
    n, inits, ho, R = kat()
    run = py_lattice(n, inits, ho, R, variant)
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.LatticeAgreement(variant=variant), n, R, [inits], ho_array([ho], n),
                                          value_range=31)
    got = [(int(fr[0][p]["decision"]), int(dr[0][p]), int(fr[0][p]["halt_round"]), int(fr[0][p]["final_x"]))
           for p in range(n)]
    assert got == recs
    assert ([int(x) for x in pi[0]["first_fail"][:6]], int(pi[0]["term_round"]), int(pi[0]["n_decided"])) == (ff, term, nd)
    assert_equal_to_restatement([run], pi, dec, dr, fs, fr)


def test_mutant_kat_on_the_gpu():
    """Two disjoint quarters decide {0} and {1}: Comparability, Invariant0 and Safety first fail at
    check point 1 under variant 1; the reference algorithm decides nothing and holds."""
    n, inits, ho, R = lattice_kat_mutant_n5()
    hoa = ho_array([ho], n)
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.LatticeAgreement(variant=1), n, R, [inits], hoa)
    assert [int(x) for x in pi[0]["first_fail"][:6]] == [1, 1, 1, NEVER, NEVER, NEVER]
    assert [int(x) for x in dec[0]] == [1, 1, 2, 2, 0] and [int(x) for x in dr[0]] == [0, 0, 0, 0, -1]
    assert list(s.fail_count)[:6] == [1, 1, 1, 0, 0, 0]
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.LatticeAgreement(), n, R, [inits], hoa)
    assert [int(x) for x in pi[0]["first_fail"][:6]] == [NEVER] * 6 and [int(x) for x in dr[0]] == [-1] * n


# ------------------------------------------------------------------------------------ 3. seeded schedules
@pytest.mark.parametrize("n,drop,crash,U", [(5, 1, None, 16), (5, 2, None, 3), (64, 2, None, 16), (64, 2, 31, 16),
                                           (100, 1, None, 31), (256, 2, None, 16), (256, 1, None, 2)])
def test_seeded_run_equals_the_restatement_on_its_materialized_schedule(n, drop, crash, U, oracle_mod):
    cnt, begin = (96 if n <= 64 else 24), 1000
    alg = psync.LatticeAgreement()
    sched = psync.HOSchedule(drop_log2=drop, good_round=0.0, crash_fmax=crash)
    with psync.GpuRound(alg, n, seed=21, schedule=sched, value_range=U, batch_capacity=cnt) as g:
        cfg = g.cfg
        R = cfg.rounds
        assert R == 8
        ctx = g._ctx
        ho, cr = g.materialize_schedule(begin, cnt)
        s, pi = ctx.run_batch_np(begin, cnt)
        dec, dr = ctx.copy_decisions_np()
        fs, fr = ctx.fetch_np(np.arange(begin, begin + cnt, dtype=np.uint64))
        inits = seeded_inits(cfg, oracle_mod, begin, cnt)
        runs = [py_lattice(n, inits[i], ho_ints(ho[i]), R) for i in range(cnt)]
        assert_equal_to_restatement(runs, pi, dec, dr, fs, fr)
        assert (cr == -1).all() if crash is None else (cr >= 0).any()
        # the summary counters
        steps = [[(x[2] + 1 if x[2] >= 0 else R) for x in r.rec] for r in runs]
        assert (s.instances, s.process_rounds) == (cnt, cnt * n * R)
        assert s.active_process_rounds == sum(sum(x) for x in steps)
        assert s.live_instance_rounds == sum(max(x) for x in steps)
        assert s.decided_processes == sum(r.n_decided for r in runs)
        assert list(s.fail_count)[:6] == [0] * 6
        assert s.digest & M64 == sum(digest_of(r) for r in runs) & M64
        hist = [0] * (R + 2)
        for r in runs:
            hist[R + 1 if r.term_round == NEVER else r.term_round] += 1
        assert [s.term_hist[c] for c in range(R + 2)] == hist
        # replay through psg_load_schedule: the same run bit for bit
        ctx.load_inputs(begin, cnt, inits)
        ctx.load_schedule(begin, cnt, ho, None)
        s2, pi2 = ctx.run_batch_np(begin, cnt)
        assert s2.digest == s.digest and pi2.tobytes() == pi.tobytes()
        # ... and with the inputs seeded on the device (psg_load_inputs without host values)
        ctx.load_inputs(begin, cnt, None)
        s3, pi3 = ctx.run_batch_np(begin, cnt)
        assert s3.digest == s.digest and pi3.tobytes() == pi.tobytes()


# ------------------------------------------------------------------------------------ 4. sharding and fetch
@pytest.mark.parametrize("n,cnt", [(64, 1), (64, 3), (5, 5), (64, 200), (130, 50)])
def test_sharding_and_fetch_equal_one_range(n, cnt):
    for rec in sharding_and_fetch(psync.LatticeAgreement(), n, cnt):
        assert (rec["halt_round"] == rec["decision_round"]).all()


def test_multi_device_context_equals_one_device():
    assert_multi_device_equals_one_device(psync.LatticeAgreement())


# ------------------------------------------------------------------------------------ 5. rounds past 64
def test_rounds_past_64_check_only_tail():
    """R = 70: everyone has halted after two rounds, the other 68 check points are evaluated on
    the frozen state; the mutant's first_fail stays 1 and a never-failing slot stays PSG_NEVER
    (check points past 63 need the full uint8 width)."""
    n, R = 5, 70
    ho = [[0b00111, 0b00111, 0b01100, 0b11000, 0b11000]] + [[0b11100] * 5] * (R - 1)
    inits = (1, 1, 1, 3, 3)
    run = py_lattice(n, inits, ho, R)
    assert run.term_round == 2 and len(run.states) == R + 1
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.LatticeAgreement(), n, R, [inits], ho_array([ho], n))
    assert_equal_to_restatement([run], pi, dec, dr, fs, fr)
    assert (s.active_process_rounds, s.live_instance_rounds, s.process_rounds) == (1 + 1 + 3 * 2, 2, n * R)
    # three decide in round 0, then p3 and p4 never hold a majority (p4 deaf until round 66): live to R
    ho2 = [[0b00111, 0b00111, 0b00111, 0b11000, 0]] + [[0b11111] * 4 + [0]] * 65 + [[0b11111] * 5] * 4
    inits2 = (1, 1, 1, 3, 3)
    run2 = py_lattice(n, inits2, ho2, R)
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.LatticeAgreement(), n, R, [inits2], ho_array([ho2], n))
    assert_equal_to_restatement([run2], pi, dec, dr, fs, fr)
    assert s.term_hist[R + 1] == 1 and run2.rec[4][1] == -1 and s.live_instance_rounds == R
    # a late violation: the mutant's second quarter decides in round 65
    ho3 = [[0b00011, 0b00011, 0, 0, 0]] + [[0] * 5] * 64 + [[0, 0, 0b01100, 0b01100, 0]] + [[0] * 5] * 4
    inits3 = (1, 1, 2, 2, 2)
    run3 = py_lattice(n, inits3, ho3, R, variant=1)
    assert run3.first_fail == [66, 66, 66, NEVER, NEVER, NEVER]
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.LatticeAgreement(variant=1), n, R, [inits3], ho_array([ho3], n))
    assert_equal_to_restatement([run3], pi, dec, dr, fs, fr)


# ------------------------------------------------------------------------------------ 6. generic Spec
def spec_from_states(run):
    """spec_cases.lattice_custom's slots evaluated in Python from py_lattice's states."""
    ff, term = [NEVER] * 5, NEVER
    st = run.states
    for c, cur in enumerate(st):
        prev = st[c - 1] if c else None
        ok = [all(not d or dv == x for x, d, dv, _ in cur),
              all(cur[p][0] >= st[0][p][0] for p in range(run.n)),
              prev is None or all(not prev[p][1] or (cur[p][1] and cur[p][2] == prev[p][2]) for p in range(run.n)),
              all(hs > 2 * run.n // 3 for _, _, _, hs in cur),
              len({x for x, _, _, _ in cur}) == 1]
        for s in range(5):
            if not ok[s] and ff[s] == NEVER:
                ff[s] = c
        if term == NEVER and all(d for _, d, _, _ in cur):
            term = c
    return ff, term


@pytest.mark.parametrize("mode", ["vm", "native", "fused"])
@pytest.mark.parametrize("n", [8, 130])
def test_custom_spec_equals_the_restatement(n, mode):
    I, R = 24, 4
    rng = np.random.default_rng(n)
    ho = S.random_omission(rng, I, R, n, 0.7, True)
    ho[::3, 2:] = S.full_mask(n)
    ho[1::3, 0] = S.full_mask(n)
    v = rng.integers(0, 16, (I, n))
    inits = ((1 << (v // 4)) | (1 << (v % 4))).astype(np.int32)
    spec = spec_cases.lattice_custom()
    prog = F.compile_spec(spec, LATTICE) if mode == "vm" else F.compile_native(spec, LATTICE, fused=mode == "fused", n=n)
    with psync.GpuRound(psync.LatticeAgreement(), n, R, batch_capacity=I) as g:
        g._ctx.load_inputs(0, I, inits)
        g.load_schedule(0, I, ho)
        built = g.run(0, I, per_instance=True)
        sp = g.run_spec(0, I, prog, per_instance=True)
    runs = [py_lattice(n, inits[i], ho_ints(ho[i]), R) for i in range(I)]
    want = [spec_from_states(r) for r in runs]
    assert [(list(s.first_fail)[:5], s.term_round) for s in sp.per_instance] == want
    assert len({w[0][3] for w in want}) > 1 and all(w[0][:3] == [NEVER] * 3 for w in want)
    assert [s.digest for s in sp.per_instance] == [s.digest for s in built.per_instance]
    # the Spec's Irrevocability slot is the built-in slot 5; its Termination the built-in one
    assert [s.first_fail[2] for s in sp.per_instance] == [s.first_fail[5] for s in built.per_instance]
    assert [s.term_round for s in sp.per_instance] == [s.term_round for s in built.per_instance]


# ------------------------------------------------------------------------------------ 7. parameter rules
@pytest.mark.parametrize("U", [0, 32])
def test_create_rejects_value_range_outside_1_31(U):
    with pytest.raises(Exception, match="value_range"):
        psync.GpuRound(psync.LatticeAgreement(), 8, value_range=U, batch_capacity=4)


# ------------------------------------------------------------------------------------ 8. adversary
@pytest.mark.parametrize("n", [5, 6, 7])
def test_adversary_finds_shrinks_and_replays_the_mutant(n, tmp_path):
    alg, R = psync.LatticeAgreement(variant=1), 2
    with A.Adversary(alg, n=n, rounds=R, targets=["Comparability"], population=1024, values=3, seed=5) as adv:
        res = adv.search(generations=40, want=1)
        assert res.counterexamples, f"no counterexample in {res.schedules_evaluated} schedules"
        c = res.counterexamples[0]
        assert c.violated == ["Comparability"]
        missing = sum(1 for k in range(R) for p in range(n) for q in range(n)
                      if q != p and not (int(c.ho[k, p, q >> 6]) >> (q & 63)) & 1)
        assert c.omitted_links == missing
        path = str(tmp_path / "lattice.psgr")
        A.save(path, adv, res.counterexamples)
    back = records.read(path)
    assert back.class_name == "example.LatticeAgreement" and back.count == 1
    records.replay(path)  # raises unless the record's summaries are reproduced
    # the restatement agrees: the mutant breaks Comparability on this schedule, the reference does not
    ho = ho_ints(c.ho)
    assert py_lattice(n, c.init, ho, R, variant=1).first_fail[2] == c.check_point
    assert py_lattice(n, c.init, ho, R).first_fail == [NEVER] * 6


def test_adversary_reference_algorithm_holds():
    with A.Adversary(psync.LatticeAgreement(), n=6, rounds=2, population=1024, values=3, seed=5) as adv:
        res = adv.search(generations=40, want=1, shrink=False)
    assert not res.counterexamples and res.schedules_evaluated == 40 * 1024
