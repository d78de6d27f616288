"""GPU: TwoPhaseCommit (psg_tpc.hip) against the pure-Python restatement of the reference.

The oracle library has no TwoPhaseCommit, so the reference side is `py_tpc`
(tests/restatement.py, written from example/TwoPhaseCommit.scala). Explicit and seeded
schedules, hand KATs, sharding and fetch, the generic Spec in its three forms, the adversary.
"""
import functools

import numpy as np
import pytest

from round_amd import abi, adversary as A, formula as F, psync, records, schedules as S

from gpu_support import (assert_equal_to_restatement, assert_multi_device_equals_one_device, gpu_explicit, seeded_votes,
                         sharding_and_fetch, spec_rows)
from restatement import (M64, NEVER, NONE32, TPC_KAT_IDS, TPC_KATS, digest_of, ho_array, ho_ints, py_tpc,
                         tpc_kat_coord_crashed_from_round2, tpc_kat_mutant_n5, tpc_outcomes)

pytestmark = pytest.mark.gpu
TPC = abi.PSG_ALG_TPC


# ------------------------------------------------------------------------------------ 1. explicit schedules
def _cases():
    """n x coord in {0, n/2, n-1} (another wave / mask word than most lanes) x R x self_bit, trimmed:
    per (n, coord) one case at R = 3 and one at another R, with alternating self_bit."""
    out = []
    Rs = [1, 2, 4, 7, 3]
    for a, n in enumerate([1, 2, 3, 5, 8, 63, 64, 65, 128, 130, 256]):
        for b, coord in enumerate(sorted({0, n // 2, n - 1})):
            out.append((n, coord, 3, (a + b) % 2 == 0))
            out.append((n, coord, Rs[(a + b) % 5], (a + b) % 2 == 1))
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def _explicit_inputs(n, coord, R, self_bit):
    """64 instances: random omission (keep 0.98 for n <= 8, 255/256 for n >= 63), P(no vote) =
    0.5 / n, and the restatement's runs. For n >= 3 and R >= 3 the instances hold all three
    outcomes (checked on the restatement): the seed is the first of a fixed sequence that does."""
    keep = 0.98 if n <= 8 else 255 / 256
    for salt in range(40):
        rng = np.random.default_rng([n, coord, R, int(self_bit), salt])
        ho = S.random_omission(rng, 64, R, n, keep, self_bit)
        votes = (rng.random((64, n)) >= 0.5 / n).astype(np.int32)
        runs = [py_tpc(n, coord, votes[i], ho_ints(ho[i]), R) for i in range(64)]
        if n < 3 or R < 3 or tpc_outcomes(runs) == {"commit", "abort", "suspect"}:
            return ho, votes, runs
    raise AssertionError("no seed of the sequence gives all three outcomes")


@pytest.mark.parametrize("n,coord,R,self_bit", _cases())
def test_explicit_schedules_equal_the_restatement(n, coord, R, self_bit):
    ho, votes, runs = _explicit_inputs(n, coord, R, self_bit)
    if n >= 3 and R >= 3:
        assert tpc_outcomes(runs) == {"commit", "abort", "suspect"}
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.TwoPhaseCommit(coord=coord), n, R, votes, ho)
    assert_equal_to_restatement(runs, pi, dec, dr, fs, fr)
    assert s.decided_processes == sum(r.n_decided for r in runs)
    assert list(s.fail_count)[:4] == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------ 2. hand KATs
@pytest.mark.parametrize("kat,recs,ff,term,nd", TPC_KATS, ids=TPC_KAT_IDS)
def test_hand_kats_on_the_gpu(kat, recs, ff, term, nd):
    n, coord, votes, ho, R = kat()
    run = py_tpc(n, coord, votes, ho, R)
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.TwoPhaseCommit(coord=coord), n, R, [votes], ho_array([ho], n))
    assert [(int(dec[0][p]), int(dr[0][p]), int(fr[0][p]["halt_round"])) for p in range(n)] == recs
    assert ([int(x) for x in pi[0]["first_fail"][:4]], int(pi[0]["term_round"]), int(pi[0]["n_decided"])) == (ff, term, nd)
    assert_equal_to_restatement([run], pi, dec, dr, fs, fr)


def test_mutant_kat_on_the_gpu():
    """A no-voter's slot-1 link to the coordinator is dropped: the mutant commits, Validity and
    Safety first fail at check point 2; the reference algorithm aborts with no violation."""
    n, coord, votes, ho, R = tpc_kat_mutant_n5()
    hoa = ho_array([ho], n)
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.TwoPhaseCommit(coord=coord, variant=1), n, R, [votes], hoa)
    assert [int(x) for x in pi[0]["first_fail"][:4]] == [2, 2, NEVER, 2]
    assert [int(x) for x in dec[0]] == [1] * n
    assert list(s.fail_count)[:4] == [1, 1, 0, 1]
    assert_equal_to_restatement([py_tpc(n, coord, votes, ho, R, mutant=True)], pi, dec, dr, fs, fr)
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.TwoPhaseCommit(coord=coord), n, R, [votes], hoa)
    assert [int(x) for x in pi[0]["first_fail"][:4]] == [NEVER] * 4 and [int(x) for x in dec[0]] == [0] * n


def test_crashed_coordinator_is_suspected():
    n, coord, votes, ho, R = tpc_kat_coord_crashed_from_round2()
    s, pi, dec, dr, fs, fr = gpu_explicit(psync.TwoPhaseCommit(coord=coord), n, R, [votes], ho_array([ho], n))
    assert [int(x) for x in dec[0][1:]] == [NONE32] * (n - 1) and [int(x) for x in dr[0][1:]] == [-1] * (n - 1)
    assert int(pi[0]["n_decided"]) == 1 and int(pi[0]["term_round"]) == NEVER


# ------------------------------------------------------------------------------------ 3. seeded schedules
@pytest.mark.parametrize("n", [5, 64, 100, 256])
def test_seeded_run_equals_the_restatement_on_its_materialized_schedule(n, oracle_mod):
    cnt, begin = 96, 1000
    alg = psync.TwoPhaseCommit(coord=n // 3)
    with psync.GpuRound(alg, n, seed=21, batch_capacity=cnt) as g:
        cfg = g.cfg
        ctx = g._ctx
        ho, cr = g.materialize_schedule(begin, cnt)
        s, pi = ctx.run_batch_np(begin, cnt)
        dec, dr = ctx.copy_decisions_np()
        fs, fr = ctx.fetch_np(np.arange(begin, begin + cnt, dtype=np.uint64))
        votes = seeded_votes(cfg, oracle_mod, begin, cnt)
        runs = [py_tpc(n, alg.param, votes[i], ho_ints(ho[i]), cfg.rounds) for i in range(cnt)]
        assert_equal_to_restatement(runs, pi, dec, dr, fs, fr)
        assert (cr == -1).all()
        # the summary counters
        assert (s.instances, s.process_rounds) == (cnt, cnt * n * 3)
        assert (s.active_process_rounds, s.live_instance_rounds) == (cnt * n * 3, cnt * 3)
        assert s.decided_processes == sum(r.n_decided for r in runs)
        assert list(s.fail_count)[:4] == [0] * 4
        assert s.digest & M64 == sum(digest_of(r) for r in runs) & M64
        hist = [0] * 5
        for r in runs:
            hist[4 if r.term_round == NEVER else r.term_round] += 1
        assert [s.term_hist[c] for c in range(5)] == hist
        # replay through psg_load_schedule: the same run bit for bit
        ctx.load_inputs(begin, cnt, votes)
        ctx.load_schedule(begin, cnt, ho, None)
        s2, pi2 = ctx.run_batch_np(begin, cnt)
        assert s2.digest == s.digest and pi2.tobytes() == pi.tobytes()
    if n == 64:  # default value_range 2n: both outcomes are common
        assert 0 < sum(1 for r in runs if r.rec[alg.param][0] == 1) < cnt


# ------------------------------------------------------------------------------------ 4. sharding and fetch
@pytest.mark.parametrize("n,cnt", [(64, 1), (64, 3), (5, 5), (64, 200), (130, 50)])
def test_sharding_and_fetch_equal_one_range(n, cnt):
    for rec in sharding_and_fetch(psync.TwoPhaseCommit(), n, cnt):
        assert (rec["halt_round"] == 2).all()


def test_multi_device_context_equals_one_device():
    assert_multi_device_equals_one_device(psync.TwoPhaseCommit(coord=129))


# ------------------------------------------------------------------------------------ 5. generic Spec
def _spec_inputs(n):
    """The mutant schedule of the KAT at size n (a no-voter's slot-1 link to the coordinator is
    dropped) beside random omission: failing and passing slots."""
    rng = np.random.default_rng(n)
    I, R, coord = 40, 4, n - 2
    ho = S.random_omission(rng, I, R, n, 0.98 if n <= 8 else 255 / 256, True)
    votes = (rng.random((I, n)) >= 0.5 / n).astype(np.int32)
    fm = S.full_mask(n)
    for i in range(0, I, 4):
        q = (3 * i + 1) % n if (3 * i + 1) % n != coord else 0
        votes[i] = 1
        votes[i, q] = 0
        ho[i, 1, coord] = fm
        ho[i, 1, coord, q >> 6] &= ~np.uint64(1 << (q & 63))
    return I, R, coord, ho, votes


@pytest.mark.parametrize("mode", ["vm", "native", "fused"])
@pytest.mark.parametrize("n", [8, 130])
def test_reference_spec_equals_the_builtin_checks(n, mode):
    I, R, coord, ho, votes = _spec_inputs(n)
    spec = F.REFERENCE_SPECS[TPC]()
    prog = F.compile_spec(spec, TPC) if mode == "vm" else F.compile_native(spec, TPC, fused=mode == "fused", n=n)
    with psync.GpuRound(psync.TwoPhaseCommit(coord=coord, variant=1), n, R, batch_capacity=I) as g:
        g._ctx.load_inputs(0, I, votes)
        g.load_schedule(0, I, ho)
        built = g.run(0, I, per_instance=True)
        sp = g.run_spec(0, I, prog, per_instance=True)
    built_rows = spec_rows(built.per_instance, 4, digest=True)
    assert spec_rows(sp.per_instance, 4, digest=True) == built_rows
    assert list(sp.summary.fail_count)[:4] == list(built.summary.fail_count)[:4]
    assert built.summary.fail_count[3] >= I // 4 and built.summary.fail_count[2] == 0
    runs = [py_tpc(n, coord, votes[i], ho_ints(ho[i]), R, mutant=True) for i in range(I)]
    assert [(tuple(r.first_fail), r.term_round) for r in runs] == [x[:2] for x in built_rows]


# ------------------------------------------------------------------------------------ 6. adversary
def test_adversary_finds_shrinks_and_replays_the_mutant(tmp_path):
    alg, n, R = psync.TwoPhaseCommit(variant=1), 8, 3
    with A.Adversary(alg, n=n, rounds=R, targets=["Validity"], population=1024, seed=5) as adv:
        res = adv.search(generations=60, want=1)
        assert res.counterexamples, f"no counterexample in {res.schedules_evaluated} schedules"
        c = res.counterexamples[0]
        assert c.violated == ["Validity"] and c.check_point == 2
        # shrunk: no omitted link can be restored without losing the violation
        cands = []
        for k in range(R):
            for p in range(n):
                for q in range(n):
                    if not (int(c.ho[k, p, q >> 6]) >> (q & 63)) & 1:
                        h = c.ho.copy()
                        h[k, p, q >> 6] |= np.uint64(1 << (q & 63))
                        cands.append(h)
        assert cands and len(cands) == c.omitted_links
        e = adv.evaluator(c.inst_id, np.stack(cands), None, np.repeat(c.init[None], len(cands), 0))
        assert not adv._violations(e)[0].any()
        path = str(tmp_path / "tpc.psgr")
        A.save(path, adv, res.counterexamples)
    back = records.read(path)
    assert back.class_name == "example.TwoPhaseCommit" and back.count == 1
    records.replay(path)  # raises unless the record's summaries are reproduced
    # the restatement agrees: the mutant violates Validity on this schedule, the reference does not
    ho = ho_ints(c.ho)
    assert py_tpc(n, 0, c.init, ho, R, mutant=True).first_fail[3] == 2
    assert py_tpc(n, 0, c.init, ho, R).first_fail == [NEVER] * 4


def test_adversary_reference_algorithm_holds():
    with A.Adversary(psync.TwoPhaseCommit(), n=8, rounds=3, population=1024, seed=5) as adv:
        res = adv.search(generations=60, want=1, shrink=False)
    assert not res.counterexamples and res.schedules_evaluated == 60 * 1024
