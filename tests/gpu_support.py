"""What the GPU test modules share: the comparison of a GPU run with the oracle's (or with a
restatement's, tests/restatement.py), the runners several modules drive, and their seeded and
explicit inputs. Nothing here runs on import; the CPU-side guard tests import it too."""
import ctypes as C
import math

import numpy as np

from round_amd import abi, psync, schedules as S

from restatement import M64, digest_of, ho_ints, py_tpc

BEGIN = 1000  # non-zero instance ids


# ------------------------------------------------------------------------------------ comparisons
def cmp_summary(g, o, rounds):
    assert g.instances == o.instances
    assert g.process_rounds == o.process_rounds
    assert (g.active_process_rounds, g.live_instance_rounds) == (o.active_process_rounds, o.live_instance_rounds)
    assert list(g.fail_count) == list(o.fail_count)
    assert g.decided_processes == o.decided_processes
    assert g.digest == o.digest
    assert list(g.term_hist)[: rounds + 2] == list(o.term_hist)[: rounds + 2]


def inst_tuple(s):
    """A per-instance summary (psg_instance_summary), every one of the PSG_MAX_CHECKS slots."""
    return (s.digest, tuple(s.first_fail), s.term_round, s.n_checks, s.n_decided)


def np_inst_tuple(a):
    """inst_tuple of a records.SUMMARY_DTYPE row."""
    return (int(a["digest"]), tuple(int(v) for v in a["first_fail"]), int(a["term_round"]), int(a["n_checks"]),
            int(a["n_decided"]))


def rec_tuple(r):
    return (r.decision, r.decision_round, r.halt_round, r.final_x)


def cmp_instances(gpu_pi, opi):
    """Per-instance summaries of a GPU run (structs, or a SUMMARY_DTYPE array) against the oracle's."""
    row = np_inst_tuple if isinstance(gpu_pi, np.ndarray) else inst_tuple
    mism = [i for i in range(len(opi)) if row(gpu_pi[i]) != inst_tuple(opi[i])]
    assert not mism, f"{len(mism)} instance summaries differ, first {mism[:5]}: " \
                     f"{row(gpu_pi[mism[0]])} != {inst_tuple(opi[mism[0]])}"


def spec_rows(pi, k, digest=False):
    """(first_fail[:k], term_round) per instance of a Spec run, with the digest on request."""
    return [(tuple(s.first_fail)[:k], s.term_round) + ((s.digest,) if digest else ()) for s in pi]


# EpsilonConsensus (Double) values: every step is the same IEEE operation in the same order on
# both sides, so the GPU reproduces the oracle bit for bit; the stated tolerance covers libm log()
# differing by an ulp (which can move maxR only when r1 sits within an ulp of an integer). Integer
# results (rounds, first failing check points) must match exactly.
F64_ABS_TOL = 1e-12


def close(a, b, tol=F64_ABS_TOL):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= tol


def check_eps(gr, res, dec, dround, begin, count, init=None, oracle_mod=None):
    n = gr.cfg.n
    osum, opi, orec, odec, ofx = oracle_mod.run_real(gr.cfg, begin, count, init=init, per_instance=True,
                                                     records=True, threads=8)
    cmp_summary(res.summary, osum, gr.cfg.rounds)
    for i in range(count):
        g, o = res.per_instance[i], opi[i]
        assert (tuple(g.first_fail), g.term_round, g.n_decided) == (tuple(o.first_fail), o.term_round, o.n_decided), i
        assert g.digest == o.digest, i
    for c in range(count * n):
        assert dround[c] == orec[c].decision_round, c
        assert close(dec[c], odec[c]), (c, dec[c], odec[c])
    return opi, orec, odec, ofx


# ------------------------------------------------------------------------------------ against the oracle
def assert_run_equals_oracle(gr, count, osum, opi, orec, sample):
    """One GPU run of [BEGIN, BEGIN + count) against the oracle's results."""
    n = gr.cfg.n
    res = gr.run(BEGIN, count, per_instance=True)
    dec, dround = gr.decisions()
    fsums, frecs = gr.fetch(sample)
    cmp_summary(res.summary, osum, gr.cfg.rounds)
    cmp_instances(res.per_instance, opi)
    odec = np.array([(r.decision, r.decision_round) for r in orec], np.int64)
    bad = np.nonzero((np.array(dec, np.int64) != odec[:, 0]) | (np.array(dround, np.int64) != odec[:, 1]))[0]
    assert bad.size == 0, f"decisions differ, first (instance, process) {divmod(int(bad[0]), n)}"
    for j, inst in enumerate(sample):
        i = inst - BEGIN
        assert inst_tuple(fsums[j]) == inst_tuple(opi[i]), inst
        for p in range(n):
            assert rec_tuple(frecs[j * n + p]) == rec_tuple(orec[i * n + p]), (inst, p)
    return res


def run_any(gr, oracle_mod, count, sample):
    """One GPU run against a fresh oracle run of the same config (integer or Double algorithm)."""
    n = gr.cfg.n
    if not gr.alg.real:
        osum, opi, orec = oracle_mod.run(gr.cfg, BEGIN, count, per_instance=True, records=True, threads=8)
        assert_run_equals_oracle(gr, count, osum, opi, orec, sample)
        return opi, orec
    res = gr.run(BEGIN, count, per_instance=True)
    dec, dround = gr.decisions()
    fsums, frecs, fdec, ffx = gr.fetch_real(sample)
    opi, orec, odec, ofx = check_eps(gr, res, dec, dround, BEGIN, count, oracle_mod=oracle_mod)
    assert [inst_tuple(s) for s in res.per_instance] == [inst_tuple(s) for s in opi]
    as_bits = lambda xs: np.array(xs, np.float64).view(np.uint64)  # noqa: E731
    assert (as_bits(dec) == as_bits(odec)).all()
    for j, inst in enumerate(sample):
        i = inst - BEGIN
        assert inst_tuple(fsums[j]) == inst_tuple(opi[i]), inst
        assert ([rec_tuple(r) for r in frecs[j * n:(j + 1) * n]]
                == [rec_tuple(r) for r in orec[i * n:(i + 1) * n]]), inst
        assert (as_bits(fdec[j * n:(j + 1) * n]) == as_bits(odec[i * n:(i + 1) * n])).all(), inst
        assert (as_bits(ffx[j * n:(j + 1) * n]) == as_bits(ofx[i * n:(i + 1) * n])).all(), inst
    return opi, orec


def otr_alg(name, **kw):
    return (psync.OTR2 if name == "otr2" else psync.OTR)(**kw)


# ------------------------------------------------------------------------------------ explicit inputs
def random_schedule(rng, alg, n, R, I, family):
    """HO sets [I][R][n][W] of a family ("crash": crash-stop with a little loss on top, else random
    omission, repaired to the algorithm's safety predicate) and the crash rounds, or None."""
    if family == "crash":
        fmax = max(1, alg.param)
        crash, partial = S.random_crash(rng, I, R, n, fmax, p_partial=(0.1, 0.5, 0.9))
        ho = S.crash_to_ho(crash, partial, R, n)
        # a little benign loss on top, so explicit sets are not crash patterns only
        ho &= ~(S.random_bits(rng, ho.shape, 1 / 64) & ~S.self_mask(n)[None, None])
        return ho, crash
    ho = S.random_omission(rng, I, R, n, 0.8)
    if alg.alg_id == abi.PSG_ALG_BENOR:
        S.repair_min_size(ho, rng, n, n // 2 + 1)
    if alg.alg_id == abi.PSG_ALG_EPSILON:
        S.repair_min_size(ho, rng, n, n - alg.param)
    return ho, None


def random_init(rng, alg, I, n, V):
    if alg.real:
        return rng.random((I, n))
    if alg.alg_id == abi.PSG_ALG_BENOR:
        return rng.integers(0, 2, (I, n), dtype=np.int32)
    return rng.integers(1, V + 1, (I, n), dtype=np.int32)


# ------------------------------------------------------------------------------------ against a restatement
def gpu_explicit(alg, n, R, inits, ho, **kw):
    """Run explicit schedules; returns (summary, per-instance summaries, decision, decision_round,
    fetched summaries, fetched process records)."""
    I = len(inits)
    with psync.GpuRound(alg, n, R, batch_capacity=I, **kw) as g:
        ctx = g._ctx
        ctx.load_inputs(0, I, np.asarray(inits, np.int32))
        ctx.load_schedule(0, I, ho, None)
        s, pi = ctx.run_batch_np(0, I)
        dec, dr = ctx.copy_decisions_np()
        fs, fr = ctx.fetch_np(np.arange(I, dtype=np.uint64))
    return s, pi, dec, dr, fs, fr


def assert_equal_to_restatement(runs, pi, dec, dr, fs, fr):
    """GPU results against py_tpc / py_lattice runs; the run's first_fail has the algorithm's slots."""
    for i, run in enumerate(runs):
        k = len(run.first_fail)
        assert [int(x) for x in dec[i]] == [r[0] for r in run.rec], i
        assert [int(x) for x in dr[i]] == [r[1] for r in run.rec], i
        assert [int(x) for x in fr[i]["halt_round"]] == [r[2] for r in run.rec], i
        assert [int(x) for x in fr[i]["decision"]] == [r[0] for r in run.rec], i
        assert [int(x) for x in fr[i]["decision_round"]] == [r[1] for r in run.rec], i
        assert [int(x) for x in fr[i]["final_x"]] == [r[3] for r in run.rec], i
        for s in (pi[i], fs[i]):
            assert [int(x) for x in s["first_fail"][:k]] == run.first_fail, i
            assert (int(s["term_round"]), int(s["n_decided"]), int(s["n_checks"])) == (run.term_round, run.n_decided, k), i
            assert int(s["digest"]) == digest_of(run), i


def schedule_cfg(cfg):
    """The config under an algorithm the oracle library has: the schedule generator reads n, R,
    the seed and the schedule parameters only (as seeded_votes does for the init words)."""
    c = abi.Config()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(abi.Config))
    c.alg, c.param = abi.PSG_ALG_OTR, 2
    return c


def seeded_votes(cfg, oracle_mod, begin, count):
    """TwoPhaseCommit: canCommit = (1 + mulhi32(w, V)) != 1 with the init word of every other
    algorithm: the oracle's init value for the same seed and value_range under OTR's rule."""
    c = schedule_cfg(cfg)
    return np.array([[int(oracle_mod.init_value(c, begin + i, p) != 1) for p in range(cfg.n)] for i in range(count)],
                    np.int32)


def seeded_inits(cfg, oracle_mod, begin, count):
    """LatticeAgreement: lattice_init(w, U) is a function of OTR's init value at value_range U * U:
    that value is 1 + mulhi32(w, U * U) with the same init word, so v = value - 1, elements v / U
    and v % U."""
    U = cfg.value_range
    c = schedule_cfg(cfg)
    c.value_range = U * U
    v = np.array([[oracle_mod.init_value(c, begin + i, p) - 1 for p in range(cfg.n)] for i in range(count)], np.int64)
    assert v.min() >= 0 and v.max() < U * U
    return ((1 << (v // U)) | (1 << (v % U))).astype(np.int32)


def tpc_seeded(n, R, coord, sched, cnt, seed, oracle_mod):
    """A seeded TwoPhaseCommit run == py_tpc on the schedule the library exports, and that schedule
    == the oracle's restatement of the generator. Returns (runs, crash rounds)."""
    alg = psync.TwoPhaseCommit(coord=coord)
    with psync.GpuRound(alg, n, R, seed=seed, schedule=sched, batch_capacity=cnt) as g:
        ctx = g._ctx
        ho, cr = g.materialize_schedule(BEGIN, cnt)
        s, pi = ctx.run_batch_np(BEGIN, cnt)
        dec, dr = ctx.copy_decisions_np()
        fs, fr = ctx.fetch_np(np.arange(BEGIN, BEGIN + cnt, dtype=np.uint64))
        votes = seeded_votes(g.cfg, oracle_mod, BEGIN, cnt)
    oho, ocr = oracle_mod.materialize_schedule(schedule_cfg(g.cfg), BEGIN, cnt)
    assert (ho == oho).all() and (cr == ocr).all()
    runs = [py_tpc(n, coord, votes[i], ho_ints(ho[i]), R) for i in range(cnt)]
    assert_equal_to_restatement(runs, pi, dec, dr, fs, fr)
    assert s.decided_processes == sum(r.n_decided for r in runs)
    assert s.digest & M64 == sum(digest_of(r) for r in runs) & M64
    hist = [0] * (R + 2)
    for r in runs:
        hist[R + 1 if r.term_round == abi.PSG_NEVER else r.term_round] += 1
    assert [s.term_hist[c] for c in range(R + 2)] == hist
    return runs, cr


def sharding_and_fetch(alg, n, cnt):
    """One range == its two halves, and fetched instances == the batch's. Returns the fetched
    process records, for the caller's algorithm-specific check of halt_round."""
    begin = 500
    with psync.GpuRound(alg, n, rounds=4, seed=8, batch_capacity=cnt) as g:
        ctx = g._ctx
        s, pi = ctx.run_batch_np(begin, cnt)
        dec, dr = ctx.copy_decisions_np()
        a = cnt // 2
        parts = [ctx.run_batch_np(begin, a), ctx.run_batch_np(begin + a, cnt - a)] if a else [ctx.run_batch_np(begin, cnt)]
        assert np.concatenate([p[1] for p in parts]).tobytes() == pi.tobytes()
        assert sum(p[0].digest for p in parts) & M64 == s.digest & M64
        assert sum(p[0].decided_processes for p in parts) == s.decided_processes
        ids = np.array(sorted({begin + (7 * j) % cnt for j in range(min(cnt, 9))}, reverse=True), np.uint64)
        fs, fr = ctx.fetch_np(ids)
    for j, i in enumerate(int(x) - begin for x in ids):
        assert fs[j].tobytes() == pi[i].tobytes()
        assert (fr[j]["decision"] == dec[i]).all() and (fr[j]["decision_round"] == dr[i]).all()
    return fr


def assert_multi_device_equals_one_device(alg):
    """A device-list context ([0, 0]: two per-device contexts on the one card) gives the single
    context's summary, per-instance summaries, decisions and fetched records."""
    n, cnt, begin = 130, 201, 77
    out = []
    for devices in (None, [0, 0]):
        with psync.GpuRound(alg, n, seed=6, batch_capacity=cnt, devices=devices) as g:
            r = g.run(begin, cnt, per_instance=True)
            f = g.fetch([begin, begin + 100, begin + cnt - 1])
            out.append((abi.summary_to_list(r.summary)[:-1],
                        [(s.digest, tuple(s.first_fail), s.term_round, s.n_decided) for s in r.per_instance],
                        g.decisions(), [s.digest for s in f[0]],
                        [(x.decision, x.decision_round, x.halt_round, x.final_x) for x in f[1]]))
    assert out[0] == out[1]
