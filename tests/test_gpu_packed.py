"""Packed small-n mode on the GPU (psg_config.pack = 1): example.OTR at n <= 32 runs G = 64 / P
instances per wave64 (psg_otr_packed.hip). Everything is compared bit for bit with the CPU
oracle, which ignores `pack`, or with a pack = 0 context of the same config.

Seed 5 and BEGIN = 1000 unless a case says otherwise. Count 203 is 11 mod 16, 3 mod 8, 3 mod 4 and
1 mod 2: every G leaves idle sub-groups at the ends of the queue slices and of the batch."""
import ctypes as C

import numpy as np
import pytest

from round_amd import abi, formula as F, lib, psync

from gpu_support import (BEGIN, assert_run_equals_oracle, cmp_instances, cmp_summary, inst_tuple, random_schedule,
                         rec_tuple, spec_rows)
from restatement import M64

pytestmark = pytest.mark.gpu

H = psync.HOSchedule
SEED = 5
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def sample_of(count):
    """The first id, the last id and two inside."""
    return sorted({BEGIN, BEGIN + count // 3, BEGIN + (2 * count) // 3, BEGIN + count - 1})


def packed_vs_oracle(oracle_mod, alg, n, R, count, guard=None, **kw):
    """One pack = 1 run of [BEGIN, BEGIN + count) against the oracle's; guard(opi) first."""
    kw.setdefault("seed", SEED)
    with psync.GpuRound(alg, n, R, batch_capacity=count, pack=True, **kw) as gr:
        assert gr.cfg.pack == 1 and lib.pack_width(alg.alg_id, n) > 1
        osum, opi, orec = oracle_mod.run(gr.cfg, BEGIN, count, per_instance=True, records=True, threads=8)
        if guard:
            guard(opi)
        assert_run_equals_oracle(gr, count, osum, opi, orec, sample_of(count))
    return osum, opi, orec


# ------------------------------------------------------------------------------------ 1. every P and its edges
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32])
def test_parity_every_width(n, oracle_mod):
    packed_vs_oracle(oracle_mod, psync.OTR(), n, 20, 203)


@pytest.mark.parametrize("n", [4, 17])
@pytest.mark.parametrize("which", ["one", "G-1"])
def test_parity_fewer_rows_than_a_wave(n, which, oracle_mod):
    count = 1 if which == "one" else lib.pack_width(abi.PSG_ALG_OTR, n) - 1
    packed_vs_oracle(oracle_mod, psync.OTR(), n, 20, count)


# ------------------------------------------------------------------------------------ 2. schedule families
FAMILIES = {
    "crash": lambda n: (psync.OTR(), 20, 203, dict(schedule=H(drop_log2=2, good_round=0.25, crash_fmax=(n - 1) // 2))),
    "pure-ho": lambda n: (psync.OTR(afterDecision=1), 20, 203,
                          dict(schedule=H(drop_log2=1, good_round=0.1, self_bit=False), value_range=2)),
    "ho-min": lambda n: (psync.OTR(afterDecision=5), 70, 67,
                         dict(schedule=H(drop_log2=1, good_round=0.0, ho_min=(2 * n) // 3), value_range=100)),
    "lossless": lambda n: (psync.OTR(), 20, 203, dict(schedule=H(drop_log2=0, good_round=0.0))),
    "R1": lambda n: (psync.OTR(), 1, 203, dict()),
}


@pytest.mark.parametrize("n", [4, 5, 16, 32])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_parity_schedule_families(family, n, oracle_mod):
    alg, R, count, kw = FAMILIES[family](n)
    packed_vs_oracle(oracle_mod, alg, n, R, count, **kw)


@pytest.mark.parametrize("R", [70, 250])
def test_parity_long_runs(R, oracle_mod):
    """Good rounds past round 64 and first-fail bytes near the uint8 limit (n = 5, default schedule)."""
    packed_vs_oracle(oracle_mod, psync.OTR(), 5, R, 67)


# ------------------------------------------------------------------------------------ 3. mutant
@pytest.mark.parametrize("n", [3, 5, 7, 13, 17, 21])
def test_parity_mutant_fails_in_every_sub_group(n, oracle_mod):
    """Failing slots and the witness arms of the checks: Safety, Agreement and Irrevocability each
    fail in some instance at every row position i % G (guard, on the oracle's result)."""
    G = lib.pack_width(abi.PSG_ALG_OTR, n)

    def guard(opi):
        for slot in (0, 4, 7):
            pos = {i % G for i, s in enumerate(opi) if s.first_fail[slot] != abi.PSG_NEVER}
            assert pos == set(range(G)), (slot, sorted(pos))

    packed_vs_oracle(oracle_mod, psync.OTR(variant=1, afterDecision=3), n, 20, 1003, guard=guard,
                     schedule=H(drop_log2=2, good_round=0.0, self_bit=False), value_range=2)


# ------------------------------------------------------------------------------------ 4. host inputs
@pytest.mark.parametrize("n", [4, 7, 16, 32])
def test_parity_host_inputs_with_the_extremes(n, oracle_mod):
    count = 67
    extremes = np.array([INT32_MIN, INT32_MAX, -1, 0], np.int64)
    rng = np.random.default_rng(7)
    init = extremes[rng.integers(0, 4, (count, n))]
    for i in range(count):  # the four values, at four random positions of every row
        init[i, rng.permutation(n)[:4]] = extremes
    init = init.astype(np.int32)
    with psync.GpuRound(psync.OTR(), n, 20, seed=9, batch_capacity=count, pack=True) as gr:
        osum, opi, orec = oracle_mod.run(gr.cfg, BEGIN, count, init=[[int(v) for v in row] for row in init],
                                         per_instance=True, records=True, threads=8)
        decided = {r.decision for r in orec if r.decision_round >= 0}
        assert len(decided) >= 2 and INT32_MIN in decided, decided
        gr.load_inputs(BEGIN, count, init)
        res = gr.run(BEGIN, count, per_instance=True)
        dec, dround = gr.decisions()
    cmp_summary(res.summary, osum, 20)
    cmp_instances(res.per_instance, opi)
    assert dec == [r.decision for r in orec]
    assert dround == [r.decision_round for r in orec]


# ------------------------------------------------------------------------------------ 5. packed == unpacked
def summary_list(s):
    return abi.summary_to_list(s)[:-1]  # (all but kernel_ns)


def test_packed_equals_unpacked_and_its_parts():
    n, count = 4, 5003
    out = []
    for pack in (False, True):
        with psync.GpuRound(psync.OTR(), n, 20, seed=SEED, batch_capacity=count, pack=pack) as gr:
            ctx = gr._ctx
            s, pi = ctx.run_batch_np(BEGIN, count)
            dec, dr = ctx.copy_decisions_np()
            out.append((summary_list(s), pi.tobytes(), dec.tobytes(), dr.tobytes()))
            if pack:
                parts = [ctx.run_batch_np(BEGIN, 101), ctx.run_batch_np(BEGIN + 101, count - 101)]
                assert np.concatenate([p[1] for p in parts]).tobytes() == pi.tobytes()
                assert sum(p[0].digest for p in parts) & M64 == s.digest & M64
                a, b = (summary_list(p[0]) for p in parts)
                whole = summary_list(s)
                di = 4 + abi.PSG_MAX_CHECKS + 1  # the digest: a sum mod 2^64, compared above
                assert whole[di] == s.digest
                assert [x + y for j, (x, y) in enumerate(zip(a, b)) if j != di] == \
                       [x for j, x in enumerate(whole) if j != di]
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------ 6. the rest of a packed context
def test_other_calls_of_a_packed_context_are_unchanged():
    n, R, count = 5, 10, 37
    alg = psync.OTR()
    prog = F.compile_spec(F.REFERENCE_SPECS[alg.alg_id](), alg.alg_id)
    k = len(prog.slot_names)
    rng = np.random.default_rng(11)
    ho, _ = random_schedule(rng, alg, n, R, count, "omission")
    init = rng.integers(1, 5, (count, n), dtype=np.int32)
    ids = [BEGIN, BEGIN + 7, BEGIN + 18, BEGIN + 29, BEGIN + count - 1]
    out = []
    for pack in (False, True):
        with psync.GpuRound(alg, n, R, seed=SEED, batch_capacity=count, pack=pack) as gr:
            sp = gr.run_spec(BEGIN, count, prog, per_instance=True)
            mho, mcr = gr.materialize_schedule(BEGIN, count)
            fs, fr = gr.fetch(ids)
            gr.load_inputs(BEGIN, count, init)
            gr.load_schedule(BEGIN, count, ho)
            xs = gr.run(BEGIN, count, per_instance=True)
            xdec = gr.decisions()
            out.append((spec_rows(sp.per_instance, k, digest=True), summary_list(sp.summary), mho.tobytes(), mcr.tobytes(),
                        [inst_tuple(s) for s in fs], [rec_tuple(r) for r in fr],
                        summary_list(xs.summary), [inst_tuple(s) for s in xs.per_instance], xdec))
    assert out[0] == out[1]


def test_packed_device_list_equals_one_packed_context():
    n, count = 7, 201
    out = []
    for devices in (None, [0, 0]):
        with psync.GpuRound(psync.OTR(), n, 20, seed=SEED, batch_capacity=count, devices=devices, pack=True) as gr:
            r = gr.run(BEGIN, count, per_instance=True)
            out.append((summary_list(r.summary), [inst_tuple(s) for s in r.per_instance], gr.decisions()))
    assert out[0] == out[1]


def test_create_rejects_other_pack_values():
    L = lib.load()
    cfg = psync.make_config(psync.OTR(), 4, batch_capacity=16)
    cfg.pack = 2
    h = C.c_void_p()
    assert L.psg_create(C.byref(h), C.byref(cfg)) == abi.PSG_EINVAL
    assert h.value is None
    assert L.psg_create_error().decode() == "pack must be 0 or 1"


@pytest.mark.parametrize("alg,n", [(psync.LastVoting(), 5), (psync.OTR(), 40)], ids=["lv-n5", "otr-n40"])
def test_pack_changes_nothing_without_a_packed_kernel(alg, n):
    assert lib.pack_width(alg.alg_id, n) == 1
    count = 203
    out = []
    for pack in (False, True):
        with psync.GpuRound(alg, n, seed=SEED, batch_capacity=count, pack=pack) as gr:
            r = gr.run(BEGIN, count, per_instance=True)
            out.append((summary_list(r.summary), [inst_tuple(s) for s in r.per_instance], gr.decisions()))
    assert out[0] == out[1]
