"""The wave primitives of the EpsilonConsensus kernel (psg_epsilon.hip), each run alone on the
device through its self-test entry point (psg_selftest_eps_*) and compared with the plain
references of tests/eps_ref.py on inputs the whole-algorithm parity runs never form: denormals and
the 2/3 mantissa split for log, NaNs with the sign bit set, keys a few ulp apart against pid order,
member masks with exactly 32 bits in one half, single-bit matrices at every block boundary of the
transpose, and span / eps at an exact power of c, where maxR hangs on the last bit of two logs.

The W = 1 sort sequence, the sel8 table loop, the Us transposes and the maxR expression stand
inline in the round kernel; the self-tests run statement-for-statement copies of them (sharing
them as functions cost the round kernel 0.5 %), and test_integer_r1_end_to_end and the parity
tests of test_gpu_parity.py tie the inline text to the copies.

Measured on an MI355X (the figures the assertions below bound):
  log_ocml and the device library's log agree bit for bit on all 10 425 inputs; the largest
  error of either against mpmath's log rounded once to double is 1 ulp (e.g. at
  0x1.5555555555555p+0). At the 160 exact powers c**k < 2**53 the device gives maxR = k + 1 at
  17, the same 17 as glibc's log on the test host (the list is in DESIGN.md)."""
import math

import numpy as np
import pytest

from round_amd import lib, psync

import eps_ref as E

pytestmark = pytest.mark.gpu


def f64_run(xs):
    return lib.selftest_eps_f64(E.bits_of(xs))


def as_bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------- log
@pytest.fixture(scope="module")
def log_run():
    xs = E.log_inputs()
    return xs, f64_run(xs), [E.log_ref(x) for x in xs]


def test_log_ocml_is_the_device_library_log_bit_for_bit(log_run):
    xs, out, _ = log_run
    bad = np.nonzero(as_bits(out["log_ocml"]) != as_bits(out["log"]))[0]
    print(f"log: {len(xs)} inputs compared")
    assert bad.size == 0, [(xs[i].hex(), out["log_ocml"][i].hex(), out["log"][i].hex()) for i in bad[:5]]
    sp = E.log_specials()
    so = f64_run([x for x, _ in sp])
    for i, (x, kind) in enumerate(sp):
        for name in ("log_ocml", "log"):
            y = float(so[name][i])
            ok = math.isnan(y) if kind == "nan" else y == (math.inf if kind == "+inf" else -math.inf)
            assert ok, (name, E.bits(x), y, kind)


def test_log_within_one_ulp_of_mpmath(log_run):
    xs, out, ref = log_run
    worst = {}
    for name in ("log_ocml", "log"):
        d = [E.ulp_diff(float(y), r) for y, r in zip(out[name], ref)]
        w = max(range(len(xs)), key=d.__getitem__)
        worst[name] = (d[w], xs[w].hex())
    print(f"log: max ulp error against mpmath over {len(xs)} inputs: {worst}")
    assert worst["log"][0] <= 1, worst      # the library's own error (the kernel header's bound)
    assert worst["log_ocml"][0] <= 1, worst


# ---------------------------------------------------------------------------------- maxr
def maxr_of_powers():
    pw = E.exact_powers()
    got = lib.selftest_eps_maxr([float(c ** k) for c, k in pw], [float(c) for c, _ in pw])
    return pw, [int(v) for v in got]


def test_maxr_at_exact_powers_is_k_or_k_plus_one():
    pw, got = maxr_of_powers()
    bad = [(c, k, g) for (c, k), g in zip(pw, got) if g not in (k, k + 1)]
    assert not bad, bad[:10]
    dev = [(c, k) for (c, k), g in zip(pw, got) if g == k + 1]
    host = [(c, k) for c, k in pw if math.ceil(math.log(float(c ** k)) / math.log(float(c))) == k + 1]
    print(f"maxr: {len(pw)} exact powers; k + 1 on the device at {len(dev)}: {dev}")
    print(f"maxr: k + 1 under the host's libm at {len(host)}: {host}")


def test_maxr_away_from_integers_is_exact():
    pairs, _ = E.maxr_inputs()
    got = lib.selftest_eps_maxr([q for q, _, _ in pairs], [c for _, c, _ in pairs])
    bad = [(q.hex(), c, int(g), w) for (q, c, w), g in zip(pairs, got) if int(g) != w]
    print(f"maxr: {len(pairs)} pairs compared")
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------------- end to end
def oracle_rows(oracle_mod, cfg, count, ho, init):
    osum, opi, orec, odec, _ = oracle_mod.run_schedule(cfg, 0, count, ho, None, init, per_instance=True, records=True)
    return osum, opi, orec, odec


@pytest.mark.parametrize("n,f,c", [(7, 1, 2), (16, 2, 3), (64, 5, 5)])
def test_integer_r1_end_to_end(n, f, c, oracle_mod):
    """span / eps = c**k exactly (eps = 1, inputs 0.0 and c**k, every HO set full): every process
    decides in round maxR + 1 with maxR the self-test's value for (c**k, c) — the kernel's inline
    expression is the tested one — and decides the 2f-th smallest input bit for bit. Where the
    oracle's libm gives the same maxR the whole run equals the oracle's; else they differ by exactly
    one round (the documented tolerance)."""
    I = 24
    rng = np.random.default_rng(100 + n)
    ks = list(range(1, 13))
    maxr = [int(v) for v in lib.selftest_eps_maxr([float(c ** k) for k in ks], [float(c)] * len(ks))]
    differ = []
    for k, mr in zip(ks, maxr):
        assert mr in (k, k + 1), (k, mr)
        R = k + 3
        top = float(c ** k)
        init = np.where(rng.random((I, n)) < rng.choice([0.2, 0.5, 0.8], (I, 1)), top, 0.0)
        for i in range(I):  # both values in every instance, so span = c**k
            init[i, rng.choice(n, 2, replace=False)] = (top, 0.0)
        assert ((init == top).any(axis=1) & (init == 0.0).any(axis=1)).all()
        ho = np.full((I, R, n, 1), (1 << n) - 1, np.uint64)
        with psync.GpuRound(psync.EpsilonConsensus(f, 1.0), n, R, batch_capacity=I) as g:
            ctx = g._ctx
            ctx.load_inputs(0, I, init)
            ctx.load_schedule(0, I, ho, None)
            s, pi = ctx.run_batch_np(0, I)
            dec, dr = ctx.copy_decisions_np()
        assert (dr == mr + 1).all(), (k, mr, np.unique(dr))
        want = np.sort(init, axis=1)[:, 2 * f]
        assert (as_bits(dec) == as_bits(np.repeat(want[:, None], n, axis=1))).all(), k
        osum, opi, orec, odec = oracle_rows(oracle_mod, g.cfg, I, ho, init)
        odr = np.array([r.decision_round for r in orec]).reshape(I, n)
        if (odr == dr).all():
            assert list(s.fail_count) == list(osum.fail_count) and s.digest == osum.digest
            assert s.decided_processes == osum.decided_processes
            for i in range(I):
                assert (int(pi[i]["digest"]), tuple(int(v) for v in pi[i]["first_fail"]), int(pi[i]["term_round"]),
                        int(pi[i]["n_decided"])) == (opi[i].digest, tuple(opi[i].first_fail), opi[i].term_round,
                                                     opi[i].n_decided), (k, i)
            assert (as_bits(dec) == as_bits(odec.reshape(I, n))).all()
        else:
            assert (np.abs(odr - dr) == 1).all() and len(np.unique(odr)) == 1, (k, np.unique(odr), np.unique(dr))
            assert (as_bits(dec) == as_bits(odec.reshape(I, n))).all()
            differ.append((c, k, mr, int(odr[0, 0]) - 1))
    print(f"end to end n = {n}, c = {c}: maxR per k {dict(zip(ks, maxr))}; device and oracle one round apart at "
          f"(c, k, device, oracle) {differ}")


# ---------------------------------------------------------------------------------- keys and d2i
def test_total_key_orders_like_double_compare():
    xs = E.edge_doubles()
    out = f64_run(xs)
    dk = out["key"]
    jk = np.array([E.java_key(x) for x in xs], np.int64)
    print(f"keys: {len(xs)} doubles, {len(xs) ** 2} pairs compared")
    assert ((dk[:, None] < dk[None, :]) == (jk[:, None] < jk[None, :])).all()
    assert ((dk[:, None] == dk[None, :]) == (jk[:, None] == jk[None, :])).all()
    back = as_bits(out["key_value"])
    for i, x in enumerate(xs):
        if x != x:
            assert int(dk[i]) == E.CANONICAL_NAN and int(back[i]) == E.CANONICAL_NAN, hex(E.bits(x))
        else:
            assert int(back[i]) == E.bits(x), hex(E.bits(x))
    assert (dk == jk).all()  # the reference key is the same integer


def test_d2i_and_fold():
    xs = E.edge_doubles()
    out = f64_run(xs)

    def ceil_of(x):
        return x if (x != x or abs(x) >= 2.0 ** 52) else float(math.ceil(x))

    for i, x in enumerate(xs):
        assert int(out["d2i"][i]) == E.java_d2i(x), x.hex()
        assert int(out["d2i_ceil"][i]) == E.java_d2i(ceil_of(x)), x.hex()
        assert int(out["fold32"][i]) == E.fold32(x), x.hex()
    print(f"d2i: {len(xs)} doubles compared")


# ---------------------------------------------------------------------------------- sort
@pytest.mark.parametrize("network", [0, 1], ids=["kernel-sequence", "key-pid-network"])
def test_wave_sort_equals_sorted_pairs(network):
    cases = E.sort_cases()
    xb = np.array([E.bits_of(xs) for _, xs, _ in cases])
    ns = [n for _, _, n in cases]
    vals, pid, fell = lib.selftest_eps_sort(xb, ns, network=network)
    n_fell = 0
    for i, (name, xs, n) in enumerate(cases):
        want = E.sorted_pairs(xs, n)
        assert [int(p) for p in pid[i, :n]] == [p for _, p in want], name
        assert [int(b) for b in vals[i, :n]] == [E.bits(v) for v, _ in want], name
        assert sorted(int(p) for p in pid[i, n:]) == list(range(n, 64)), name  # padding lanes sort last
        need = E.needs_pair_sort(xs, n)
        assert int(fell[i]) == (1 if need and network == 0 else 0), (name, int(fell[i]), need)
        n_fell += need
    print(f"sort: {len(cases)} cases compared, {n_fell} of them need the (key, pid) network")
    assert n_fell >= 50 and n_fell <= len(cases) - 50


# ---------------------------------------------------------------------------------- transpose
def test_wave_transpose64():
    ms = E.transpose_cases()
    rows = np.array(ms, np.uint64)
    got = lib.selftest_eps_transpose(rows)
    for i, m in enumerate(ms):
        assert [int(v) for v in got[i]] == E.transpose(m), i
    assert (lib.selftest_eps_transpose(got) == rows).all()
    print(f"transpose: {len(ms)} matrices compared, and their double transposes")


# ---------------------------------------------------------------------------------- rank select
def test_rank_select():
    ms = E.select_masks()
    got = lib.selftest_eps_select(np.array(ms, np.uint64))
    for i, m in enumerate(ms):
        assert [int(v) for v in got[i]] == E.select_row(m), hex(m)
    print(f"rank select: {len(ms)} masks, {sum(bin(m).count('1') for m in ms)} positions compared")
    with pytest.raises(lib.PsgError):
        lib.selftest_eps_select(np.array([1, 0], np.uint64))


# ---------------------------------------------------------------------------------- Us
def test_sorted_membership_mask():
    cases = E.us_cases()
    got = lib.selftest_eps_members(np.array([U for U, _, _ in cases], np.uint64), [s for _, s, _ in cases])
    for i, (U, spid, n) in enumerate(cases):
        assert [int(v) for v in got[i]] == E.us(U, spid), (i, n)
    print(f"Us: {len(cases)} cases compared")


# ---------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("W,n", E.REDUCE_SHAPES, ids=[f"W{W}-n{n}" for W, n in E.REDUCE_SHAPES])
def test_group_reductions(W, n):
    cases = E.reduce_cases(W, n)
    v = np.array([[s[0] for s in c] for c in cases], np.int64)
    fl = np.array([[s[1] for s in c] for c in cases], np.uint8)
    got = lib.selftest_eps_reduce(W, n, v, fl)
    for i, c in enumerate(cases):
        want = ([E.red_min(sv, sf, n) for sv, sf in c] + [E.red_max(sv, sf, n) for sv, sf in c]
                + [E.red_sum(sv, n) for sv, _ in c])
        for w in range(W):  # every wave holds the group's result
            assert [int(x) for x in got[i, :, w]] == want, (i, w)
    print(f"reductions W = {W}, n = {n}: {len(cases)} cases x 9 results x {W} waves compared")
