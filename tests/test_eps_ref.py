"""Hand-written known answers for tests/eps_ref.py, the references the device self-tests of the
EpsilonConsensus primitives are compared with (tests/test_gpu_eps_primitives.py), and the sizes
of the seeded inputs. No GPU."""
import math

import numpy as np

import eps_ref as E

INF, NAN = math.inf, math.nan
TINY = 5e-324  # the smallest denormal


def test_java_key_orders_a_hand_written_list():
    """Double.compare's order, written out: ascending, with the NaNs equal and last."""
    ordered = [-INF, -E.DBL_MAX, -1.5, -1.0, -2.2250738585072014e-308, -TINY, -0.0, 0.0, TINY,
               2.2250738585072014e-308, 0.5, 1.0, 1.0000000000000002, 2.0, 1e300, E.DBL_MAX, INF]
    keys = [E.java_key(x) for x in ordered]
    assert all(a < b for a, b in zip(keys, keys[1:])), keys
    nans = [NAN, -NAN, E.from_bits(0x7FF0000000000001), E.from_bits(0xFFF0000000000001), E.from_bits(0xFFFFFFFFFFFFFFFF)]
    assert len({E.java_key(x) for x in nans}) == 1 and E.java_key(NAN) > E.java_key(INF)
    assert (E.java_key(-0.0), E.java_key(0.0), E.java_key(TINY), E.java_key(-TINY)) == (-1, 0, 1, -2)
    assert E.java_key(1.0) == 0x3FF0000000000000 and E.java_key(-INF) == -0x7FF0000000000000 - 1
    for x in ordered:
        assert E.bits(E.key_to_double(E.java_key(x))) == E.bits(x)


def test_java_d2i_known_answers():
    kat = [(NAN, 0), (INF, E.INT32_MAX), (-INF, E.INT32_MIN), (2147483648.0, E.INT32_MAX), (-2147483648.0, E.INT32_MIN),
           (2147483647.5, E.INT32_MAX), (-2147483648.5, E.INT32_MIN), (2147483647.0, 2147483647),
           (2147483646.5, 2147483646), (-2147483647.5, -2147483647), (-0.9, 0), (0.9, 0), (TINY, 0), (-TINY, 0),
           (-0.0, 0), (1.5, 1), (-1.5, -1), (1e300, E.INT32_MAX), (-1e300, E.INT32_MIN)]
    for x, want in kat:
        assert E.java_d2i(x) == want, x


def test_sorted_pairs_and_fallback_rule():
    xs = [1.0, NAN, -0.0, 0.0, 1.0, -INF, 7.0, 9.0]
    assert [p for _, p in E.sorted_pairs(xs, 7)] == [5, 2, 3, 0, 4, 6, 1]
    assert [p for _, p in E.sorted_pairs([NAN, -NAN, 2.0], 3)] == [2, 0, 1]
    one = E.from_bits(0x3FF0000000000001)
    assert E.needs_pair_sort([one, 1.0], 2) and not E.needs_pair_sort([1.0, one], 2)
    assert not E.needs_pair_sort([one, 1.0], 1)
    assert not E.needs_pair_sort([E.from_bits(0x3FF0000000000040), 1.0], 2)  # top 58 bits differ
    assert E.needs_pair_sort([-1.0, -one], 2) and not E.needs_pair_sort([-one, -1.0], 2)
    assert not E.needs_pair_sort([NAN, -NAN], 2)
    # -0.0 and 0.0 have keys -1 and 0: they differ in every bit, so the one-word sort orders them
    assert (E.java_key(-0.0) >> 6, E.java_key(0.0) >> 6) == (-1, 0) and not E.needs_pair_sort([0.0, -0.0], 2)
    assert E.needs_pair_sort([TINY, 0.0], 2)


def test_transpose_select_us():
    rows = [0] * 64
    rows[3] = 1 << 60 | 1 << 2
    t = E.transpose(rows)
    assert t[60] == 1 << 3 and t[2] == 1 << 3 and sum(map(bool, t)) == 2
    m = 0b1011_0000_0001
    assert [E.select(m, j) for j in range(5)] == [0, 8, 9, 11, -1]
    assert E.select(1 << 63, 0) == 63 and E.select(E.M64, 40) == 40
    for mask in (m, 1 << 63, E.M64, 0x8000000100000001):
        assert E.select_row(mask) == [E.select(mask, j) for j in range(64)]
    dense = [0x0123456789ABCDEF ^ (i * 0x9E3779B97F4A7C15 & E.M64) for i in range(64)]
    assert E.transpose(E.transpose(dense)) == dense
    assert all((E.transpose(dense)[j] >> i) & 1 == (dense[i] >> j) & 1 for i in range(64) for j in range(64))
    spid = list(reversed(range(64)))
    U = [0] * 64
    U[5] = 1 << 63 | 1 << 1
    assert E.us(U, spid)[5] == 1 << 0 | 1 << 62 and E.us(U, spid)[4] == 0


def test_reductions():
    v = [5, -7, E.INT64_MIN, E.INT64_MAX]
    assert E.red_min(v, [1, 1, 0, 0], 4) == -7 and E.red_max(v, [1, 1, 0, 0], 4) == 5
    assert E.red_min(v, [0, 0, 1, 1], 2) == E.INT64_MAX and E.red_max(v, [0] * 4, 4) == E.INT64_MIN
    assert E.red_sum(v, 4) == 5 - 7 - 1 and E.red_sum([E.INT64_MAX, 1], 2) == E.INT64_MIN


def test_log_ref_known_answers():
    import mpmath
    assert E.log_ref(1.0) == 0.0 and E.bits(E.log_ref(1.0)) == 0
    mpmath.mp.prec = 300
    for k in (-1074, -1022, -1, 1, 2, 10, 52, 1023):
        assert E.log_ref(math.ldexp(1.0, k)) == float(k * mpmath.ln2), k
    assert E.log_ref(0.0) == -INF and E.log_ref(-0.0) == -INF and E.log_ref(INF) == INF
    assert math.isnan(E.log_ref(-1.0)) and math.isnan(E.log_ref(NAN)) and math.isnan(E.log_ref(-INF))
    assert E.log_ref(math.e) == 1.0  # (the double nearest e: its log rounds to 1)


def test_ulp_diff():
    assert E.ulp_diff(1.0, 1.0) == 0 and E.ulp_diff(1.0, E.from_bits(0x3FF0000000000001)) == 1
    assert E.ulp_diff(0.0, -0.0) == 0 and E.ulp_diff(TINY, -TINY) == 2 and E.ulp_diff(NAN, NAN) == 0
    assert E.ulp_diff(NAN, 1.0) > 1 << 60


def test_input_builders_respect_their_caps():
    xs = E.log_inputs()
    assert 8192 < len(xs) <= 1 << 14
    assert all(0.0 < x < INF for x in xs) and len({E.bits(x) for x in xs}) == len(xs)
    assert xs == E.log_inputs()  # deterministic
    pw = E.exact_powers()
    assert (5, 3) in pw and (2, 52) in pw and (3, 33) in pw and (3, 34) not in pw and (10, 15) in pw
    assert len(pw) == 52 + 33 + 22 + 20 + 18 + 15 and all(int(float(c ** k)) == c ** k for c, k in pw)
    kinds = {k for _, k in E.log_specials()}
    assert kinds == {"+inf", "-inf", "nan"}
    edge = E.edge_doubles()
    assert 250 <= len(edge) <= 350
    assert sum(x != x for x in edge) >= 16 and sum(x != x and E.bits(x) >> 63 for x in edge) >= 8
    assert len(E.select_masks()) > 2000 and all(0 < m <= E.M64 for m in E.select_masks())
    assert len(E.transpose_cases()) == 1 + 64 + 64 + 64 + 64 + 128
    assert len(E.us_cases()) == 200
    for U, spid, n in E.us_cases():
        assert sorted(spid) == list(range(64)) and all(p < n for p in spid[:n])
        assert all(u >> n == 0 for u in U) and all(u == 0 for u in U[n:])


def test_maxr_builder_discards_at_most_one_percent():
    pairs, dropped = E.maxr_inputs()
    assert len(pairs) == 4096 and dropped <= 0.01 * (4096 + dropped), dropped
    # one-ulp errors of both logs move r1 <= 2**11 by far less than the margin
    assert 2 ** 11 * 4 * 2.0 ** -52 < E.MAXR_MARGIN / 100
    assert all(abs(w) <= 2 ** 11 for _, _, w in pairs)
    assert E.maxr_ref(6.0, 2.0)[0] == 3 and E.maxr_ref(0.3, 3.0)[0] == -1


def test_sort_cases_cover_the_families():
    cases = E.sort_cases()
    assert {n for _, _, n in cases} == set(E.SORT_N)
    assert all(len(xs) == 64 for _, xs, _ in cases)
    by = {name: (xs, n) for name, xs, n in cases}
    for step in E.SORT_STEPS:
        for side in ("pos", "neg", "zero"):
            xs, n = by[f"desc-{step}-{side}-n64"]
            ks = [E.java_key(x) for x in xs]
            assert all(a - b == step for a, b in zip(ks, ks[1:]))
            # descending by pid: the fallback is needed exactly when neighbours can share their top 58 bits
            assert E.needs_pair_sort(xs, n) == any(a >> 6 == b >> 6 for a, b in zip(ks, ks[1:]))
            assert E.needs_pair_sort(xs, n) or step >= 63
            assert not E.needs_pair_sort(by[f"asc-{step}-{side}-n64"][0], 64)
        ks = [E.java_key(x) for x in by[f"desc-{step}-zero-n64"][0]]
        assert ks[0] > 0 > ks[-1]
    assert E.needs_pair_sort(*by["desc-1-pos-n2"]) and not E.needs_pair_sort(*by["desc-1-pos-n1"])
    xs, n = by["half-nan-n33"]
    assert sum(x != x for x in xs[:n]) >= 17


def test_reduce_cases_shapes():
    for W, n in E.REDUCE_SHAPES:
        cases = E.reduce_cases(W, n)
        assert len(cases) == 24 and all(len(c) == 3 for c in cases)
        sets = [s for c in cases for s in c]
        assert all(len(v) == 64 * W and len(f) == 64 * W for v, f in sets)
        assert any(not any(f) for _, f in sets)                                   # empty
        assert any(sum(f) == 1 and any(f[64 * (W - 1):n]) for _, f in sets)       # one lane of the last wave
        if n < 64 * W:
            assert any(any(f) and not any(f[:n]) for _, f in sets)                # padding lanes only
        assert np.array([v for v, _ in sets], np.int64).shape == (72, 64 * W)
