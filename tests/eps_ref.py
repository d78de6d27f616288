"""Plain references for the wave primitives of the EpsilonConsensus kernel (psg_epsilon.hip), and
the seeded inputs their device self-tests run on (psg_selftest_eps_*). Nothing here touches the
GPU: tests/test_eps_ref.py pins these helpers by hand, tests/test_gpu_eps_primitives.py compares
the device with them on the same data."""
import math
import random
import struct

import numpy as np

M64 = (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
SIGN = 1 << 63
CANONICAL_NAN = 0x7FF8000000000000
DBL_MAX = 1.7976931348623157e308
POWER_BASES = (2, 3, 5, 6, 7, 10)
LOG_EPS = tuple(10.0 ** -e for e in range(1, 16)) + (1e-300,)


# ---------------------------------------------------------------------------------- bit patterns
def bits(x):
    """The 64 bits of a double as an unsigned integer."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b & M64))[0]


def bits_of(xs):
    """uint64 bit patterns of a sequence of doubles (payloads of NaNs kept)."""
    return np.array([bits(x) for x in xs], np.uint64)


# ---------------------------------------------------------------------------------- Double.compare
def java_key(x):
    """java.lang.Double.compare as an integer order: sign and magnitude, -0.0 below 0.0, every NaN
    one value above +inf."""
    if x != x:
        return CANONICAL_NAN
    b = bits(x)
    mag = b & (SIGN - 1)
    return -mag - 1 if b & SIGN else mag


def key_to_double(k):
    """The non-NaN double whose java_key is k."""
    return from_bits(k if k >= 0 else SIGN | (-k - 1))


def java_d2i(x):
    """Java's narrowing (int) of a double: NaN -> 0, saturating, else toward zero."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return INT32_MAX
    if x <= -2147483648.0:
        return INT32_MIN
    return int(x)


def fold32(x):
    """The 32-bit fold of a double's bits the digests use (low ^ high word), as a signed int."""
    b = bits(x)
    v = (b ^ (b >> 32)) & 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def sorted_pairs(xs, n):
    """(value, pid) of the first n processes in Double.compare order, ties by pid."""
    return [(xs[p], p) for p in sorted(range(n), key=lambda p: (java_key(xs[p]), p))]


def needs_pair_sort(xs, n):
    """Whether the one-word sort (top 58 key bits, then pid) leaves the list out of (key, pid) order:
    two keys agree in their top 58 bits and stand against their pid order."""
    ks = [java_key(xs[p]) for p in range(n)]
    return any(ks[p] >> 6 == ks[q] >> 6 and ks[p] > ks[q] for p in range(n) for q in range(p + 1, n))


# ---------------------------------------------------------------------------------- bit matrices
def transpose(rows):
    """64 x 64 bit-matrix transpose: rows[i] bit j -> result[j] bit i."""
    a = np.unpackbits(np.array([int(r) for r in rows], "<u8").view(np.uint8).reshape(64, 8), axis=1, bitorder="little")
    t = np.ascontiguousarray(np.packbits(np.ascontiguousarray(a.T), axis=1, bitorder="little"))
    return [int(r) for r in t.view("<u8").reshape(64)]


def select(m, j):
    """Position of the j-th set bit of m (0-based), -1 when m has no more than j bits."""
    for b in range(64):
        if (m >> b) & 1:
            if j == 0:
                return b
            j -= 1
    return -1


def select_row(m):
    """select(m, j) for j = 0 .. 63 in one pass (what the device self-test returns per mask)."""
    pos = [b for b in range(64) if (m >> b) & 1]
    return pos + [-1] * (64 - len(pos))


def us(U, spid):
    """Sorted-membership masks: result[p] bit t = the process at sorted position t is in U[p]."""
    return [sum(((int(U[p]) >> int(spid[t])) & 1) << t for t in range(64)) for p in range(64)]


# ---------------------------------------------------------------------------------- reductions
def red_min(v, flag, n):
    return min([int(v[p]) for p in range(n) if flag[p]], default=INT64_MAX)


def red_max(v, flag, n):
    return max([int(v[p]) for p in range(n) if flag[p]], default=INT64_MIN)


def red_sum(v, n):
    """Sum of the first n values mod 2**64, as a signed 64-bit integer (Grp::sum64 takes no flag)."""
    s = sum(int(v[p]) for p in range(n)) & M64
    return s - (1 << 64) if s >> 63 else s


# ---------------------------------------------------------------------------------- log
def _mp():
    import mpmath
    mpmath.mp.prec = 256
    return mpmath


def log_ref(x):
    """log(x) from mpmath at 256 bits, rounded once to double; IEEE results at the edges."""
    if x != x or x < 0.0:
        return math.nan
    if x == 0.0:
        return -math.inf
    if x == math.inf:
        return math.inf
    mp = _mp()
    return float(mp.log(mp.mpf(x)))


def ulp_diff(a, b):
    """Doubles between a and b in the ordered line of non-NaN doubles (0 when the bits agree;
    -0.0 and 0.0 count as one)."""
    if a != a or b != b:
        return 0 if (a != a and b != b) else M64
    ka, kb = java_key(a), java_key(b)
    ka += 1 if ka < 0 else 0  # -0.0 and 0.0 are the same point
    kb += 1 if kb < 0 else 0
    return abs(ka - kb)


def exact_powers():
    """(c, k), k >= 1, for the bases of POWER_BASES while c**k is below 2**53 (an integer every
    double arithmetic step holds exactly)."""
    out = []
    for c in POWER_BASES:
        k = 1
        while c ** k < 2 ** 53:
            out.append((c, k))
            k += 1
    return out


def log_inputs(seed=1):
    """The positive finite inputs of the log comparison, without repeats."""
    rng = random.Random(seed)
    xs = [from_bits(1), from_bits(0x000FFFFFFFFFFFFF), from_bits(0x0010000000000000)]
    xs += [from_bits(0x3FEFFFFFFFFFFFFF), 1.0, from_bits(0x3FF0000000000001)]
    for d in (-2, -1, 0, 1, 2):  # the 2/3 mantissa split of the range reduction
        for e in (-1022, -1, 0, 1, 1023):
            xs.append(math.ldexp(from_bits(0x3FE5555555555555 + d), e))
    xs += [math.ldexp(1.0, k) for k in range(-1074, 1024)]
    xs += [float(c ** k) for c, k in exact_powers()]
    xs.append(DBL_MAX)
    for _ in range(4096):
        while True:
            b = rng.getrandbits(63)
            if b and (b >> 52) != 0x7FF:
                break
        xs.append(from_bits(b))
    for i in range(4096):
        span = 0.0
        while span == 0.0:
            span = rng.random()
        xs.append(span / LOG_EPS[i % len(LOG_EPS)])
    seen, out = set(), []
    for x in xs:
        if bits(x) not in seen:
            seen.add(bits(x))
            out.append(x)
    return out


def log_specials():
    """(x, kind) with kind in "+inf", "-inf", "nan": what log must return outside (0, inf)."""
    nans = [from_bits(b) for b in (CANONICAL_NAN, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,
                                   0x7FFFFFFFFFFFFFFF)]
    neg = [-1.0, -from_bits(1), -DBL_MAX, -0.5, -math.inf]
    return ([(math.inf, "+inf"), (0.0, "-inf"), (-0.0, "-inf")] + [(x, "nan") for x in neg] + [(x, "nan") for x in nans])


def maxr_ref(q, c):
    """(ceil(log(q) / log(c)), distance of the quotient from the nearest integer) from mpmath."""
    mp = _mp()
    r1 = mp.log(mp.mpf(q)) / mp.log(mp.mpf(c))
    return int(mp.ceil(r1)), float(abs(r1 - mp.nint(r1)))


MAXR_MARGIN = 1e-9


def maxr_inputs(seed=2, count=4096):
    """count pairs (q, c, ceil(r1)) with r1 = log(q) / log(c) farther than MAXR_MARGIN from an integer
    (q = span / eps as the kernel forms it, c an integer >= 2), and the number of draws discarded."""
    rng = random.Random(seed)
    out, dropped = [], 0
    while len(out) < count:
        span = rng.random() * rng.choice((1.0, 1.0, 1e-3, 1e3))
        if span == 0.0:
            continue
        q = span / rng.choice(LOG_EPS)
        c = float(rng.choice((2, 2, 3, 3, 5, 5, 4, 6, 7, 10, rng.randrange(2, 65))))
        want, dist = maxr_ref(q, c)
        if dist <= MAXR_MARGIN:
            dropped += 1
            continue
        out.append((q, c, want))
    return out, dropped


# ---------------------------------------------------------------------------------- keys and d2i
def edge_doubles():
    """About 300 doubles at the edges of the key order and of the int narrowing."""
    pats = [0, 1, 2, 3, 0x000FFFFFFFFFFFFE, 0x000FFFFFFFFFFFFF]
    for e in (1, 2, 3, 0x100, 0x200, 0x300, 0x3E0, 0x3FC, 0x3FD, 0x3FE, 0x3FF, 0x400, 0x401, 0x402, 0x410, 0x41C,
              0x41D, 0x41E, 0x41F, 0x420, 0x421, 0x431, 0x432, 0x433, 0x434, 0x435, 0x43E, 0x43F, 0x500, 0x600, 0x700,
              0x7FD, 0x7FE):
        pats += [(e << 52) - 1, e << 52, (e << 52) + 1, (e << 52) | 0x000FFFFFFFFFFFFE]
    pats += [0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000]
    # NaNs: signalling (quiet bit clear) and quiet, low and high payloads
    pats += [0x7FF0000000000001, 0x7FF0000000000002, 0x7FF4000000000000, 0x7FF7FFFFFFFFFFFF, CANONICAL_NAN,
             0x7FF8000000000001, 0x7FF800000000003F, 0x7FF8000000000040, 0x7FFFFFFFFFFFFFFF, 0x7FF00000FFFFFFFF]
    xs = [from_bits(p) for p in pats] + [from_bits(SIGN | p) for p in pats]
    for m in (2147483648.0, 2147483647.0):
        for d in (0.0, 0.5, 1.0):
            xs += [m + d, m - d, -(m + d), -(m - d)]
    xs += [2147483647.5, -2147483648.5, -0.9, 0.9, 0.5, -0.5, 1.5, -1.5, 1e10, -1e10, 1e300, -1e300, 4294967296.0,
           -4294967296.0, 4294967295.0, 2147483646.9999998, -2147483648.0000005]
    seen, out = set(), []
    for x in xs:
        if bits(x) not in seen:
            seen.add(bits(x))
            out.append(x)
    return out


# ---------------------------------------------------------------------------------- sort
SORT_N = (1, 2, 3, 31, 32, 33, 63, 64)
SORT_STEPS = (1, 7, 63, 64, 65)


def sort_cases(seed=3):
    """(name, xs[64], n): the first n values are the processes', the rest stand in padding lanes
    and must not show."""
    rng = random.Random(seed)
    neg_nans = [from_bits(b) for b in (0xFFF8000000000000, 0xFFF0000000000001, 0xFFFFFFFFFFFFFFFF,
                                       0x7FF0000000000001, 0x7FF800000000002A)]

    def rnd():
        return rng.choice((rng.uniform(-5, 5), rng.random(), -rng.random() * 1e-300, from_bits(rng.getrandbits(64))))

    def ladder(base_key, step, n, descending):
        ks = [base_key + i * step for i in range(n)]
        return [key_to_double(k) for k in (reversed(ks) if descending else ks)]

    cases = []
    for n in SORT_N:
        fam = {
            "random": [rnd() for _ in range(n)],
            "equal": [rng.uniform(-3, 3)] * n,
            "all-nan": [math.nan] * n,
            "half-nan": [math.nan if p % 2 == 0 else rnd() for p in range(n)],
            "zeros": [rng.choice((0.0, -0.0)) for _ in range(n)],
            "zeros-mixed": [rng.choice((0.0, -0.0, from_bits(1), -from_bits(1), 1.0)) for _ in range(n)],
            "inf-max": [rng.choice((math.inf, DBL_MAX, -math.inf, -DBL_MAX, rnd())) for _ in range(n)],
            "neg-nan": [rng.choice(neg_nans + [rnd(), math.inf]) for _ in range(n)],
        }
        for step in SORT_STEPS:
            for side, base in (("pos", java_key(rng.uniform(0.1, 4.0))), ("neg", java_key(-rng.uniform(0.1, 4.0))),
                               ("zero", -(n // 2) * step - step // 2)):
                fam[f"desc-{step}-{side}"] = ladder(base, step, n, True)
                fam[f"asc-{step}-{side}"] = ladder(base, step, n, False)
        for name, xs in fam.items():
            pad = [rng.choice((-math.inf, -DBL_MAX, 0.0, math.nan, rnd())) for _ in range(64 - n)]
            cases.append((f"{name}-n{n}", list(xs) + pad, n))
    return cases


# ---------------------------------------------------------------------------------- transpose
def transpose_cases(seed=4):
    """Lists of 64 rows: the identity, single rows and columns, permutations, single bits around the
    block boundaries of every stage, random matrices at three densities."""
    rng = random.Random(seed)
    ms = [[1 << i for i in range(64)]]
    ms += [[M64 if i == r else 0 for i in range(64)] for r in range(64)]
    ms += [[1 << c for _ in range(64)] for c in range(64)]
    for _ in range(64):
        perm = list(range(64))
        rng.shuffle(perm)
        ms.append([1 << perm[i] for i in range(64)])
    for i in (0, 1, 2, 4, 8, 16, 32, 63):
        for j in (0, 3, 7, 15, 16, 31, 32, 63):
            ms.append([(1 << j) if r == i else 0 for r in range(64)])
    for t in range(128):
        d = (0.05, 0.5, 0.95)[t % 3]
        ms.append([sum((rng.random() < d) << j for j in range(64)) for _ in range(64)])
    return ms


# ---------------------------------------------------------------------------------- rank select
def select_masks(seed=5):
    rng = random.Random(seed)

    def pick(lo, hi):  # lo bits in the low half, hi in the high half
        return (sum(1 << b for b in rng.sample(range(32), lo)) | sum(1 << (32 + b) for b in rng.sample(range(32), hi)))

    ms = [1 << b for b in range(64)] + [M64] + [0xFF << (8 * b) for b in range(8)]
    ms += [0x0101010101010101, 0x8080808080808080, sum(1 << (8 * b + rng.randrange(8)) for b in range(8))]
    ms += [0xFFFFFFFF00000000, 0x00000000FFFFFFFF, pick(0, 13), pick(13, 0), pick(0, 1), pick(1, 0)]
    ms += [pick(32, 0), pick(31, 0), pick(32, 1), pick(16, 16), pick(16, 15), pick(15, 16), pick(17, 16), pick(16, 17),
           pick(31, 1), pick(1, 31), pick(1, 32), pick(0, 32), pick(32, 31), pick(31, 32)]
    for _ in range(2000):
        d = rng.choice((0.03, 0.2, 0.5, 0.8, 0.97))
        m = 0
        while m == 0:
            m = sum((rng.random() < d) << b for b in range(64))
        ms.append(m)
    return ms


# ---------------------------------------------------------------------------------- Us
US_N = (7, 33, 64)


def us_cases(seed=6, count=200):
    """(U[64], spid[64], n): U of a padding lane is 0 and no U holds a padding process; spid lists
    the n processes in a random order, then the padding lanes (they sort last)."""
    rng = random.Random(seed)
    cases = []
    for i in range(count):
        n = US_N[i % len(US_N)]
        d = rng.choice((0.1, 0.5, 0.9, 1.0))
        U = [sum((rng.random() < d) << q for q in range(n)) if p < n else 0 for p in range(64)]
        head, tail = list(range(n)), list(range(n, 64))
        rng.shuffle(head)
        rng.shuffle(tail)
        cases.append((U, head + tail, n))
    return cases


# ---------------------------------------------------------------------------------- reductions
REDUCE_SHAPES = ((1, 64), (1, 40), (2, 128), (2, 100), (4, 256), (4, 193))


def reduce_cases(W, n, seed=7):
    """Cases of three data sets (v int64 [64W], flag uint8 [64W]) each: the device calls every
    reduction once per set, back to back. Padding lanes carry extreme values that must not show."""
    rng = random.Random(seed * 1000 + n)
    T = 64 * W
    special = [INT64_MIN, INT64_MAX, java_key(-0.0), java_key(0.0), -1, 0, 1, java_key(math.inf), java_key(-math.inf)]

    def values(kind):
        if kind == "random":
            v = [rng.getrandbits(64) - (1 << 63) for _ in range(T)]
        elif kind == "special":
            v = [rng.choice(special) for _ in range(T)]
        else:  # keys of small doubles around zero
            v = [java_key(rng.choice((0.0, -0.0, 1e-300, -1e-300, 0.5))) for _ in range(T)]
        for p in range(n, T):
            v[p] = rng.choice((INT64_MIN, INT64_MAX))
        return v

    def flags(kind):
        if kind == "empty":
            return [0] * T
        if kind == "all":
            return [1] * T
        if kind == "last-wave-one":
            f = [0] * T
            f[rng.randrange(64 * (W - 1), n)] = 1
            return f
        if kind == "padding-only":
            return [1 if p >= n else 0 for p in range(T)]
        if kind == "one-per-wave":
            f = [0] * T
            for w in range(W):
                f[rng.randrange(64 * w, min(n, 64 * w + 64))] = 1
            return f
        return [1 if rng.random() < 0.5 else 0 for _ in range(T)]

    fk = ["random", "all", "empty", "last-wave-one", "padding-only", "one-per-wave"]
    vk = ["random", "special", "zeros"]
    cases = []
    for i in range(24):
        cases.append([(values(vk[(i + s) % 3]), flags(fk[(i // 3 + 2 * s) % len(fk)])) for s in range(3)])
    return cases
