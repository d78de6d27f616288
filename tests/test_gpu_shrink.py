"""Shrinking on the device (psg_shrink_*, psg_population_links): the candidate lists against
tests/shrink_ref.py (pinned to Adversary.shrink by tests/test_shrink_rule.py), adoption, the crash
level, the loaded state, the error table, and Adversary.shrink_device == Adversary.shrink."""
import numpy as np
import pytest

from round_amd import abi, adversary as A, lib, psync, schedules as S

from shrink_ref import candidates, same_cex

pytestmark = pytest.mark.gpu

TAIL, ROUND, SET, LINK, CRASH = (abi.PSG_SHRINK_TAIL, abi.PSG_SHRINK_ROUND, abi.PSG_SHRINK_SET, abi.PSG_SHRINK_LINK,
                                 abi.PSG_SHRINK_CRASH)
CAP = 64  # batch_capacity of the enumeration tests


def _base(n, R, keep=0.8, seed=0):
    """A random base with bits >= n clear and the self bit set, and initial values."""
    rng = np.random.default_rng(1000 * n + R + seed)
    return S.random_omission(rng, 1, R, n, keep, True)[0], rng.integers(1, 4, n, dtype=np.int32)


def _load_all(ctx, level, arg, total, begin=500, head=37):
    """Candidates [0, total) in chunks: one of `head` (so the next `first` is no multiple of the
    capacity), then of the capacity, the last one partial. (ho [total][R][n][W], init [total][n])."""
    hos, inits = [], []
    first = 0
    while first < total:
        k = min(head if first == 0 else CAP, total - first)
        ctx.shrink_load(level, arg, first, k, begin + first)
        ho, init = ctx.population_read(np.arange(k))
        hos.append(ho)
        inits.append(init)
        first += k
    return np.concatenate(hos), np.concatenate(inits)


def _inside_cap(ho, n):
    """(a LINK cap that falls strictly inside the links of a set in the middle of the base, the
    level's total under it)."""
    miss = (n - S.sizes(ho[None])[0]).reshape(-1)
    incl = np.cumsum(miss)
    wide = np.nonzero(miss >= 2)[0]
    s = wide[len(wide) // 2]
    return int(incl[s] - 1), int(incl[s])


# ---------------------------------------------------------------- 1. enumeration

@pytest.mark.parametrize("n,R", [(5, 3), (64, 2), (70, 3), (130, 1)], ids=["n5", "n64", "n70", "n130"])
def test_levels_enumerate_the_hosts_lists(n, R):
    ho, init = _base(n, R)
    cap_in, cut = _inside_cap(ho, n)
    cases = [(TAIL, 0), (TAIL, 1), (TAIL, R), (TAIL, abi.PSG_NEVER), (ROUND, 0), (SET, 0), (LINK, 0), (LINK, 1),
             (LINK, cap_in)]
    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=CAP) as g:
        ctx = g._ctx
        junk = ho.copy()
        if n % 64:  # bits >= n of the base are cleared on entry
            junk |= ~S.full_mask(n)
        ctx.shrink_begin(junk, None, init)
        back, cr = ctx.shrink_read()
        assert (back == ho).all() and cr is None
        for level, arg in cases:
            want, _ = candidates(ho, None, level, arg, n, R)
            total = ctx.shrink_count(level, arg)
            assert total == len(want), (level, arg)
            got, inits = _load_all(ctx, level, arg, total)
            assert got.shape == want.shape and (got == want).all(), (level, arg)
            assert (inits == init).all()
            print(f"n={n} level {level} arg {arg}: {total} candidates")
        assert ctx.shrink_count(LINK, cap_in) == cut <= ctx.shrink_count(LINK, 0)
        assert n == 5 or cut < ctx.shrink_count(LINK, 0)  # (n = 5: one set only has two links missing)
        assert ctx.shrink_count(TAIL, 0) == 1
        # the last chunk alone, and an empty one at the end
        total = ctx.shrink_count(SET, 0)
        ctx.shrink_load(SET, 0, total - 3, 3, 9)
        assert (ctx.population_read(np.arange(3))[0] == candidates(ho, None, SET, 0, n, R)[0][-3:]).all()
        ctx.shrink_load(SET, 0, total, 0, 9)
        assert ctx.population_links().shape == (0,)
        # a base of full sets: nothing to restore, and the tail candidate is the base
        full = np.broadcast_to(S.full_mask(n), ho.shape).copy()
        ctx.shrink_begin(full, None, init)
        assert [ctx.shrink_count(lv, 0) for lv in (ROUND, SET, LINK)] == [0, 0, 0]
        assert ctx.shrink_count(TAIL, 1) == 1
        ctx.shrink_load(TAIL, 1, 0, 1, 0)
        assert (ctx.population_read(np.arange(1))[0][0] == full).all()


@pytest.mark.parametrize("n", [5, 64, 70])
def test_population_links(n):
    R, P = 4, 101
    p = abi.PopulationParams()
    p.seed, p.generation, p.flips, p.self_bit, p.value_range = 5, 0, 3, 1, 3
    for j, k in enumerate((128, 192, 224, 250)):
        p.keep_p256[j] = k
    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=P) as g:
        ctx = g._ctx
        with pytest.raises(lib.PsgError) as e:
            ctx.population_links()  # nothing loaded
        assert e.value.rc == abi.PSG_EINVAL
        ctx.population_fresh(0, P, p)
        ho, _ = ctx.population_read(np.arange(P))
        links = ctx.population_links()
        assert links.dtype == np.uint32 and (links == S.sizes(ho).sum((-1, -2))).all()
        assert len(np.unique(links)) > 10
        junk = ho[:7].copy()
        if n % 64:  # bits >= n are not counted
            junk |= ~S.full_mask(n)
        ctx.load_schedule(3, 7, junk)
        assert (ctx.population_links() == links[:7]).all()


# ---------------------------------------------------------------- 2. adoption

@pytest.mark.parametrize("n,R", [(5, 3), (70, 3)], ids=["n5", "n70"])
def test_adopt_makes_the_candidate_the_base(n, R):
    ho, init = _base(n, R)
    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=CAP) as g:
        ctx = g._ctx
        for level, arg in ((TAIL, 1), (ROUND, 0), (SET, 0), (LINK, 0), (LINK, _inside_cap(ho, n)[0])):
            want, _ = candidates(ho, None, level, arg, n, R)
            for j in sorted({0, len(want) // 2, len(want) - 1}):
                ctx.shrink_begin(ho, None, init)
                ctx.shrink_load(level, arg, 0, min(CAP, len(want)), 0)  # (adoption does not need j loaded)
                ctx.shrink_adopt(level, arg, j)
                got, cr = ctx.shrink_read()
                assert cr is None and (got == want[j]).all(), (level, arg, j)
        # adoption moves the base: the next level's list is over the new one
        ctx.shrink_begin(ho, None, init)
        ctx.shrink_adopt(ROUND, 0, 0)
        base2 = candidates(ho, None, ROUND, 0, n, R)[0][0]
        want = candidates(base2, None, SET, 0, n, R)[0]
        assert ctx.shrink_count(SET, 0) == len(want) < len(candidates(ho, None, SET, 0, n, R)[0])
        got, _ = _load_all(ctx, SET, 0, len(want))
        assert (got == want).all()


# ---------------------------------------------------------------- 3. the crash level

def _crash_base(ctx, n, R, fmax, self_bit):
    """A base of the crash family from psg_population_fresh_model: a genome with at least two
    crashes, one of them in the last round where the search found one (it cannot move later)."""
    p = abi.PopulationParams()
    p.seed, p.generation, p.flips, p.self_bit, p.value_range = 7, 0, 1, self_bit, 3
    m = abi.PopulationModel()
    m.family, m.fmax = abi.PSG_POP_CRASH, fmax
    for j, d in enumerate((13, 38, 128, 218)):
        m.partial_p256[j] = d
    P = 256
    ctx.population_fresh_model(0, P, p, m)
    rows = np.arange(P)
    ho, init = ctx.population_read(rows)
    crash, _ = ctx.population_read_crash(rows)
    score = (crash >= 0).sum(1) * 2 + (crash == R - 1).any(1)
    i = int(np.argmax(np.where((crash >= 0).sum(1) >= 2, score, -1)))
    assert (crash[i] >= 0).sum() >= 2
    return ho[i], crash[i], init[i]


@pytest.mark.parametrize("n,R,fmax", [(8, 4, 3), (70, 3, 4)], ids=["n8", "n70"])
@pytest.mark.parametrize("self_bit", [1, 0])
def test_crash_level(n, R, fmax, self_bit):
    alg = psync.KSetEarlyStopping(t=fmax, k=2, variant=1)
    with psync.GpuRound(alg, n, R, batch_capacity=256) as g:
        ctx = g._ctx
        ho, crash, init = _crash_base(ctx, n, R, fmax, self_bit)
        want_ho, want_cr = candidates(ho, crash, CRASH, 0, n, R, bool(self_bit))
        f = int((crash >= 0).sum())
        later = int(((crash >= 0) & (crash + 1 < R)).sum())
        assert len(want_ho) == f + later
        print(f"n={n} self_bit={self_bit}: {f} crashes, {later} can move later")
        ctx.shrink_begin(ho, crash, init)
        total = ctx.shrink_count(CRASH, self_bit)
        assert total == len(want_ho)
        ctx.shrink_load(CRASH, self_bit, 0, total, 40)
        got, inits = ctx.population_read(np.arange(total))
        assert (got == want_ho).all() and (inits == init).all()
        with pytest.raises(lib.PsgError) as e:  # not a crash-family population
            ctx.population_read_crash(np.arange(total))
        assert e.value.rc == abi.PSG_EINVAL
        # the loaded crash rounds reach the kernels: the run equals the host-loaded one
        _, pi = ctx.run_batch_np(40, total)
        dec = ctx.copy_decisions_np()
        ctx.load_inputs(40, total, np.repeat(init[None], total, 0))
        ctx.load_schedule(40, total, want_ho, want_cr)
        _, pi2 = ctx.run_batch_np(40, total)
        dec2 = ctx.copy_decisions_np()
        assert pi.tobytes() == pi2.tobytes() and all((a == b).all() for a, b in zip(dec, dec2))
        # a part of the list, and every candidate adopted
        ctx.shrink_load(CRASH, self_bit, 1, total - 1, 0)
        assert (ctx.population_read(np.arange(total - 1))[0] == want_ho[1:]).all()
        for j in range(total):
            ctx.shrink_begin(ho, crash, init)
            ctx.shrink_adopt(CRASH, self_bit, j)
            got, cr = ctx.shrink_read()
            assert (got == want_ho[j]).all() and (cr == want_cr[j]).all(), j
        # below CRASH a candidate keeps the base's crash rounds
        ctx.shrink_begin(ho, crash, init)
        k = ctx.shrink_count(ROUND, 0)
        want_ho, want_cr = candidates(ho, crash, ROUND, 0, n, R)
        assert k == len(want_ho) and k >= 1
        ctx.shrink_load(ROUND, 0, 0, k, 0)
        _, pi = ctx.run_batch_np(0, k)
        ctx.load_inputs(0, k, np.repeat(init[None], k, 0))
        ctx.load_schedule(0, k, want_ho, want_cr)
        assert ctx.run_batch_np(0, k)[1].tobytes() == pi.tobytes()
        ctx.shrink_adopt(ROUND, 0, k - 1)
        got, cr = ctx.shrink_read()
        assert (got == want_ho[-1]).all() and (cr == crash).all()


# ---------------------------------------------------------------- 4. the loaded state

def test_loaded_candidates_run_as_host_loaded_ones():
    n, R = 70, 4
    ho, init = _base(n, R, keep=0.6)
    init = np.random.default_rng(3).integers(1, 3, n, dtype=np.int32)
    with psync.GpuRound(psync.OTR(variant=1), n, R, batch_capacity=256, value_range=2) as g:
        ctx = g._ctx
        ctx.shrink_begin(ho, None, init)
        total = ctx.shrink_count(SET, 0)
        k = min(256, total)
        ctx.shrink_load(SET, 0, total - k, k, 77)
        _, pi = ctx.run_batch_np(77, k)
        dec = ctx.copy_decisions_np()
        fs, fr = ctx.fetch_np(np.array([77, 77 + k - 1], np.uint64))
        live = ctx.population_live(abi.PSG_LIVE_GOOD_ROUND)
        got, inits = ctx.population_read(np.arange(k))
        ctx.load_inputs(77, k, inits)
        ctx.load_schedule(77, k, got)
        _, pi2 = ctx.run_batch_np(77, k)
        dec2 = ctx.copy_decisions_np()
        fs2, fr2 = ctx.fetch_np(np.array([77, 77 + k - 1], np.uint64))
        live2 = ctx.population_live(abi.PSG_LIVE_GOOD_ROUND)
    assert pi.tobytes() == pi2.tobytes() and all((a == b).all() for a, b in zip(dec, dec2))
    assert fs.tobytes() == fs2.tobytes() and fr.tobytes() == fr2.tobytes() and (live == live2).all()
    assert len({bytes(x["first_fail"]) for x in pi}) > 1 or len(set(pi["digest"].tolist())) > 1  # the candidates differ


# ---------------------------------------------------------------- 5. errors

def test_errors_change_nothing():
    n, R, P = 8, 4, 16
    ho, init = _base(n, R, keep=0.5)
    sched = S.random_omission(np.random.default_rng(1), P, R, n, 0.7)

    def refused(rc, call):
        with pytest.raises(lib.PsgError) as e:
            call()
        assert e.value.rc == rc, (e.value.rc, rc)

    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=P) as g:
        ctx = g._ctx
        ctx.load_inputs(5, P, np.repeat(init[None], P, 0))
        ctx.load_schedule(5, P, sched)
        for call in (lambda: ctx.shrink_count(ROUND), lambda: ctx.shrink_load(ROUND, 0, 0, 0, 0),
                     lambda: ctx.shrink_adopt(ROUND, 0, 0), lambda: ctx.shrink_read()):  # no base
            refused(abi.PSG_EINVAL, call)
        ctx.shrink_begin(ho, None, init)
        total = ctx.shrink_count(LINK, 0)
        assert total > P
        before = (ctx.population_read(np.arange(P)), ctx.shrink_read()[0], ctx.run_batch_np(5, P)[1].tobytes())
        for level in (5, -1, 77):
            for call in (lambda: ctx.shrink_count(level), lambda: ctx.shrink_load(level, 0, 0, 1, 0),
                         lambda: ctx.shrink_adopt(level, 0, 0)):  # unknown level
                refused(abi.PSG_EINVAL, call)
        for call in (lambda: ctx.shrink_count(CRASH, 1), lambda: ctx.shrink_load(CRASH, 1, 0, 0, 0),
                     lambda: ctx.shrink_adopt(CRASH, 1, 0)):  # CRASH without crash rounds
            refused(abi.PSG_EINVAL, call)
        refused(abi.PSG_ERANGE, lambda: ctx.shrink_load(LINK, 0, 0, P + 1, 0))            # count > batch_capacity
        refused(abi.PSG_ERANGE, lambda: ctx.shrink_load(LINK, 0, total - 3, 4, 0))         # first + count > total
        refused(abi.PSG_ERANGE, lambda: ctx.shrink_load(LINK, 0, total + 1, 0, 0))
        refused(abi.PSG_ERANGE, lambda: ctx.shrink_load(TAIL, 2, 1, 1, 0))
        refused(abi.PSG_ERANGE, lambda: ctx.shrink_adopt(LINK, 0, total))                  # j >= total
        refused(abi.PSG_ERANGE, lambda: ctx.shrink_adopt(TAIL, 2, 1))
        with pytest.raises(ValueError):
            ctx.shrink_begin(ho[:1], None, init)
        after = (ctx.population_read(np.arange(P)), ctx.shrink_read()[0], ctx.run_batch_np(5, P)[1].tobytes())
        assert all((x == y).all() for x, y in zip(before[0], after[0]))
        assert (before[1] == after[1]).all() and (after[1] == ho).all() and before[2] == after[2]
        assert (after[0][0] == sched).all()
        ctx.shrink_load(LINK, 0, total - 3, 3, 0)  # the edge itself is fine
        assert (ctx.population_read(np.arange(3))[0] == candidates(ho, None, LINK, 0, n, R)[0][-3:]).all()
    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=P, devices=[0, 0]) as g:  # a device-list context
        refused(abi.PSG_EINVAL, lambda: g._ctx.shrink_begin(ho, None, init))
        refused(abi.PSG_EINVAL, lambda: g._ctx.shrink_count(ROUND))
        refused(abi.PSG_EINVAL, lambda: g._ctx.shrink_read())
        g._ctx.load_schedule(0, 4, sched[:4])
        refused(abi.PSG_EINVAL, lambda: g._ctx.population_links())
    with psync.GpuRound(psync.EpsilonConsensus(), n, R, batch_capacity=P) as g:
        refused(abi.PSG_EINVAL, lambda: g._ctx.shrink_begin(ho, None, init))
        refused(abi.PSG_EINVAL, lambda: g._ctx.shrink_count(ROUND))


# ---------------------------------------------------------------- 6. shrink_device == shrink

#        name, algorithm, n, R, population, values, keywords
END_TO_END = [
    ("otr-n64", psync.OTR(variant=1), 64, 8, 1024, 3, dict(targets=["Safety"])),
    ("otr-n16-cap", psync.OTR(variant=1), 16, 8, 64, 2, {}),
    ("otr-n70", psync.OTR(variant=1), 70, 6, 1024, 3, dict(targets=["Safety"])),
    ("lv-n8", psync.LastVoting(variant=1), 8, 12, 1024, 3, {}),
    ("kses-n8", psync.KSetEarlyStopping(t=3, k=2, variant=1), 8, 5, 1024, 3, {}),
    ("otr-live-n32", psync.OTR(), 32, 6, 1024, 3, dict(mode="liveness", live_rounds=1)),
    ("tpc-live-n8", psync.TwoPhaseCommit(), 8, 6, 1024, 3, dict(mode="liveness", live_rounds=1)),
]


@pytest.mark.parametrize("name,alg,n,R,P,V,kw", END_TO_END, ids=[c[0] for c in END_TO_END])
def test_shrink_device_equals_shrink(name, alg, n, R, P, V, kw):
    """Every case: a counterexample is found, shrink() changes it, and shrink_device() returns the
    same one bit for bit, on the same Counterexample and the same Adversary."""
    with A.Adversary(alg, n, R, population=P, values=V, seed=5, **kw) as adv:
        assert adv.device_shrink_available() and adv.device_shrink is False
        res = adv.search(generations=60, want=1, shrink=False)
        assert res.counterexamples, f"{name}: no counterexample in {res.schedules_evaluated} schedules"
        c0 = res.counterexamples[0]
        host = adv.shrink(c0)
        dev = adv.shrink_device(c0)
        again = adv.shrink_device(c0)
        stats = adv.shrink_stats
    print(f"{name}: found after {res.generations} generations; omitted links {c0.omitted_links} -> "
          f"{host.omitted_links}, check point {c0.check_point} -> {host.check_point}, {stats}")
    assert not same_cex(c0, host), f"{name}: shrink() left the counterexample unchanged"
    assert (dev.ho == host.ho).all() and dev.ho.dtype == host.ho.dtype and dev.ho.shape == host.ho.shape
    assert same_cex(dev, host) and same_cex(again, host)
    assert (dev.crash is None) == (adv.model.family != "crash")
    assert stats["steps"] >= 1 and stats["candidates"] >= stats["steps"]


def test_shrink_device_under_the_link_cap():
    """End to end with LINK steps cut by the cap: the counterexample of a population-64 search is
    shrunk by an Adversary of population 2 (cap 8, chunks of 2 candidates), both paths on it: the
    tail step leaves one round's links, fewer than the cap of a larger population."""
    alg, n, R = psync.OTR(variant=1), 16, 8
    with A.Adversary(alg, n, R, population=64, values=2, seed=5) as adv:
        c0 = adv.search(generations=60, want=1, shrink=False).counterexamples[0]
    with A.Adversary(alg, n, R, population=2, values=2, seed=5) as adv:
        host = adv.shrink(c0)
        ctx = adv.evaluator.gr._ctx
        count, capped = ctx.shrink_count, []

        def counting(level, arg=0):
            if level == LINK and arg:
                capped.append((count(level, 0), count(level, arg)))
            return count(level, arg)

        ctx.shrink_count = counting
        dev = adv.shrink_device(c0)
    print(f"LINK steps (uncapped, capped): {capped}")
    assert not same_cex(c0, host) and same_cex(dev, host)
    assert capped and all(c <= f for f, c in capped)
    assert any(8 < c < f for f, c in capped), "no LINK step was cut by the cap 4 * population"


def test_shrink_device_respects_max_steps():
    with A.Adversary(psync.OTR(variant=1), 16, 8, population=256, values=2, seed=5) as adv:
        c0 = adv.search(generations=60, want=1, shrink=False).counterexamples[0]
        for steps in (1, 2, 5):
            assert same_cex(adv.shrink(c0, max_steps=steps), adv.shrink_device(c0, max_steps=steps)), steps
            assert adv.shrink_stats["steps"] <= steps


SEARCHES = [
    ("safety-device-population", psync.OTR(variant=1), 8, 6, dict(targets=["Agreement"], population=512)),
    ("safety-host-generator", psync.OTR(variant=1), 8, 6, dict(targets=["Agreement"], population=512, device_pop=False)),
    ("liveness-device-models", psync.OTR(), 8, 4, dict(mode="liveness", live_rounds=1, live_at=[0], keep=0.5,
                                                        population=2048, device_models=True)),
    ("crash-device-models", psync.FloodMin(2, variant=1), 8, 4, dict(population=2048, device_models=True)),
]


@pytest.mark.parametrize("name,alg,n,R,kw", SEARCHES, ids=[c[0] for c in SEARCHES])
def test_search_with_device_shrink_returns_the_same(name, alg, n, R, kw):
    out = []
    for flag in (False, True):
        with A.Adversary(alg, n, R, seed=7, device_shrink=flag, **kw) as adv:
            assert adv.device_population() is (name != "safety-host-generator")
            calls = []
            inner = adv.shrink_device
            adv.shrink_device = lambda c, inner=inner, calls=calls: calls.append(1) or inner(c)
            out.append(adv.search(generations=60, want=2).counterexamples)
            assert bool(calls) is flag and (not flag or len(calls) == len(out[-1]))
    assert out[0] and len(out[0]) == len(out[1])
    assert all(same_cex(a, b) for a, b in zip(*out))


def test_benor_shrinks_on_the_host():
    out = []
    for flag in (False, True):
        with A.Adversary(psync.BenOr(variant=1), 8, 12, population=2048, values=2, seed=11, device_shrink=flag) as adv:
            assert adv.device_shrink_available() is False
            out.append(adv.search(generations=60, want=1).counterexamples)
            with pytest.raises(ValueError):
                adv.shrink_device(out[-1][0])
    assert out[0] and len(out[0]) == len(out[1])
    assert all(same_cex(a, b) for a, b in zip(*out))
