"""Device-resident populations under a model (psg_population_fresh_model / _next_model /
_read_crash / psg_population_live): the crash-stop family's genome and HO sets against
schedules.crash_to_ho, the liveness predicates against schedules.good_round / coord_hears_all /
fixed_coord_live, the forced live rounds, and the Adversary's device_models searches."""
import numpy as np
import pytest

from round_amd import abi, adversary as A, lib, psync, records, schedules as S

pytestmark = pytest.mark.gpu

LEVELS = (13, 38, 128, 218)


def _params(seed=5, gen=0, flips=3, min_size=0, self_bit=1, keep=(128, 192, 224, 250), V=3, redraw=5):
    p = abi.PopulationParams()
    p.seed, p.generation, p.flips, p.min_size, p.self_bit = seed, gen, flips, min_size, self_bit
    for j, k in enumerate(keep):
        p.keep_p256[j] = k
    p.value_range, p.redraw_p256 = V, redraw
    return p


def _crash_model(fmax, levels=LEVELS, rates=(77, 77, 38)):
    m = abi.PopulationModel()
    m.family, m.fmax = abi.PSG_POP_CRASH, fmax
    for j, d in enumerate(levels):
        m.partial_p256[j] = d
    m.move_p256, m.add_p256, m.drop_p256 = rates
    return m


def _live_model(kind, live_at, phase=1, coord=0):
    m = abi.PopulationModel()
    m.live_kind, m.live_rounds, m.phase, m.coord = kind, len(live_at), phase, coord
    for j, k in enumerate(live_at):
        m.live_at[j] = k
    return m


def _bits(x, n):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8), bitorder="little").reshape(x.shape[:-1] + (-1,))[..., :n]


def _read_all(ctx, P):
    rows = np.arange(P)
    ho, init = ctx.population_read(rows)
    crash, partial = ctx.population_read_crash(rows)
    return ho, init, crash, partial


# ---------------------------------------------------------------- 1. crash family, fresh

CRASH_CASES = [(psync.FloodMin(3), 5, 4, 3), (psync.KSetAgreement(2), 64, 4, 1), (psync.FloodMin(4), 70, 6, 4),
               (psync.FloodMin(3), 130, 3, 3)]


@pytest.mark.parametrize("alg,n,R,fmax", CRASH_CASES, ids=["fm-n5", "kset-n64", "fm-n70", "fm-n130"])
def test_crash_fresh_properties(alg, n, R, fmax):
    P = 403
    W = S.words(n)
    with psync.GpuRound(alg, n, R, batch_capacity=P) as g:
        ctx = g._ctx
        out = {}
        for sb in (1, 0):
            ctx.population_fresh_model(10, P, _params(self_bit=sb), _crash_model(fmax))
            out[sb] = _read_all(ctx, P)
    ho, init, crash, partial = out[1]
    for sb in (1, 0):  # the HO sets are the genome's, bit for bit (word edges, bits >= n)
        h, _, c, p = out[sb]
        assert (h == S.crash_to_ho(c, p, R, n, bool(sb))).all()
        assert (c == crash).all() and (p == partial).all()  # the genome does not depend on the self bit
    assert S.crash_consistent(ho, crash, n, fmax).all()
    assert ((crash >= -1) & (crash < R)).all()
    assert not _bits(partial, 64 * W)[..., n:].any()
    f = (crash >= 0).sum(1)
    assert set(f.tolist()) == set(range(fmax + 1))
    assert set(crash[crash >= 0].tolist()) == set(range(R))
    if n == 5:  # every process is chosen somewhere
        assert (crash >= 0).any(0).all()
    if n >= 64:
        for j, level in enumerate(LEVELS):
            d = _bits(partial[j::4], n).mean()
            print(f"n={n} level {level}/256: partial density {d:.4f}")
            assert abs(d - level / 256) < 0.02
    assert init.min() >= 1 and init.max() <= 3 and len(np.unique(init)) == 3


def test_crash_fresh_edges():
    n, R = 70, 4
    with psync.GpuRound(psync.FloodMin(2), n, R, batch_capacity=64) as g:
        ctx = g._ctx
        ctx.population_fresh_model(0, 64, _params(), _crash_model(0))  # fmax = 0: nobody crashes
        ho, init, crash, partial = _read_all(ctx, 64)
        assert (crash == -1).all() and (ho == S.full_mask(n)).all()
        ctx.population_fresh_model(7, 1, _params(), _crash_model(n))  # one instance, fmax = n
        ho, init, crash, partial = _read_all(ctx, 1)
        assert (ho == S.crash_to_ho(crash, partial, R, n, True)).all()
        _, pi = ctx.run_batch_np(7, 1)
        assert len(pi) == 1
        ctx.population_fresh_model(0, 0, _params(), _crash_model(2))  # an empty population
        ho, init, crash, partial = _read_all(ctx, 0)
        assert ho.shape[0] == 0 and crash.shape == (0, n)
        assert ctx.population_live(abi.PSG_LIVE_GOOD_ROUND).shape == (0, R)


# ---------------------------------------------------------------- 2. crash family, next generation

def test_crash_next_ops_and_determinism(oracle_mod):
    """Copies, mutants and fresh slots of the crash family; a population is a pure function of
    its parameters; the round kernels run the loaded population as the oracle does under the
    read-back sets and crash rounds. Random populations of 64 at this shape do not violate
    FloodMin's mutant and hardly depend on the crash array (the oracle over 20 populations of
    schedules.random_crash: no failing instance, 0 or 1 instance whose result changes without the
    crash rounds), so a guard on them cannot hold here: the guarded comparison is
    test_crash_population_runs_as_the_oracle_under_a_violation."""
    n, R, P, flips = 32, 5, 64, 3
    alg = psync.FloodMin(2, variant=1)
    outs = []
    for _ in range(2):
        with psync.GpuRound(alg, n, R, batch_capacity=P, value_range=1000) as g:
            ctx = g._ctx
            model = _crash_model(2)
            ctx.population_fresh_model(0, P, _params(flips=flips, V=1000), model)
            ho0, in0, cr0, pa0 = _read_all(ctx, P)
            parent = np.array([5] * 10 + [3] * 20 + list(range(10)) + [0] * (P - 40), np.uint32)
            op = np.array([0] * 10 + [1] * 30 + [2] * (P - 40), np.uint8)
            ctx.population_next_model(parent, op, _params(gen=1, flips=flips, V=1000), model)
            ho1, in1, cr1, pa1 = _read_all(ctx, P)
            _, pi = ctx.run_batch_np(0, P)
            # five all-mutate generations at fmax = 1, from a population of that bound
            m1 = _crash_model(1)
            ctx.population_fresh_model(0, P, _params(flips=flips), m1)
            for gen in range(1, 6):
                ctx.population_next_model(np.arange(P, dtype=np.uint32), np.ones(P, np.uint8),
                                          _params(gen=gen, flips=flips), m1)
            ho5, _, cr5, pa5 = _read_all(ctx, P)
            with pytest.raises(lib.PsgError):  # the plain call does not continue a crash population
                ctx.population_next(parent, op, _params(gen=9))
        outs.append((ho0, in0, cr0, pa0, ho1, in1, cr1, pa1, ho5, cr5, pa5))
        assert (ho1[:10] == ho0[5]).all() and (in1[:10] == in0[5]).all()
        assert (cr1[:10] == cr0[5]).all() and (pa1[:10] == pa0[5]).all()
        par = parent[10:40]
        dc = (cr1[10:40] != cr0[par]).sum(1)
        dp = (_bits(pa1[10:40], n) != _bits(pa0[par], n)).sum((1, 2))
        assert (dc <= 1).all() and dc.any()
        assert (dp <= flips).all() and dp.any()
        assert ((cr1 >= 0).sum(1) <= 2).all()
        assert (ho1 == S.crash_to_ho(cr1, pa1, R, n, True)).all()
        assert S.crash_consistent(ho1, cr1, n, 2).all()
        assert (in1[10:40] != in0[par]).mean() < 0.2
        assert ((cr5 >= 0).sum(1) <= 1).all() and S.crash_consistent(ho5, cr5, n, 1).all()
        assert (ho5 == S.crash_to_ho(cr5, pa5, R, n, True)).all()
        assert len({tuple(r) for r in cr5.tolist()}) > P // 4  # the mutants moved
        _, opi, _, _, _ = oracle_mod.run_schedule(g.cfg, 0, P, ho1, cr1, in1, per_instance=True)
        assert [int(x["digest"]) for x in pi] == [x.digest for x in opi]
        assert [bytes(x["first_fail"])[:2] for x in pi] == [bytes(x.first_fail)[:2] for x in opi]
    a, b = outs
    assert all((x == y).all() for x, y in zip(a, b))


def test_crash_population_runs_as_the_oracle_under_a_violation(oracle_mod):
    """The population in which the device search finds FloodMin's mutant violating k-agreement
    runs on the GPU exactly as on the oracle under the read-back sets, crash rounds and inputs.
    Guard, on the oracle alone: some instance fails a slot, and without the crash rounds the
    oracle's result differs (a crash array that never reached the kernels would not pass)."""
    n, R, P = 8, 4, 2048
    alg = psync.FloodMin(2, variant=1)
    with A.Adversary(alg, n, R, population=P, values=3, seed=11, device_models=True) as adv:
        assert adv.device_population()
        res = adv.search(generations=60, want=1, shrink=False)
        assert res.counterexamples
        ctx = adv.evaluator.gr._ctx
        base = adv.next_id - P
        ho, init, crash, _ = _read_all(ctx, P)
        _, pi = ctx.run_batch_np(base, P)
        cfg = adv.evaluator.cfg
    _, opi, _, _, _ = oracle_mod.run_schedule(cfg, base, P, ho, crash, init, per_instance=True)
    _, npi, _, _, _ = oracle_mod.run_schedule(cfg, base, P, ho, None, init, per_instance=True)
    k = len(alg.check_names)
    fails = sum(any(v != abi.PSG_NEVER for v in list(x.first_fail)[:k]) for x in opi)
    differ = sum(x.digest != y.digest or bytes(x.first_fail) != bytes(y.first_fail) for x, y in zip(opi, npi))
    print(f"oracle: {fails} failing instances, {differ} depend on the crash rounds")
    assert fails >= 1 and differ >= 1
    assert [int(x["digest"]) for x in pi] == [x.digest for x in opi]
    assert [bytes(x["first_fail"])[:k] for x in pi] == [bytes(x.first_fail)[:k] for x in opi]


# ---------------------------------------------------------------- 3. the predicate kernel

@pytest.mark.parametrize("n", [5, 64, 70, 256])
def test_live_predicates_match_host(n):
    rng = np.random.default_rng(n)
    I, R = 24, 12
    W = S.words(n)
    ho = S.random_omission(rng, I, R, n, 0.8)
    S.force_good_round(ho, rng, n, np.array([0, 1, 1, 2]), np.array([2, 0, 3, 5]))           # a common subset
    S.force_good_round(ho, rng, n, np.array([3, 4]), np.array([1, 7]), self_bit=True)       # everyone
    small = np.zeros(W, np.uint64)  # a common set that is too small: n / 2 members
    for q in range(n // 2):
        small[q >> 6] |= np.uint64(1 << (q & 63))
    ho[5, 4] = small
    S.force_coord_hears_all(ho[6:12], n, [0, 1, 4, 5, 6, 9], 4)
    S.force_fixed_coord(ho[12:18], n, 2, [1, 2, 4, 8, 10, 11])
    want = {abi.PSG_LIVE_GOOD_ROUND: S.good_round(ho, n),
            abi.PSG_LIVE_COORD_HEARS_ALL: S.coord_hears_all(ho, n, 4),
            abi.PSG_LIVE_FIXED_COORD: S.fixed_coord_live(ho, n, 2)}
    junk = ho.copy()
    if n % 64:  # bits >= n are ignored
        junk |= ~S.full_mask(n) & rng.integers(0, 1 << 64, size=ho.shape, dtype=np.uint64, endpoint=False)
        assert (junk != ho).any()
    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=I) as g:
        ctx = g._ctx
        with pytest.raises(lib.PsgError):
            ctx.population_live(abi.PSG_LIVE_GOOD_ROUND)  # nothing loaded
        ctx.load_schedule(100, I, junk)
        got = {abi.PSG_LIVE_GOOD_ROUND: ctx.population_live(abi.PSG_LIVE_GOOD_ROUND),
               abi.PSG_LIVE_COORD_HEARS_ALL: ctx.population_live(abi.PSG_LIVE_COORD_HEARS_ALL, phase=4),
               abi.PSG_LIVE_FIXED_COORD: ctx.population_live(abi.PSG_LIVE_FIXED_COORD, phase=3, coord=2)}
        for bad in ((0, 1, 0), (4, 1, 0), (1, 0, 0), (3, 3, n), (3, 3, -1)):
            with pytest.raises(lib.PsgError):
                ctx.population_live(*bad)
    for kind, w in want.items():
        assert w.any() and not w.all(), kind
        assert got[kind].dtype == np.uint8 and got[kind].shape == (I, R)
        assert (got[kind].astype(bool) == w).all(), kind


# ---------------------------------------------------------------- 4. forced rounds

def test_forced_good_rounds():
    n, R, P = 32, 6, 256
    good = abi.PSG_LIVE_GOOD_ROUND
    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=P) as g:
        ctx = g._ctx
        model = _live_model(good, [0, 1])
        ctx.population_fresh_model(0, P, _params(), model)
        live = ctx.population_live(good)
        ho, _ = ctx.population_read(np.arange(P))
        assert live[:, :2].all() and (ho[:, :2] == S.full_mask(n)).all()
        assert (live.astype(bool) == S.good_round(ho, n)).all()
        assert not live[2::4, 2:].all()  # the other rounds stay lossy
        # a mutant cannot lose them
        ctx.population_next_model(np.arange(P, dtype=np.uint32), np.ones(P, np.uint8), _params(gen=1, flips=50), model)
        ho1, _ = ctx.population_read(np.arange(P))
        assert ctx.population_live(good)[:, :2].all() and (ho1[:, :2] == S.full_mask(n)).all()
        assert (ho1[:, 2:] != ho[:, 2:]).any()
        # drawn rounds: per instance, anywhere
        ctx.population_fresh_model(0, P, _params(), _live_model(good, [-1, -1]))
        live = ctx.population_live(good).astype(bool)
        ho, _ = ctx.population_read(np.arange(P))
        full = (ho == S.full_mask(n)).all((2, 3))[0::4]  # (levels below 256/256: a full round is a forced one)
        assert (live.sum(1) >= 1).all() and (live[0::4].sum(1) <= 2).all()
        assert (full == live[0::4]).all() and len({tuple(r) for r in full.tolist()}) > R
        assert full.any(0).all()  # every round is drawn somewhere
    n = 16
    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=P) as g:  # no self bit: a common subset
        ctx = g._ctx
        ctx.population_fresh_model(0, P, _params(self_bit=0), _live_model(good, [0, 1]))
        ho, _ = ctx.population_read(np.arange(P))
        live = ctx.population_live(good)
    assert live[:, :2].all()
    assert (ho[:, :2] == ho[:, :2, :1]).all()
    size = S.sizes(ho[:, :2, 0])
    assert (size > 2 * n // 3).all() and (size < n).any()  # larger than 2n/3, not everyone everywhere
    assert not _bits(ho, 64)[..., n:].any()
    assert len(np.unique(ho[:, 0, 0])) > 8


def test_forced_coordinator_phases():
    P = 128
    kind = abi.PSG_LIVE_COORD_HEARS_ALL
    n, R = 8, 12
    with psync.GpuRound(psync.LastVoting(), n, R, batch_capacity=P) as g:
        ctx = g._ctx
        model = _live_model(kind, [5], phase=4)
        ctx.population_fresh_model(0, P, _params(keep=(64, 96, 128, 160)), model)
        live = ctx.population_live(kind, phase=4).astype(bool)
        ho, _ = ctx.population_read(np.arange(P))
        assert live[:, 4:8].all() and (ho[:, 4:8, 1] == S.full_mask(n)).all()
        assert (live == S.coord_hears_all(ho, n, 4)).all() and not live[:, :4].all()
        ctx.population_next_model(np.arange(P, dtype=np.uint32), np.ones(P, np.uint8), _params(gen=1, flips=50), model)
        assert ctx.population_live(kind, phase=4)[:, 4:8].all()
    kind = abi.PSG_LIVE_FIXED_COORD
    n, R = 5, 3
    with psync.GpuRound(psync.TwoPhaseCommit(coord=2), n, R, batch_capacity=P) as g:
        ctx = g._ctx
        model = _live_model(kind, [1], phase=3, coord=2)
        ctx.population_fresh_model(0, P, _params(keep=(64, 96, 128, 160)), model)
        live = ctx.population_live(kind, phase=3, coord=2).astype(bool)
        ho, init = ctx.population_read(np.arange(P))
        assert live.all() and (live == S.fixed_coord_live(ho, n, 2)).all()
        assert (ho[:, 1, 2] == S.full_mask(n)).all() and S.contains(ho[:, 2], 2).all()
        assert not (ho[:, 1] == S.full_mask(n)).all()  # only the coordinator's set is forced
        # the coordinator hears every vote in slot 1 and everyone hears its decision in slot 2
        _, pi = ctx.run_batch_np(0, P)
        assert (pi["term_round"] == 3).all()
        ctx.population_next_model(np.arange(P, dtype=np.uint32), np.ones(P, np.uint8), _params(gen=1, flips=50), model)
        assert ctx.population_live(kind, phase=3, coord=2).all()


def test_invalid_models_change_nothing():
    n, R, P = 8, 6, 16

    def crash(**kw):
        m = _crash_model(2)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def live(kind=abi.PSG_LIVE_GOOD_ROUND, at=(0,), **kw):
        m = _live_model(kind, list(at), phase=kw.pop("phase", 3), coord=kw.pop("coord", 0))
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    bad = [
        (crash(family=2), _params()), (live(kind=4), _params()), (live(kind=-1), _params()),
        (crash(fmax=-1), _params()), (crash(fmax=n + 1), _params()),
        (crash(), _params(min_size=3)), (crash(live_kind=abi.PSG_LIVE_GOOD_ROUND), _params()),
        (live(live_rounds=-1), _params()), (live(live_rounds=abi.PSG_POP_MAX_LIVE + 1), _params()),
        (live(at=(R,)), _params()), (live(at=(0, R + 3)), _params()),
        (live(phase=0), _params()), (live(coord=-1), _params()), (live(coord=n), _params()),
        (crash(move_p256=200, add_p256=50, drop_p256=7), _params()),
    ]
    with psync.GpuRound(psync.FloodMin(2), n, R, batch_capacity=P) as g:
        ctx = g._ctx
        ctx.population_fresh_model(0, P, _params(), _crash_model(2))
        before = _read_all(ctx, P)
        parent, op = np.arange(P, dtype=np.uint32), np.ones(P, np.uint8)
        for m, p in bad:
            for call in (lambda: ctx.population_fresh_model(0, P, p, m),
                         lambda: ctx.population_next_model(parent, op, p, m)):
                with pytest.raises(lib.PsgError) as e:
                    call()
                assert e.value.rc == abi.PSG_EINVAL
        with pytest.raises(lib.PsgError):  # the other family does not continue a crash population
            ctx.population_next_model(parent, op, _params(), live())
        after = _read_all(ctx, P)
        assert all((x == y).all() for x, y in zip(before, after))
        _, pi = ctx.run_batch_np(0, P)  # and it is still loaded
        assert len(pi) == P
    with psync.GpuRound(psync.OTR(), n, R, batch_capacity=P) as g:
        ctx = g._ctx
        with pytest.raises(lib.PsgError):
            ctx.population_next_model(parent, op, _params(), live())  # nothing loaded
        # the omission family with nothing forced is the plain call, bit for bit
        ctx.population_fresh(0, P, _params())
        ctx.population_next(parent[::-1].copy(), (np.arange(P) % 3).astype(np.uint8), _params(gen=1))
        plain = ctx.population_read(np.arange(P))
        ctx.population_fresh_model(0, P, _params(), abi.PopulationModel())
        ctx.population_next_model(parent[::-1].copy(), (np.arange(P) % 3).astype(np.uint8), _params(gen=1),
                                  abi.PopulationModel())
        assert all((x == y).all() for x, y in zip(plain, ctx.population_read(np.arange(P))))
        with pytest.raises(lib.PsgError):
            ctx.population_read_crash(np.arange(P))  # not a crash population
    with psync.GpuRound(psync.EpsilonConsensus(), n, R, batch_capacity=P) as g:
        with pytest.raises(lib.PsgError):
            g._ctx.population_fresh_model(0, P, _params(), abi.PopulationModel())
        g._ctx.load_schedule(0, 2, S.random_omission(np.random.default_rng(0), 2, R, n, 0.5))
        with pytest.raises(lib.PsgError):
            g._ctx.population_live(abi.PSG_LIVE_GOOD_ROUND)


# ---------------------------------------------------------------- 5. search with device_models

MUTANTS = [("fm-mutant-n8", psync.FloodMin(2, variant=1), 8, 4),
           ("kses-mutant-n8", psync.KSetEarlyStopping(t=2, k=2, variant=1), 8, 4)]


@pytest.mark.parametrize("name,alg,n,R", MUTANTS, ids=[c[0] for c in MUTANTS])
def test_device_crash_search_finds_and_replays(name, alg, n, R, tmp_path, oracle_mod):
    with A.Adversary(alg, n, R, population=2048, values=3, seed=11, device_models=True) as adv:
        assert adv.device_population()
        res = adv.search(generations=60, want=2)
        assert res.counterexamples, f"{name}: no counterexample in {res.schedules_evaluated} schedules"
        print(f"{name}: found after {res.generations} generations")
        assert all(c.crash is not None for c in res.counterexamples)
        path = str(tmp_path / "cex.psgr")
        A.save(path, adv, res.counterexamples, meta={"test": name})
    back = records.read(path)
    assert back.count == len(res.counterexamples) and back.crash is not None
    records.replay(path)
    for j in range(back.count):
        assert S.crash_consistent(back.ho[j:j + 1], back.crash[j:j + 1], n, alg.param).all()
        _, opi, _, _, _ = oracle_mod.run_schedule(back.cfg, int(back.ids[j]), 1, back.ho[j:j + 1], back.crash[j:j + 1],
                                                  back.init[j:j + 1], per_instance=True)
        assert opi[0].digest == int(back.summary[j]["digest"])
        assert bytes(opi[0].first_fail)[:len(back.slot_names)] == bytes(back.summary[j]["first_fail"])[
            :len(back.slot_names)]
    for c in res.counterexamples:
        assert c.violated and c.check_point < abi.PSG_NEVER


def test_device_crash_search_reference_holds():
    with A.Adversary(psync.FloodMin(2), 16, 4, population=4096, values=3, seed=12, device_models=True) as adv:
        assert adv.device_population()
        res = adv.search(generations=15, want=1, shrink=False)
    assert not res.counterexamples, A.describe(res.counterexamples[0], 16)
    assert res.schedules_evaluated == 15 * 4096
    with A.Adversary(psync.FloodMin(2), 16, 4, population=64, values=3, seed=12) as adv:
        assert adv.device_population() is False  # the switch is off by default
    with A.Adversary(psync.OTR(), 8, 4, mode="liveness", population=64) as adv:
        assert adv.device_population() is False


def test_device_liveness_searches():
    # two good rounds at rounds 0 and 1: OTR terminates
    with A.Adversary(psync.OTR(), 32, 6, mode="liveness", live_at=[0, 1], population=2048, seed=14,
                     device_models=True) as adv:
        assert adv.device_population()
        res = adv.search(generations=5, want=1, shrink=False)
    assert not res.counterexamples and res.schedules_evaluated == 5 * 2048
    # one good round is not enough under heavy loss (the host path: <= 5 generations of 512)
    with A.Adversary(psync.OTR(), 8, 4, mode="liveness", live_rounds=1, live_at=[0], keep=0.5, population=2048,
                     seed=7, device_models=True) as adv:
        assert adv.device_population()
        res = adv.search(generations=20, want=1)
    assert res.counterexamples and res.counterexamples[0].violated == ["Termination"]
    c = res.counterexamples[0]
    print(f"otr liveness: found after {res.generations} generations")
    assert c.crash is None and S.good_round(c.ho[None], 8)[0].sum() >= 1
    assert int(c.summary["term_round"]) == abi.PSG_NEVER
    # TwoPhaseCommit with a live phase terminates
    with A.Adversary(psync.TwoPhaseCommit(coord=2), 5, 3, mode="liveness", live_at=[1], population=1024, seed=5,
                     device_models=True) as adv:
        assert adv.device_population()
        res = adv.search(generations=5, want=1, shrink=False)
    assert not res.counterexamples and res.schedules_evaluated == 5 * 1024
