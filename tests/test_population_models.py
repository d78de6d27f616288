"""Population models without a GPU: the psg_population_model ABI (layout, symbols), the
Adversary's device_models switch, TwoPhaseCommit's liveness model on the host path, and the
host-path liveness searches that the GPU tests of tests/test_gpu_population_models.py mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from round_amd import abi, adversary as A, lib, psync, schedules as S

from oracle_eval import OracleEvaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "psg.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F));
int main(void) {
  printf("psg_population_model %zu\n", sizeof(psg_population_model));
  P(psg_population_model, partial_p256) P(psg_population_model, live_kind) P(psg_population_model, live_at)
  P(psg_population_model, coord)
  printf("psg_population_params %zu\n", sizeof(psg_population_params));
  printf("PSG_POP_MAX_LIVE %d\n", PSG_POP_MAX_LIVE);
  printf("enums %d\n", PSG_POP_CRASH * 1000 + PSG_LIVE_GOOD_ROUND * 100 + PSG_LIVE_COORD_HEARS_ALL * 10
                       + PSG_LIVE_FIXED_COORD);
  printf("PSG_ABI_VERSION %d\n", PSG_ABI_VERSION);
  return 0;
}
"""


def test_model_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in
                                  subprocess.check_output([str(exe)], text=True).splitlines())}
    M = abi.PopulationModel
    assert got == {
        "psg_population_model": C.sizeof(M),
        "psg_population_model.partial_p256": M.partial_p256.offset,
        "psg_population_model.live_kind": M.live_kind.offset,
        "psg_population_model.live_at": M.live_at.offset,
        "psg_population_model.coord": M.coord.offset,
        "psg_population_params": 48,  # unchanged
        "PSG_POP_MAX_LIVE": abi.PSG_POP_MAX_LIVE,
        "enums": abi.PSG_POP_CRASH * 1000 + abi.PSG_LIVE_GOOD_ROUND * 100 + abi.PSG_LIVE_COORD_HEARS_ALL * 10
        + abi.PSG_LIVE_FIXED_COORD,
        "PSG_ABI_VERSION": 4,
    }
    assert C.sizeof(abi.PopulationParams) == 48
    assert abi.PopulationModel().phase == 1 and abi.PopulationModel().family == abi.PSG_POP_OMISSION


def test_model_symbols_exported():
    L = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("psg_population_fresh_model", "psg_population_next_model", "psg_population_read_crash",
                 "psg_population_live"):
        assert name in exported and name in lib.EXPORTED_SYMBOLS and hasattr(L, name)
    # null arguments are refused before anything is touched
    assert L.psg_population_fresh_model(None, 0, 0, None, None) == abi.PSG_EINVAL
    assert L.psg_population_next_model(None, None, None, None, None) == abi.PSG_EINVAL
    assert L.psg_population_read_crash(None, None, 0, None, None) == abi.PSG_EINVAL
    assert L.psg_population_live(None, 1, 1, 0, None) == abi.PSG_EINVAL


def test_device_models_needs_the_gpu_evaluator():
    alg = psync.FloodMin(2)
    adv = A.Adversary(alg, 8, 4, evaluator=OracleEvaluator(alg, 8, 4), device_models=True)
    assert adv.device_population() is False
    pm = adv._pop_model()  # the model the device path would pass
    assert pm.family == abi.PSG_POP_CRASH and pm.fmax == 2 and list(pm.partial_p256) == [13, 38, 128, 218]
    assert (pm.move_p256, pm.add_p256, pm.drop_p256) == (77, 77, 38)
    alg = psync.OTR()
    adv = A.Adversary(alg, 8, 4, mode="liveness", live_at=[0, 1], evaluator=OracleEvaluator(alg, 8, 4),
                      device_models=True)
    assert adv.device_population() is False
    pm = adv._pop_model()
    assert pm.family == abi.PSG_POP_OMISSION and pm.live_kind == abi.PSG_LIVE_GOOD_ROUND
    assert pm.live_rounds == 2 and list(pm.live_at)[:2] == [0, 1]
    assert A.Adversary(alg, 8, 4, evaluator=OracleEvaluator(alg, 8, 4))._pop_model() is None


def test_tpc_liveness_model_on_the_host_path():
    alg = psync.TwoPhaseCommit(coord=2)
    adv = A.Adversary(alg, 5, 3, mode="liveness", live_at=[1], evaluator=lambda *a: None)
    assert (adv.model.liveness, adv.model.phase, adv.model.coord) == ("fixed_coord", 3, 2)
    genome = adv._fresh(64)
    assert not S.fixed_coord_live(S.apply_universe(genome["ho"].copy(), 5, True), 5, 2).all()  # not live by chance
    ho, crash, valid = adv._realize(genome)
    assert crash is None and valid.all()
    assert S.fixed_coord_live(ho, 5, 2).all()
    assert (adv._live_count(ho) == 3).all()
    pm = adv._pop_model()
    assert (pm.live_kind, pm.phase, pm.coord) == (abi.PSG_LIVE_FIXED_COORD, 3, 2)
    # the forcing function alone: slot 1 the coordinator hears all, slot 2 all hear it, nothing else changes
    rng = np.random.default_rng(3)
    h0 = S.random_omission(rng, 4, 6, 70, 0.5)
    h1 = S.force_fixed_coord(h0.copy(), 70, 66, [3, 4, 5])
    assert S.fixed_coord_live(h1, 70, 66)[:, 3:].all() and not S.fixed_coord_live(h0, 70, 66)[:, 3:].all()
    assert (h1[:, :4] == h0[:, :4]).all() and (h1[:, 4, 66] == S.full_mask(70)).all() and (h1 | h0 == h1).all()


def test_liveness_still_raises_without_a_predicate():
    ev = OracleEvaluator(psync.OTR(), 4, 3)
    for alg in (psync.LatticeAgreement(), psync.FloodMin(2), psync.KSetAgreement(2), psync.KSetEarlyStopping(2, 2)):
        with pytest.raises(ValueError):
            A.Adversary(alg, 4, 3, mode="liveness", evaluator=ev, device_models=True)


def test_liveness_search_finds_non_termination_on_the_host_path():
    """One good round does not make OTR terminate within 4 rounds under heavy loss; two good
    rounds (rounds 0 and 1) do. The reference outcomes for the device-path search."""
    alg, n = psync.OTR(), 8
    adv = A.Adversary(alg, n, 4, mode="liveness", live_rounds=1, live_at=[0], keep=0.5, population=512,
                      evaluator=OracleEvaluator(alg, n, 4), seed=7)
    res = adv.search(generations=5, want=1)
    assert res.counterexamples and res.counterexamples[0].violated == ["Termination"]
    c = res.counterexamples[0]
    assert S.good_round(c.ho[None], n)[0].sum() >= 1 and int(c.summary["term_round"]) == abi.PSG_NEVER
    adv = A.Adversary(alg, n, 6, mode="liveness", live_rounds=2, live_at=[0, 1], keep=0.5, population=512,
                      evaluator=OracleEvaluator(alg, n, 6), seed=7)
    res = adv.search(generations=5, want=1)
    assert not res.counterexamples and res.schedules_evaluated == 5 * 512
