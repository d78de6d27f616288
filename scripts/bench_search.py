#!/usr/bin/env python3
"""Adversary-search throughput: explicit schedules evaluated
per second by round_amd.adversary on one MI355X, host generation included, and
the time to the first counterexample for mutated algorithms.

Rows (one JSON line each, then a JSON list in --out):
  * reference OTR n=64 R=20, safety search, 2^15 schedules per generation: no
    counterexample expected; reports schedules/s and the GPU share of the time;
  * mutants (OTR, LastVoting, FloodMin, BenOr): generations / seconds / schedules
    to the first counterexample and the shrunk counterexample's size;
  * reference FloodMin(f=3) n=64 R=6 (crash-stop family) and OTR liveness n=64 R=20 with good
    rounds 0 and 1, 2^15 schedules per generation, no counterexample expected: the two search
    shapes whose generations stay on the host unless --device-models moves them to the GPU
    (psg_population_*_model).
--ab-models N measures those two rows only: one warm-up search per row and path, then N passes
alternating the host-generator and the device-model path.
--ab-shrink N measures the shrink step only: per row (the OTR safety mutant at n=64, R=8, population
4096; an OTR liveness search with one good round at n=64, R=20) one counterexample found with
shrink=False, one warm-up of each path, then N passes alternating Adversary.shrink and
Adversary.shrink_device on that counterexample; per pass seconds, steps, candidates evaluated and
whether the two results are identical.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from round_amd import adversary as A, psync  # noqa: E402


def row(name, alg, n, R, targets=None, population=4096, generations=10, want=1, stop=True, values=3,
        device_models=False, **search_kw):
    t0 = time.perf_counter()
    with A.Adversary(alg, n, R, targets=targets, population=population, values=values, seed=7,
                     device_models=device_models, **search_kw) as adv:
        device = adv.device_population()
        res = adv.search(generations=generations, want=want if stop else 10 ** 9, shrink=stop)
    out = {"row": name, "class": alg.class_name, "variant": alg.variant, "n": n, "rounds": R,
           "device_population": device, "gpu_share": round(res.gpu_seconds / res.seconds, 3) if res.seconds else 0.0,
           "population": population, "generations": res.generations,
           "schedules": res.schedules_evaluated, "seconds": round(res.seconds, 3),
           "schedules_per_s": round(res.schedules_per_second, 1),
           "checked_process_rounds_per_s": round(res.schedules_per_second * n * R, 1),
           "gpu_seconds": round(res.gpu_seconds, 3), "found": len(res.counterexamples),
           "wall_s": round(time.perf_counter() - t0, 3)}
    if res.counterexamples:
        c = res.counterexamples[0]
        out.update(violated=c.violated, check_point=c.check_point, omitted_links=int(c.omitted_links))
    print(json.dumps(out), flush=True)
    return out


def model_rows(population, generations, device_models, **extra):
    """The crash-stop and the liveness reference rows (host generator unless device_models)."""
    out = [row("ref_floodmin_n64", psync.FloodMin(3), 64, 6, population=population, generations=generations,
               stop=False, device_models=device_models),
           row("live_otr_n64", psync.OTR(), 64, 20, population=population, generations=generations, stop=False,
               device_models=device_models, mode="liveness", live_at=[0, 1])]
    for r in out:
        r.update(extra)
    return out


def shrink_rows(name, alg, n, R, passes, max_steps, population, generations=60, **kw):
    """One counterexample found with shrink=False, then `passes` passes alternating Adversary.shrink
    (the host builds and uploads every candidate) and Adversary.shrink_device (psg_shrink_*) on it,
    after one warm-up of each. Per pass: seconds, steps, candidates evaluated, identical results.
    (Liveness rows: the device path also evaluates the candidates with too few live rounds, which the
    host drops before evaluating, so its count can be the larger one.)"""
    rows = []
    with A.Adversary(alg, n, R, population=population, seed=7, **kw) as adv:
        res = adv.search(generations=generations, want=1, shrink=False)
        if not res.counterexamples:
            raise SystemExit(f"{name}: no counterexample in {res.schedules_evaluated} schedules")
        c = res.counterexamples[0]

        def one(path, k):
            t0 = time.perf_counter()
            out = adv.shrink(c, max_steps) if path == "host" else adv.shrink_device(c, max_steps)
            secs = time.perf_counter() - t0
            stats = adv.shrink_stats
            return out, {"row": name, "path": path, "pass": k, "n": n, "rounds": R, "population": population,
                         "max_steps": max_steps, "seconds": round(secs, 4), "batches": stats["batches"],
                         "steps": stats["steps"], "candidates": stats["candidates"],
                         "omitted_links_before": int(c.omitted_links), "omitted_links_after": int(out.omitted_links)}

        one("host", -1)
        one("device", -1)
        for k in range(passes):
            host, hrow = one("host", k)
            dev, drow = one("device", k)
            hrow["identical"] = drow["identical"] = host.same(dev)
            for r in (hrow, drow):
                print(json.dumps(r), flush=True)
            rows += [hrow, drow]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-shrink", type=int, default=0, metavar="N",
                    help="only the shrink comparison: per row one counterexample, a warm-up, then N passes "
                         "alternating shrink() and shrink_device() on it")
    ap.add_argument("--max-steps", type=int, default=64, help="--ab-shrink: the step budget of both paths")
    ap.add_argument("--device-models", action="store_true",
                    help="crash-stop and liveness searches generate their populations on the GPU")
    ap.add_argument("--ab-models", type=int, default=0, metavar="N",
                    help="only the two model rows: a warm-up, then N passes alternating host and device generation")
    ap.add_argument("--out", default="")
    ap.add_argument("--population", type=int, default=32768)
    ap.add_argument("--generations", type=int, default=8)
    a = ap.parse_args()
    if a.ab_shrink:
        rows = shrink_rows("mut_otr_n64_safety", psync.OTR(variant=1), 64, 8, a.ab_shrink, a.max_steps, 4096,
                           targets=["Safety"])
        # one good round is not enough for OTR: found in the first generation
        rows += shrink_rows("live_otr_n64_one_good_round", psync.OTR(), 64, 20, a.ab_shrink, a.max_steps, a.population,
                            mode="liveness", live_rounds=1, device_models=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        return
    if a.ab_models:
        rows = []
        for dm in (False, True):
            model_rows(a.population, 2, dm, warmup=True)
        for k in range(a.ab_models):
            for dm in (False, True):
                rows += model_rows(a.population, a.generations, dm, **{"pass": k})
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        return
    rows = [row("ref_otr_n64", psync.OTR(), 64, 20, population=a.population, generations=a.generations,
                stop=False, values=3)]
    rows.append(row("mut_otr_n64_safety", psync.OTR(variant=1), 64, 8, ["Safety"], population=4096, generations=60))
    rows.append(row("mut_otr_n16_agreement", psync.OTR(variant=1), 16, 8, ["Agreement"], population=4096,
                    generations=60, values=2))
    rows.append(row("mut_lv_n8_agreement", psync.LastVoting(variant=1), 8, 12, ["Agreement"], population=4096,
                    generations=60))
    rows.append(row("mut_floodmin_n8", psync.FloodMin(2, variant=1), 8, 4, population=4096, generations=60,
                    device_models=a.device_models))
    rows.append(row("mut_benor_n8", psync.BenOr(variant=1), 8, 12, population=4096, generations=60, values=2))
    rows += model_rows(a.population, a.generations, a.device_models)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
