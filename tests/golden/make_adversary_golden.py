#!/usr/bin/env python3
"""Generate tests/golden/adversary_paths.json: what round_amd.adversary.Adversary.search returns,
draws and numbers on a fixed list of small searches, recorded from the code as it stands.

The file characterises the search and shrink drivers, it does not judge them: a refactor of
round_amd/adversary.py must leave every recorded field as it is (tests/test_adversary_golden.py
replays the host section on the CPU with the oracle as evaluator, tests/test_gpu_adversary_golden.py
the device section on the GPU). A change that is meant to alter a search re-records the file.

Per case: generations, schedules_evaluated, the history (repr of each float), Adversary.next_id, a
sha256 of the generator state after the search (the number and order of the random draws) and per
counterexample the instance id, sha256 of ho / crash / init / summary, check_point, violated and
omitted_links; device cases with device_shrink also Adversary.shrink_stats. Every case runs twice
and is refused if the two runs differ. Each section carries the git commit it was recorded on.

Run: python tests/golden/make_adversary_golden.py [--section host|device|all] [--out FILE]
     (--commit HASH where the tree is not a git checkout)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from round_amd import adversary as A, psync  # noqa: E402

PATH = os.path.join(HERE, "adversary_paths.json")
SEED, WANT = 5, 2

#  name: (algorithm, n, R, Adversary keywords, generations)
HOST_CASES = {
    "otr-safety": (psync.OTR(variant=1), 8, 6, dict(targets=["Agreement"], population=512), 40),
    "fm-crash": (psync.FloodMin(f=2, variant=1), 8, 4, dict(population=512), 40),
    "kses-crash": (psync.KSetEarlyStopping(t=3, k=2, variant=1), 8, 5, dict(population=512), 40),
    "otr-cap": (psync.OTR(variant=1), 16, 6, dict(population=8, values=2), 40),
    "lv-mut": (psync.LastVoting(variant=1), 6, 12, dict(targets=["Agreement"], population=1024), 60),
    "otr-live": (psync.OTR(), 8, 6, dict(mode="liveness", live_rounds=1, population=512), 40),
    "lv-live": (psync.LastVoting(), 6, 12, dict(mode="liveness", live_rounds=2, population=256), 5),
    "otr-live-at": (psync.OTR(), 8, 6, dict(mode="liveness", live_rounds=2, live_at=[0, 1], population=256), 5),
    "ref-otr": (psync.OTR(), 8, 6, dict(population=256), 6),
    "benor": (psync.BenOr(variant=1), 8, 12, dict(population=512, values=2), 40),
    "eps": (psync.EpsilonConsensus(f=1, epsilon=1e-3, variant=1), 8, 6, dict(population=512), 40),
    "otr-n70": (psync.OTR(variant=1), 70, 4, dict(population=64), 20),
}

# each one recorded with device_shrink=False ("<name>") and with device_shrink=True ("<name>+dshrink")
_DEVICE = {
    "otr-safety": (psync.OTR(variant=1), 8, 6, dict(targets=["Agreement"], population=512), 40),
    "fm-crash": (psync.FloodMin(f=2, variant=1), 8, 4, dict(population=512, device_models=True), 40),
    "otr-live": (psync.OTR(), 8, 6, dict(mode="liveness", live_rounds=1, population=512, device_models=True), 40),
    "otr-n70": (psync.OTR(variant=1), 70, 4, dict(population=64), 20),
}
DEVICE_CASES = {}
for _name, (_alg, _n, _R, _kw, _g) in _DEVICE.items():
    DEVICE_CASES[_name] = (_alg, _n, _R, dict(_kw, device_shrink=False), _g)
    DEVICE_CASES[_name + "+dshrink"] = (_alg, _n, _R, dict(_kw, device_shrink=True), _g)


def _sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def record(case, evaluator=None):
    """One run of a case -> the recorded fields (evaluator None: the default GpuEvaluator)."""
    alg, n, R, kw, generations = case
    with A.Adversary(alg, n, R, seed=SEED, evaluator=evaluator, **kw) as adv:
        res = adv.search(generations=generations, want=WANT)
        state = json.dumps(adv.rng.bit_generator.state, sort_keys=True)
        out = {
            "generations": res.generations,
            "schedules_evaluated": res.schedules_evaluated,
            "history": [repr(float(h)) for h in res.history],
            "next_id": int(adv.next_id),
            "rng_state": hashlib.sha256(state.encode()).hexdigest(),
            "counterexamples": [{
                "inst_id": int(c.inst_id), "ho": _sha(c.ho), "crash": None if c.crash is None else _sha(c.crash),
                "init": _sha(c.init), "summary": _sha(c.summary), "check_point": int(c.check_point),
                "violated": list(c.violated), "omitted_links": int(c.omitted_links)} for c in res.counterexamples],
        }
        if evaluator is None and kw.get("device_shrink"):
            out["shrink_stats"] = {k: int(v) for k, v in adv.shrink_stats.items()}
    return out


def record_host(name):
    from oracle_eval import OracleEvaluator
    alg, n, R, kw, _ = HOST_CASES[name]
    return record(HOST_CASES[name], OracleEvaluator(alg, n, R, value_range=kw.get("values", 3)))


def record_device(name):
    return record(DEVICE_CASES[name])


def load():
    with open(PATH) as f:
        return json.load(f)


def _commit():
    """HEAD, refused unless round_amd/ is as committed there."""
    head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "round_amd"], text=True).strip()
    if dirty:
        raise SystemExit("round_amd/ differs from HEAD:\n" + dirty)
    return head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("host", "device", "all"), default="all")
    ap.add_argument("--out", default=PATH, help="file to write (sections not recorded are kept from the golden file)")
    ap.add_argument("--commit", default="", help="the commit of the tree, where it is no git checkout")
    a = ap.parse_args()
    commit = a.commit or _commit()
    doc = load() if os.path.exists(PATH) else {}
    if a.section in ("host", "all"):
        import oracle
        oracle.build()
    for section, cases, rec in (("host", HOST_CASES, record_host), ("device", DEVICE_CASES, record_device)):
        if a.section not in (section, "all"):
            continue
        out = {}
        for name in cases:
            first, second = rec(name), rec(name)
            if first != second:
                raise SystemExit(f"{section}/{name}: two runs differ, nothing written")
            out[name] = first
            print(section, name, first["generations"], "generations,", len(first["counterexamples"]), "found",
                  first.get("shrink_stats", ""), flush=True)
        doc[section] = {"commit": commit, "seed": SEED, "want": WANT, "cases": out}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
