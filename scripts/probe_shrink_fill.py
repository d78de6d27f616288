#!/usr/bin/env python3
"""The shrink step's fill kernel as a write stream (DESIGN §5 "Shrinking on the device"): a random
base at n, R with a share 1 - keep of the links missing, then `--loads` psg_shrink_load calls of
`--count` LINK candidates each. Prints the bytes one load writes (count * R * n * W * 8) and the
wall time per load; run it under `rocprofv3 --kernel-trace --stats` for the kernel's own time
(`shrink_fill_kernel<W>`), bytes / that time = the achieved write rate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from round_amd import abi, psync, schedules as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--count", type=int, default=32768)
    ap.add_argument("--loads", type=int, default=20)
    ap.add_argument("--keep", type=float, default=0.75, help="density of the base's links")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ho = S.random_omission(rng, 1, a.rounds, a.n, a.keep)[0]
    init = rng.integers(1, 4, a.n, dtype=np.int32)
    with psync.GpuRound(psync.OTR(), a.n, a.rounds, batch_capacity=a.count) as g:
        ctx = g._ctx
        ctx.shrink_begin(ho, None, init)
        total = ctx.shrink_count(abi.PSG_SHRINK_LINK, 0)
        count = min(a.count, total)
        ctx.shrink_load(abi.PSG_SHRINK_LINK, 0, 0, count, 0)  # warm-up: the buffers are allocated here
        secs = []
        for k in range(a.loads):
            first = (k * count) % max(1, total - count + 1)
            t0 = time.perf_counter()
            ctx.shrink_load(abi.PSG_SHRINK_LINK, 0, first, count, 0)
            secs.append(time.perf_counter() - t0)
        links = ctx.population_links()
    per = a.rounds * a.n * S.words(a.n) * 8
    assert (links == a.rounds * a.n * a.n - total + 1).all()  # every candidate restores one link
    print(json.dumps({"n": a.n, "rounds": a.rounds, "candidates_per_load": count, "level_total": total, "keep": a.keep,
                      "bytes_per_load": count * per, "loads": a.loads,
                      "load_call_ms_median": round(1e3 * float(np.median(secs)), 4),
                      "load_call_ms_min": round(1e3 * min(secs), 4)}))


if __name__ == "__main__":
    main()
