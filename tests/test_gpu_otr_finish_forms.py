"""The W == 1 per-instance finish of the OTR kernels (finish_instance_w1, psg_device.hpp): the
digest total in lane 63, the output-presence bits (LaunchBits) and their two arms, the store
addresses. Seeded launches against the oracle: every instance's summary record, decision and
decide round, and the batch summary, across the sizes at which the finish's lanes change roles."""
import numpy as np
import pytest

from round_amd import psync

from gpu_support import (BEGIN, assert_run_equals_oracle, cmp_instances, cmp_summary, otr_alg, rec_tuple,
                         run_any, sharding_and_fetch)

pytestmark = pytest.mark.gpu

# lanes 12-15 and the quad gathers of the 24-byte summary (n = 13, 16), a partial wave, lane 63
# valid (n = 64) and invalid (the rest)
SIZES = [1, 2, 3, 13, 16, 33, 63, 64]
ROUNDS = [1, 4, 20]
COUNTS = [1, 7, 8, 9, 1000]  # around a queue chunk of 8
VALUES = [2, 64]
CAP = max(COUNTS)


def sample_of(count):
    return sorted({BEGIN, BEGIN + count - 1, BEGIN + count // 2} | {BEGIN + i for i in range(0, count, 97)})


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["otr", "otr2"])
def test_summary_digest_and_outputs_across_sizes(name, n, oracle_mod):
    """Summary records byte for byte, decisions and decide rounds element for element, the batch
    summary (digest sum, fail counts, termination histogram, decided, active, live) and the fetched
    process records, for every R, V and instance count."""
    for R in ROUNDS:
        for V in VALUES:
            with psync.GpuRound(otr_alg(name), n, R, seed=11, value_range=V, batch_capacity=CAP) as gr:
                for count in COUNTS:
                    osum, opi, orec = oracle_mod.run(gr.cfg, BEGIN, count, per_instance=True, records=True, threads=8)
                    assert_run_equals_oracle(gr, count, osum, opi, orec, sample_of(count))


@pytest.mark.parametrize("name,n", [("otr", 64), ("otr", 33), ("otr2", 13), ("otr2", 64)])
def test_each_presence_arm(name, n, oracle_mod):
    """One small launch through every route that changes which output arrays the kernel is given:
    the plain run (decision, decide round, summary: the ordinary arm), the fetch with process
    records (summary and records under an id list: the per-array arm), host-supplied initial
    values, and the fetch / sharded paths of sharding_and_fetch, each against the oracle."""
    cnt = 9
    alg = otr_alg(name)
    with psync.GpuRound(alg, n, 4, seed=8, batch_capacity=cnt) as gr:
        run_any(gr, oracle_mod, cnt, [BEGIN + i for i in range(cnt)])
        # host-supplied initial values (a.init): the same routes again
        init = np.random.default_rng(5).integers(1, gr.cfg.value_range + 1, (cnt, n), dtype=np.int32)
        gr.load_inputs(BEGIN, cnt, init)
        osum, opi, orec = oracle_mod.run(gr.cfg, BEGIN, cnt, init=init, per_instance=True, records=True, threads=8)
        assert_run_equals_oracle(gr, cnt, osum, opi, orec, [BEGIN + i for i in range(cnt)][::-1])
        cfg = gr.cfg
    # sharding_and_fetch runs [500, 500 + cnt) with seed 8 and 4 rounds: the configuration above
    fr = sharding_and_fetch(alg, n, cnt)
    osum, opi, orec = oracle_mod.run(cfg, 500, cnt, per_instance=True, records=True, threads=8)
    ids = sorted({500 + (7 * j) % cnt for j in range(min(cnt, 9))}, reverse=True)
    for j, inst in enumerate(ids):
        i = inst - 500
        got = [(int(r["decision"]), int(r["decision_round"]), int(r["halt_round"]), int(r["final_x"])) for r in fr[j]]
        assert got == [rec_tuple(r) for r in orec[i * n:(i + 1) * n]], inst
    with psync.GpuRound(alg, n, 4, seed=8, batch_capacity=cnt) as gr:
        s, pi = gr._ctx.run_batch_np(500, cnt)
        cmp_summary(s, osum, 4)
        cmp_instances(pi, opi)

