// psg_tpc.hip — TwoPhaseCommit (atomic commitment, fixed coordinator) on gfx950.
//
// Reference: example/TwoPhaseCommit.scala:15-79 (TpcProcess): three closed Round[Boolean]s.
// coord = io.coord is the same process for every process of an instance (the Axiom
// "well-coordinated", TwoPhaseCommit.scala:87): a.param, uniform per launch. vote = io.canCommit
// never changes; decision: Option[Boolean] is PSG_NONE32 / 0 / 1.
//   R0  the coordinator broadcasts a placeholder, update does nothing (30-39): no state changes,
//       so no HO set is drawn;
//   R1  every process sends vote to coord; the coordinator's mailbox is HO(coord) (nobody has
//       halted yet); with |mailbox| == n and every vote in it true its decision becomes
//       Some(true), else Some(false) (41-58). Only HO(coord) is read;
//   R2  the coordinator broadcasts decision.get; a process with coord in HO(p) takes that value;
//       every process then calls decide(decision) and exits (60-76). Only bit coord of HO(p) is
//       read. decision.get on None (63) is unreachable in lockstep: the coordinator executed R1 of
//       the same phase, which always leaves its decision defined.
// Every process halts in round 2, so rounds >= 3 take no step and draw nothing; their check
// points are still evaluated. A skipped draw moves no other draw (the Philox
// counter is (instance, round, pid, word)).
// Results: decide(Some(b)) is a decision (value b, round 2), decide(None) — "coordinator
// suspected" — is not (value PSG_NONE32, round -1); final_x = vote.
// Spec (TwoPhaseCommit.scala:89-108), on the state variable decision: slot 0 Safety (= the one
// invariant), 1 Invariant0, 2 UniformAgreement, 3 Validity; Termination = every decision defined.
// variant 1 (test mutation): the coordinator drops the mailbox.size == n conjunct (51).
#include "psg_device.hpp"
#include "psg_kernels.hpp"

namespace psg {

// Kernel body; SH: the Spec hook (NoHook in psg_device.hpp).
template <int W, bool XHO, class SH = NoHook, bool TR = true>
PSG_DEV void tpc_body(const KArgs& a) {
  __shared__ BlockCounters bc;
  __shared__ uint64_t xb[Grp<W>::kXb];
  __shared__ int32_t crl[W > 1 ? 64 * W : 1];
  __shared__ int64_t red[2 * W];
  counters_init(&bc);
  __syncthreads();
  Grp<W> g;
  grp_setup(g, a, xb, red);
  const int grp = W == 1 ? (int)(threadIdx.x >> 6) : 0;
  const int n = a.n;
  const int c = a.param;  // coord (0 <= c < n: psg_create)
  const Mask<W> full = mfull<W>(n);
  // |mailbox| is state only for a trace or a fused Spec that reads it: then R0's sets are drawn too
  const bool hs_read = SH::kFused ? ((SH::kFields >> PSG_FIELD_HOSIZE) & 1u) != 0u
                                  : (TR && a.trace != nullptr && ((a.trace_fields >> PSG_FIELD_HOSIZE) & 1u));

  InstanceQueue<W, 0, W == 1 ? PSG_QUEUE_CHUNK_LANE : 0> Q;  // dynamic instance distribution (psg_device.hpp)
  for (uint64_t i = Q.take(a); i != Q.kDone; i = Q.take(a)) {
    Inst<W, XHO> in;
    in.begin(g, a, i, crl);
    Sched<W, XHO>& sc = in.sc;
    // TpcProcess state after init(io) (TwoPhaseCommit.scala:22-27); host inputs: nonzero = true
    const int32_t vote = in.x0(g, a, i, PSG_ALG_TPC) != 0 ? 1 : 0;
    int32_t decision = PSG_NONE32;
    int32_t cdec = 0;  // the coordinator's decision.get after R1 (uniform)
    int32_t dec_val = PSG_NONE32, dec_round = -1, halt_round = -1;
    const Mask<W> noB = g.ballot(vote == 0);  // the no-voters: constant per instance
    Checks ck;
    ck.reset();
    typename SH::template State<W> sh(g, grp, n);  // fused Spec evaluation state (NoHook: empty)
    // Invariant0 = Validity && UniformAgreement (TwoPhaseCommit.scala:94-95, 102, 104)
    auto check = [&](int cp) {
      const bool pr[2] = {decision == 1, decision == 0};
      Mask<W> m[2];
      g.template ballots<2>(pr, m);
      const bool validity = !many(m[0]) || !many(noB);  // some Some(true) ==> every vote
      const bool agree = !(many(m[0]) && many(m[1]));   // two defined decisions differ
      const bool inv = validity && agree;
      ck.record(fbit(inv, 0) | fbit(inv, 1) | fbit(agree, 2) | fbit(validity, 3), meq(mor(m[0], m[1]), full), cp, g.lane);
    };
    if constexpr (!SH::kFused) check(0);
    auto trace = [&](int cp, int32_t hs) {
      emit_state<W, SH>(sh, g, a, i, cp, vote, decision != PSG_NONE32 ? 1 : 0, decision, 0, 0, 0, vote, 0, hs, false);
    };
    if (tracing<SH, TR>(a)) trace(0, n);

    // HO(pid) of round k (seeded: drawn; explicit: read)
    auto ho_of = [&](const int k, const int pid) {
      Mask<W> goodS;
      const bool good = sc.good_round(k, g.lane, a.R, goodS);
      Mask<W> CB = mzero<W>(), CN = mzero<W>();
      if (sc.crash_on) in.cs.sets(g, k, CB, CN);
      return ho_select<W, XHO>(sc, k, pid, good, goodS, CB, CN);
    };
    // round k = RS of the first phase (compile time: each slot's step specialized); nobody has
    // halted before round 2, so every process sends and the coordinator is alive
    auto round = [&](const int k, auto RSc) {
      constexpr int RS = decltype(RSc)::value;
      int32_t hs = n;  // |mailbox| of this round (Spec field HOSIZE)
      if constexpr (RS == 0) {  // R0 (TwoPhaseCommit.scala:30-39)
        if (hs_read) hs = mtest(ho_of(k, g.pid), c) ? 1 : 0;
      } else if constexpr (RS == 1) {  // R1 (TwoPhaseCommit.scala:41-58)
        Mask<W> Mc = ho_of(k, c);  // every lane forms the coordinator's set: uniform without an exchange
#pragma unroll
        for (int w = 0; w < W; ++w) Mc.w[w] = rfl64(Mc.w[w]);
        const int size = mpopc(Mc);
        const bool all_yes = !many(mand(noB, Mc));
        cdec = ((a.variant == 1 || size == n) && all_yes) ? 1 : 0;
        if (g.pid == c) decision = cdec;
        hs = g.pid == c ? size : 0;
      } else {  // R2 (TwoPhaseCommit.scala:60-76)
        const bool rcv = mtest(ho_of(k, g.pid), c);
        hs = rcv ? 1 : 0;
        if (g.valid) {
          decision = rcv ? cdec : decision;
          dec_val = decision;  // callback.decide(decision)
          dec_round = decision != PSG_NONE32 ? k : -1;
          halt_round = k;
        }
      }
      if constexpr (!SH::kFused) check(k + 1);
      if (tracing<SH, TR>(a)) trace(k + 1, hs);
    };
    round(0, Slot<0>{});
    if (1 < a.R) round(1, Slot<1>{});
    if (2 < a.R) round(2, Slot<2>{});
    for (int k = 3; k < a.R; ++k) {  // everyone has halted: check-only rounds
      if constexpr (!SH::kFused) check(k + 1);
      if (tracing<SH, TR>(a)) trace(k + 1, n);
    }
    finish_instance<W>(g, a, i, hook_checks<SH>(sh, ck), hook_slots<SH>(kTpcChecks), dec_val, dec_round, halt_round, vote, &bc);
  }
  __syncthreads();
  counters_flush(&bc, a.counters, hook_slots<SH>(kTpcChecks), a.R);
}

template <int W, bool XHO, class SH = NoHook, bool TR = true>
__global__ void __launch_bounds__(Geometry<W>::kThreads) tpc_kernel(KArgs a) {
  tpc_body<W, XHO, SH, TR>(a);
}

#ifndef PSG_FUSED_MODULE  // host launchers (not part of a fused Spec module)
template <int W>
static hipError_t launch_w(const KArgs& a, int grid, hipStream_t s) {
  if (a.ho_in) return launch_grp<W>(tpc_kernel<W, true>, a, grid, s);
  if (a.trace) return launch_grp<W>(tpc_kernel<W, false>, a, grid, s);
  return launch_grp<W>(tpc_kernel<W, false, NoHook, false>, a, grid, s);
}

hipError_t launch_tpc(const KArgs& a, int W, int grid, hipStream_t s) {
  return with_w(W, hipErrorInvalidValue, [&](auto w) { return launch_w<w()>(a, grid, s); });
}

const void* tpc_kernel_ptr(int W) {
  return with_w(W, (const void*)nullptr, [](auto w) { return (const void*)tpc_kernel<w(), false, NoHook, false>; });
}
#endif  // PSG_FUSED_MODULE

}  // namespace psg
