// psg_lattice.hip — LatticeAgreement (lattice agreement over Set[Int]) on gfx950.
//
// Reference: example/LatticeAgreement.scala:32-68 (LatticeAgreementProcess): one closed
// Round[Lattice.T]. Lattice.T = Set[Int] is finitized as the subsets of {0..30}, an int32 bit mask
// (bit e = element e, bit 31 never set: every value is >= 0 and differs from PSG_NONE32); bottom
// is 0 and join is bitwise OR.
//   send    every process that has not halted broadcasts proposed (48-50);
//   update  mailbox M(p) = HO(p) & alive; cnt(p) = |{q in M(p) : proposed_q == proposed_p}|;
//           cnt > n/2: decide(proposed), decision = Some(proposed), active = false, exit (54-58);
//           else proposed = join(proposed, every mailbox value) (60). All reads from the pre-state.
// active is false exactly when the process has halted (57-58), so it is not stored.
// Processes are lanes, elements are bits, mailboxes are 64-bit masks. The round is bit-sliced over
// the elements on which the live senders disagree: with A = OR and C = AND of proposed over the
// live processes (two uniform words, one exchange), D = A & ~C. For e in D (a scalar bit loop)
// B_e = ballot(bit e of proposed) & alive; the join gets bit e iff M(p) & B_e is non-empty, and
// the senders equal to p are narrowed by EQ(p) &= (own bit e ? B_e : ~B_e) from EQ = alive; then
// cnt(p) = popc(M(p) & EQ(p)). An element outside D is held by every live process or by none: it
// changes neither a join nor a count. At most 31 steps instead of one per sender or per distinct
// value; for W > 1 the ballots of up to Grp::kFuse elements share one LDS exchange.
// Two exits before the loop: D == 0 (every live process holds one set, the usual state from
// round 1 or 2 on): no join, cnt = popc(M(p)); no live process: a check-only round that draws
// nothing (a skipped draw moves no other draw).
// Checks (the reference has TrivialSpec, 74: the problem's stated properties), with
// J = OR of the n initial values: slot 0 Safety (= the one invariant), 1 Invariant0, 2
// Comparability, 3 DownwardValidity, 4 UpwardValidity, 5 Irrevocability; Termination = every
// decision defined. variant 1 (test mutation): the threshold is n/4.
#include "psg_device.hpp"
#include "psg_kernels.hpp"

namespace psg {

// Check point c. Every formula is evaluated from the current state; the per-process witnesses are
// lane predicates, one fused exchange for all of them:
//   !(init ⊆ proposed ⊆ J) || (decided && decision != proposed)    Invariant0
//   decided && !(init ⊆ decision)                                   DownwardValidity
//   decided && !(decision ⊆ J)                                      UpwardValidity
//   old(decided) && !(decided && old(decision) == decision)         Irrevocability
// Comparability: a uniform loop over the distinct defined decisions d (usually one): a lane's
// decision is marked when it is neither a subset nor a superset of d, and one ballot at the end
// (taken only with two or more distinct decisions) collects the marks. ds: 64 W words of LDS.
template <int W>
PSG_DEV void lattice_check(Grp<W>& g, int32_t* ds, Checks& ck, int c, const Mask<W>& full, int32_t init, int32_t J,
                           int32_t proposed, uint32_t dec01, int32_t decision, uint32_t old01, int32_t old_decision) {
  const bool dec = dec01 != 0u;
  const bool pr[5] = {dec, ((init & ~proposed) | (proposed & ~J)) != 0 || (dec && decision != proposed),
                      dec && (init & ~decision) != 0, dec && (decision & ~J) != 0,
                      old01 != 0u && !(dec && old_decision == decision)};
  Mask<W> m[5];
  g.template ballots<5>(pr, m);
  const Mask<W>& Dm = m[0];
  bool comparable = true;
  if (many(Dm)) {
    if constexpr (W > 1) {
      ds[g.pid] = decision;
      __syncthreads();
    }
    Mask<W> rem = Dm;
    bool inc = false;  // this lane's decision is incomparable with some decision
    int distinct = 0;
    while (many(rem)) {
      const int32_t d = g.bcast(decision, ds, mfirst(rem));
      rem = mandn(rem, g.ballot(dec && decision == d));
      inc = inc || (dec && (decision & ~d) != 0 && (d & ~decision) != 0);
      ++distinct;
    }
    if (distinct > 1) comparable = !g.any(inc);
  }
  const bool inv = !many(m[1]) && comparable;
  const uint32_t fb = fbit(inv, 0) | fbit(inv, 1) | fbit(comparable, 2) | fbit(!many(m[2]), 3) | fbit(!many(m[3]), 4) |
                      fbit(!many(m[4]), 5);
  ck.record(fb, meq(Dm, full), c, g.lane);
}

// Kernel body; SH: the Spec hook (NoHook in psg_device.hpp).
template <int W, bool XHO, class SH = NoHook, bool TR = true>
PSG_DEV void lattice_body(const KArgs& a) {
  __shared__ BlockCounters bc;
  __shared__ uint64_t xb[Grp<W>::kXb];
  __shared__ int32_t crl[W > 1 ? 64 * W : 1];
  __shared__ int64_t red[2 * W];
  __shared__ int32_t ds[W > 1 ? 64 * W : 1];
  counters_init(&bc);
  __syncthreads();
  Grp<W> g;
  grp_setup(g, a, xb, red);
  const int grp = W == 1 ? (int)(threadIdx.x >> 6) : 0;
  const int n = a.n;
  const int thr = a.variant == 1 ? n / 4 : n / 2;  // LatticeAgreement.scala:54 (variant 1: mutation)
  const Mask<W> full = mfull<W>(n);
  constexpr int kB = W == 1 ? 1 : Grp<W>::kFuse;  // elements per ballot exchange

  InstanceQueue<W, 0, W == 1 ? PSG_QUEUE_CHUNK_LANE : 0> Q;  // dynamic instance distribution (psg_device.hpp)
  for (uint64_t i = Q.take(a); i != Q.kDone; i = Q.take(a)) {
    Inst<W, XHO> in;
    in.begin(g, a, i, crl);
    Sched<W, XHO>& sc = in.sc;
    // LatticeAgreementProcess state after init(io) (LatticeAgreement.scala:39-43); lanes past n hold 0
    const int32_t init = in.x0(g, a, i, PSG_ALG_LATTICE) & 0x7FFFFFFF;
    const int32_t J = (int32_t)g.gor((uint32_t)init);  // the join of every initial value
    int32_t proposed = init, decision = PSG_NONE32;
    uint32_t dec01 = 0;  // decision.isDefined == halted (56-58)
    int32_t dec_round = -1;
    Checks ck;
    ck.reset();
    typename SH::template State<W> sh(g, grp, n);  // fused Spec evaluation state (NoHook: empty)
    if constexpr (!SH::kFused) lattice_check<W>(g, ds, ck, 0, full, init, J, proposed, dec01, decision, 0u, PSG_NONE32);
    auto trace = [&](int cp, int32_t hs) {
      emit_state<W, SH>(sh, g, a, i, cp, proposed, (int32_t)dec01, decision, 0, 0, 0, 0, 0, hs, false);
    };
    if (tracing<SH, TR>(a)) trace(0, n);

    for (int k = 0; k < a.R; ++k) {
      const uint32_t old01 = dec01;
      const int32_t old_decision = decision;
      const bool live = g.valid && dec01 == 0u;
      const Mask<W> act = g.ballot_any(live);
      int32_t hs = n;  // |mailbox| of this round (Spec field HOSIZE)
      if (many(act)) {
        // A | ~C << 32 over the live processes in one exchange
        const uint32_t lo = wave_or(live ? (uint32_t)proposed : 0u);
        const uint32_t hi = wave_or(live ? ~(uint32_t)proposed & 0x7FFFFFFFu : 0u);
        const uint64_t ac = rfl64((uint64_t)g.template cross64<3>((int64_t)(((uint64_t)hi << 32) | lo)));
        uint32_t rem = (uint32_t)ac & (uint32_t)(ac >> 32);  // D: some live process holds e, some does not
        Mask<W> goodS;
        const bool good = sc.good_round(k, g.lane, a.R, goodS);
        Mask<W> CB = mzero<W>(), CN = mzero<W>();
        if (sc.crash_on) in.cs.sets(g, k, CB, CN);
        const Mask<W> M = mand(ho_select<W, XHO>(sc, k, g.pid, good, goodS, CB, CN), act);
        hs = live ? mpopc(M) : n;
        uint32_t jn = 0;     // join of the mailbox, on the elements of D
        Mask<W> EQ = M;      // the mailbox senders whose set equals proposed, narrowed per element
        while (rem != 0u) {  // (uniform) not taken when every live process holds one set
          uint32_t e[kB];
          bool pr[kB];
#pragma unroll
          for (int j = 0; j < kB; ++j) {  // past the last element of D: bit 31, set in no value
            e[j] = rem != 0u ? (uint32_t)__builtin_ctz(rem) : 31u;
            rem &= rem - 1u;
            pr[j] = live && (((uint32_t)proposed >> e[j]) & 1u) != 0u;
          }
          Mask<W> B[kB];
          g.template ballots<kB>(pr, B);
#pragma unroll
          for (int j = 0; j < kB; ++j) {
            if (j == 0 || e[j] != 31u) {
              const bool own = (((uint32_t)proposed >> e[j]) & 1u) != 0u;
              uint64_t hit = 0;
#pragma unroll
              for (int w = 0; w < W; ++w) {
                hit |= M.w[w] & B[j].w[w];
                EQ.w[w] &= own ? B[j].w[w] : ~B[j].w[w];
              }
              jn |= hit != 0ull ? 1u << e[j] : 0u;
            }
          }
        }
        const int32_t cnt = mpopc(EQ);
        const bool decide = live && cnt > thr;
        decision = decide ? proposed : decision;
        dec_round = decide ? k : dec_round;
        dec01 |= decide ? 1u : 0u;
        proposed = (live && !decide) ? proposed | (int32_t)jn : proposed;
      }
      if constexpr (!SH::kFused)
        lattice_check<W>(g, ds, ck, k + 1, full, init, J, proposed, dec01, decision, old01, old_decision);
      if (tracing<SH, TR>(a)) trace(k + 1, hs);
    }
    // decide and exitAtEndOfRound come together (55-58): decision_round == halt_round
    finish_instance<W>(g, a, i, hook_checks<SH>(sh, ck), hook_slots<SH>(kLatticeChecks), dec01 ? decision : 0, dec_round,
                       dec_round, proposed, &bc);
  }
  __syncthreads();
  counters_flush(&bc, a.counters, hook_slots<SH>(kLatticeChecks), a.R);
}

template <int W, bool XHO, class SH = NoHook, bool TR = true>
__global__ void __launch_bounds__(Geometry<W>::kThreads) lattice_kernel(KArgs a) {
  lattice_body<W, XHO, SH, TR>(a);
}

#ifndef PSG_FUSED_MODULE  // host launchers (not part of a fused Spec module)
template <int W>
static hipError_t launch_w(const KArgs& a, int grid, hipStream_t s) {
  if (a.ho_in) return launch_grp<W>(lattice_kernel<W, true>, a, grid, s);
  if (a.trace) return launch_grp<W>(lattice_kernel<W, false>, a, grid, s);
  return launch_grp<W>(lattice_kernel<W, false, NoHook, false>, a, grid, s);
}

hipError_t launch_lattice(const KArgs& a, int W, int grid, hipStream_t s) {
  return with_w(W, hipErrorInvalidValue, [&](auto w) { return launch_w<w()>(a, grid, s); });
}

const void* lattice_kernel_ptr(int W) {
  return with_w(W, (const void*)nullptr, [](auto w) { return (const void*)lattice_kernel<w(), false, NoHook, false>; });
}
#endif  // PSG_FUSED_MODULE

}  // namespace psg
