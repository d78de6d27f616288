// psg_otr_packed.hip — OTR for n <= 32 with G = 64 / P instances per wave64 (psg_subwave.hpp).
//
// The same algorithm, schedule, checks and outputs as otr_kernel<1, false, false, NoHook, false>
// (psg_otr.hip), bit for bit: psg_config.pack = 1 selects this kernel for psg_run_batch without
// an explicit schedule (psg_pack_width). Reference: example/Otr.scala:13-128.
// Lane l is process l % P of sub-group l / P; a wave takes up to G consecutive batch rows at a
// time. Sets of processes are per-lane 32-bit masks in sub-group-local bit positions. A lane
// draws the Philox words of its own instance id: the counters are Sched<1>'s, (inst, round,
// pid | stream << 16), of which only the low dword of each 64-bit word is used (n <= 32). A
// sub-group without a row, and a sub-group whose processes have all halted, run the wave's
// instructions predicated off: their lanes are "halted", so they neither draw nor update, and
// nothing is stored or counted for a sub-group without a row.
#include "psg_subwave.hpp"
#include "psg_kernels.hpp"

namespace psg {

template <int P>
__global__ void __launch_bounds__(256) otr_packed_kernel(KArgs a) {
  constexpr int G = 64 / P;
  __shared__ BlockCounters bc;
  counters_init(&bc);
  __syncthreads();
  Sub<P> s;
  s.setup();
  const int n = a.n, R = a.R;
  const int thr = a.variant == 1 ? n / 2 : (2 * n) / 3;  // Otr.scala:64, 67 (variant 1: mutation)
  const int sthr = (2 * n) / 3;                          // 2*n/3 in the Spec (Otr.scala:101)
  const uint32_t full = sub_full(n);
  const bool in_n = s.pid < n;
  const bool crash_on = a.crash_fmax >= 0;
  const int good_min = a.good_min >= 0 ? a.good_min : (2 * n) / 3;
  const uint32_t drop = a.drop_log2;
  const uint32_t seed_lo = (uint32_t)a.seed, seed_hi = (uint32_t)(a.seed >> 32);

  // per-lane running sums over the wave's instances, reduced once per wave at the end
  uint64_t dig_t = 0, act_t = 0, live_t = 0;
  uint32_t dec_t = 0;   // decided processes
  uint32_t fail_t = 0;  // lane s < kOtrChecks: instances in which slot s failed

  RowQueue<G> Q;
  uint64_t base;
  int cnt;
  while (Q.take(a, base, cnt)) {
    const bool has_row = s.sub < cnt;  // else an idle sub-group: no row index is used
    const bool valid = has_row && in_n;
    const uint64_t row = base + (uint64_t)s.sub;
    const uint64_t inst = has_row ? instance_id(a, row) : 0ull;
    const uint32_t valid01 = valid ? 1u : 0u;

    // initial value: the staged row, else 1 + mulhi32(w, V) of the process's init word
    int32_t x0 = 0;
    if (valid) {
      if (a.init) x0 = a.init[init_row(a, row, inst) * (uint64_t)n + (uint64_t)s.pid];
      else x0 = 1 + (int32_t)mulhi32((uint32_t)rword(a.seed, inst, ROUND_INIT, (uint32_t)s.pid, 0), (uint32_t)a.V);
    }
    // crash round of this process (Sched::setup), -1 = correct
    int32_t cr = -1;
    if (crash_on && valid) {
      const U4 o = philox10((uint32_t)inst, (uint32_t)(inst >> 32), ROUND_CRASH, PID_GLOBAL, seed_lo, seed_hi);
      cr = Sched<1>::crash_of(a, inst, (uint32_t)s.pid, (uint64_t)o.x | ((uint64_t)o.y << 32),
                              (uint64_t)o.z | ((uint64_t)o.w << 32));
    }
    // Good rounds (Sched::prep_good): lane pid p of a sub-group draws round gbase + p of its
    // instance's PID_GLOBAL stream, P rounds per pass; the flags become the sub-group's slice of
    // one ballot, and round k's common set is read from lane k - gbase of the sub-group.
    int gbase = 0;
    uint32_t gbits = 0, gset = full;
    auto prep_good = [&](int kbase) {
      gbase = kbase;
      const int kk = kbase + s.pid;
      bool gd = false;
      uint32_t gs = full;
      if (has_row && kk < R) {
        WordStream ws(a.seed, inst, (uint32_t)kk, PID_GLOBAL);
        gd = (uint32_t)ws.word(0) < a.good_p32;
        if (gd && drop > 0) {
          uint32_t m = ~0u;
          for (uint32_t i = 0; i < drop; ++i) m &= (uint32_t)ws.word(1u + i);
          gs = full & ~m;
          if (__builtin_popcount(gs) <= good_min) gs = full;
        }
      }
      gset = gs;
      gbits = s.ballot(gd);
    };
    if (a.good_p32 != 0) prep_good(0);

    // OtrProcess state after init(io) (Otr.scala:15-26); flags are 0/1 lane words. Lanes that
    // hold no process are halted from the start.
    int32_t x = x0, decision = -1, after = a.param;
    uint32_t dec01 = 0, halted01 = 1u - valid01;
    int32_t dec_val = 0, dec_round = -1, halt_round = -1;
    int32_t live = 0;  // sub-group-uniform: the last round in which some process stepped, plus one
    // "x / decision is an initial value of this instance": an exact compare against the
    // sub-group's distinct initial values, taken again whenever the values change. lead0 holds
    // the first holder of each distinct initial value; the walks below run until every sub-group
    // of the wave is through (one whose mask is empty reads process 0's value once more).
    uint32_t lead0 = 0;
    for (uint32_t rem = s.ballot(valid); __builtin_amdgcn_ballot_w64(rem != 0u) != 0ull;) {
      const int j = rem != 0u ? (int)__builtin_ctz(rem) : 0;
      const uint32_t E = s.ballot(valid && x0 == s.bcast(x0, j));  // (holds j when rem != 0: rem shrinks)
      lead0 |= rem != 0u ? 1u << j : 0u;
      rem &= ~E;
    }
    uint32_t xin01 = 0, din01 = 0;
    auto probe_init = [&]() {
      uint32_t xi = 0, di = 0;
      for (uint32_t rem = lead0; __builtin_amdgcn_ballot_w64(rem != 0u) != 0ull; rem &= rem - 1u) {
        const int32_t v = s.bcast(x0, rem != 0u ? (int)__builtin_ctz(rem) : 0);
        xi |= eq01(x, v);
        di |= eq01(decision, v);
      }
      xin01 = xi;
      din01 = di;
    };
    probe_init();

    SubChecks ck;
    ck.reset();
    // Spec at check point c (otr_check_general's formulas, psg_otr.hip; Otr.scala:95-120), every
    // result sub-group-uniform. The four universally quantified parts are per-process witness
    // bits; one wave ballot of "some bit set" settles them for all sub-groups when there is no
    // witness in the wave, else each takes its own ballot.
    auto check = [&](int c, bool has_old, uint32_t old01, int32_t old_decision) {
      const uint32_t w_irr = has_old ? old01 & (1u - (dec01 & eq01(old_decision, decision))) : 0u;  // Irrevocability
      // Settled state (otr_check_settled), taken when every instance of the wave is in it: every
      // process decided, every decision equal to process 0's and an initial value, every x an
      // initial value, no Irrevocability witness. Then D = full, d0 is process 0's decision and
      // keepInit, Validity, Agreement and Irrevocability hold, so the formulas below reduce to
      // Invariant0 = (cnt > 2n/3), Invariant1 = (cnt == n), Invariant2, Safety, Integrity and
      // Termination hold, with the vote count taken at d0: the same values in fewer instructions
      // (most check points of a run are in this state).
      {
        const int32_t p0 = s.bcast(decision, 0);
        const uint32_t u = (valid01 & ((1u - dec01) | ne01(decision, p0) | (1u - din01) | (1u - xin01))) | w_irr;
        if (__builtin_amdgcn_ballot_w64(u != 0u) == 0ull) {
          const int vc = __builtin_popcount(s.ballot(valid && x == p0));
          ck.record(fbit(vc > sthr, 1) | fbit(vc == n, 2), true, c, s.pid);
          return;
        }
      }
      const uint32_t D = s.ballot(dec01 != 0u);  // (dec01 is 0 on lanes without a process)
      const bool anyD = D != 0u;
      const int32_t dfirst = s.bcast(decision, anyD ? (int)__builtin_ctz(D) : 0);
      const int32_t d0 = anyD ? dfirst : 0;
      const bool term = D == full;
      const uint32_t w_keep = valid01 & (1u - xin01);                                        // keepInit
      const uint32_t w_val = dec01 & (1u - din01);                                           // Validity
      const uint32_t w_same = dec01 & ne01(decision, d0);                                    // Agreement
      bool keep = true, validity = true, same = true, irrev = true;
      if (__builtin_amdgcn_ballot_w64((w_keep | w_val | w_same | w_irr) != 0u) != 0ull) {
        keep = s.ballot(w_keep != 0u) == 0u;
        validity = s.ballot(w_val != 0u) == 0u;
        same = s.ballot(w_same != 0u) == 0u;
        irrev = s.ballot(w_irr != 0u) == 0u;
      }
      // the vote count: of d0 once someone decided, else of process 0's x (read only as cnt == n)
      const int32_t x_0 = s.bcast(x, 0);
      const int32_t ref = anyD ? d0 : x_0;
      const int vc = __builtin_popcount(s.ballot(valid && x == ref));
      const bool condv = !anyD || same;
      const bool e0 = condv && vc > sthr;
      const bool e1 = condv && vc == n;
      const bool d0in = same && validity;  // all decisions equal d0 and are initial values
      const bool inv0 = (!anyD || e0) && keep;
      const bool inv1 = e1 && keep;
      const bool inv2 = term && d0in;
      const bool integrity = !anyD || d0in;
      const uint32_t fb = fbit(inv0 || inv1 || inv2, 0) | fbit(inv0, 1) | fbit(inv1, 2) | fbit(inv2, 3) |
                          fbit(same, 4) | fbit(validity, 5) | fbit(integrity, 6) | fbit(irrev, 7);
      ck.record(fb, term, c, s.pid);
    };
    check(0, false, 0u, -1);

    for (int k = 0; k < R; ++k) {
      const uint32_t old01 = dec01;
      const int32_t old_decision = decision;
      // Some process of the wave still steps; once none does, only the check points remain
      // (the state, the pre-round state included, is final).
      if (__builtin_amdgcn_ballot_w64(halted01 == 0u) != 0ull) {
        const uint32_t act = s.ballot(halted01 == 0u);  // not-yet-halted senders of this instance
        live = act != 0u ? k + 1 : live;
        bool good = false;
        uint32_t goodS = full;
        if (a.good_p32 != 0) {
          if (k - gbase >= P) prep_good(k);
          const int off = k - gbase;
          good = ((gbits >> off) & 1u) != 0u;
          goodS = (uint32_t)s.bcast((int32_t)gset, off);
        }
        uint32_t CB = 0, CN = 0;
        if (crash_on) {  // crashed before round k: 0 <= cr < k, one unsigned compare (cr = -1: correct)
          CB = s.ballot((uint32_t)cr < (uint32_t)k);
          CN = s.ballot(cr == k);
        }
        // Settled instance: every live process has decided d and holds x = d. Then every mailbox
        // holds only d, mmor is d and a mailbox above the threshold re-decides the d it holds
        // (Otr.scala:63-73): no x, decision or decided changes whatever the HO sets are, and only
        // `after` counts down. Its HO sets are not drawn (an empty HO set: no update), as in
        // psg_otr.hip; the schedule is a pure function of (instance, round, pid), so no other
        // draw moves.
        const int32_t dl = s.bcast(decision, act != 0u ? (int)__builtin_ctz(act) : 0);
        const bool unsettled = s.ballot(halted01 == 0u && !(dec01 != 0u && decision == dl && x == dl)) != 0u;
        // HO(p) of this lane's process (Sched::draw + assemble): words j < drop are the drop
        // words, word `drop` is the crash round's survival word. A halted lane draws nothing.
        uint32_t ho = 0;
        if (halted01 == 0u && unsettled) {
          const bool crash = crash_on && CN != 0u;
          uint32_t dm = ~0u, hf = ~0u;
          const uint32_t j0 = good ? drop : 0u;
          const uint32_t j1 = crash ? drop + 1u : (good ? 0u : drop);
          for (uint32_t si = j0 >> 1; 2 * si < j1; ++si) {
            const U4 o = philox10((uint32_t)inst, (uint32_t)(inst >> 32), (uint32_t)k, (uint32_t)s.pid + (si << 16),
                                  seed_lo, seed_hi);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const uint32_t j = 2 * si + (uint32_t)h;
              const uint32_t word = h ? o.z : o.x;  // the low dword of x | y << 32, z | w << 32
              if (j < j0 || j >= j1) continue;
              if (j < drop) dm &= word;
              else hf = word;
            }
          }
          uint32_t b = good ? goodS : (drop > 0 ? full & ~dm : full);
          if (crash_on) b &= ~(CB | (CN & ~hf));
          if (a.self_bit) b |= 1u << s.pid;
          if (a.ho_min >= 0 && __builtin_popcount(b) <= a.ho_min) b = full;
          ho = b;
        }
        // mailbox: broadcast(x) from every alive sender in HO(p)
        const uint32_t M = ho & act;
        const int32_t msize = __builtin_popcount(M);
        const uint32_t upd = (1u - halted01) & gt01(msize, thr);
        if (__builtin_amdgcn_ballot_w64(upd != 0u) != 0ull) {
          // mmor: max multiplicity, ties -> smaller value (OtrExample.scala:67-75), as one 64-bit
          // key count << 32 | v ^ 0x7FFFFFFF per lane. The walk visits each distinct value of the
          // instance's alive senders once (rem: senders whose value is still to come), until
          // every sub-group of the wave is through; a sub-group that is through meets process
          // 0's value again, with the key it already has.
          const int32_t xv = x ^ 0x7FFFFFFF;
          uint64_t best = (uint64_t)(uint32_t)(INT32_MAX ^ 0x7FFFFFFF);  // count 0, v = INT32_MAX
          for (uint32_t rem = act; __builtin_amdgcn_ballot_w64(rem != 0u) != 0ull;) {
            const int32_t kv = s.bcast(xv, rem != 0u ? (int)__builtin_ctz(rem) : 0);
            const uint32_t E = s.ballot(in_n && xv == kv);  // (holds the sender read when rem != 0: rem shrinks)
            rem &= ~E;
            const uint64_t key = ((uint64_t)(uint32_t)__builtin_popcount(M & E) << 32) | (uint32_t)kv;
            best = key > best ? key : best;
          }
          const int32_t best_c = (int32_t)(best >> 32);
          const int32_t best_v = (int32_t)((uint32_t)best ^ 0x7FFFFFFFu);
          // x = mmor; decide on > 2n/3 copies, callback only the first time (Otr.scala:64-73)
          x = upd ? best_v : x;
          const uint32_t newdec = upd & gt01(best_c, thr);
          const uint32_t first = newdec & (1u - dec01);
          dec_val = first ? best_v : dec_val;
          dec_round = first ? k : dec_round;
          decision = newdec ? best_v : decision;
          dec01 |= newdec;
          probe_init();
        }
        // after -= 1 once decided; exitAtEndOfRound when it reaches 0 (Otr.scala:75-80)
        const uint32_t ad = (1u - halted01) & dec01;
        after -= (int32_t)ad;
        const uint32_t h = ad & gt01(1, after);
        halt_round = h ? k : halt_round;
        halted01 |= h;
      }
      check(k + 1, true, old01, old_decision);
    }

    // finish (finish_instance, byte for byte)
    const bool decided = dec_round >= 0;
    const uint64_t d = valid ? proc_digest(s.pid, dec_val, dec_round, halt_round, x) : 0ull;
    const uint64_t dig = s.sum64(d);
    const uint32_t nd = (uint32_t)__builtin_popcount(s.ballot(valid && decided));
    const bool lead = has_row && s.pid == 0;
    dig_t += d;
    act_t += valid ? (uint64_t)(uint32_t)(halt_round >= 0 ? halt_round + 1 : R) : 0ull;
    live_t += lead ? (uint64_t)(uint32_t)live : 0ull;
    dec_t += (valid && decided) ? 1u : 0u;
    if (valid) {
      const uint64_t off = row * (uint64_t)n + (uint64_t)s.pid;
      if (a.out_decision) a.out_decision[off] = dec_val;
      if (a.out_dround) a.out_dround[off] = decided ? (uint8_t)dec_round : (uint8_t)0xFF;
      if (a.out_rec) {
        psg_process_record r;
        r.decision = dec_val;
        r.decision_round = dec_round;
        r.halt_round = halt_round;
        r.final_x = x;
        a.out_rec[off] = r;
      }
    }
    // the 24-byte psg_instance_summary: lane pid 0 the digest (bytes 0-7); lanes pid 0..2 their
    // four first_fail bytes (bytes 8-19); lane pid 3 term_round, n_checks, n_decided (bytes 20-23)
    static_assert(PSG_MAX_CHECKS == 12 && sizeof(psg_instance_summary) == 24, "summary record layout");
    if (has_row && s.pid < 4) {
      if (a.out_inst) {
        uint8_t* o = reinterpret_cast<uint8_t*>(a.out_inst + row);
        if (s.pid == 0) *reinterpret_cast<uint64_t*>(o) = dig;
        const uint32_t tail = ((uint32_t)ck.term & 0xFFu) | ((uint32_t)kOtrChecks << 8) | (nd << 16);
        *reinterpret_cast<uint32_t*>(o + 8 + 4 * s.pid) = s.pid < 3 ? ck.ffw : tail;
      }
      if (s.pid == 0) atomicAdd(&bc.hist[ck.term == (int32_t)PSG_NEVER ? R + 1 : ck.term], 1u);
    }
#pragma unroll
    for (int slot = 0; slot < kOtrChecks; ++slot) {
      const uint32_t c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(lead && ((ck.ever >> slot) & 1u) != 0u));
      fail_t += s.lane == slot ? c : 0u;
    }
  }

  Grp<1> g1;
  const uint64_t dig_w = g1.wave_sum64(dig_t), act_w = g1.wave_sum64(act_t), live_w = g1.wave_sum64(live_t);
  const uint32_t dec_w = Grp<1>::wave_sum32(dec_t);
  if (s.lane < kOtrChecks && fail_t) atomicAdd(&bc.fail[s.lane], fail_t);
  if (s.lane == 0) {
    atomicAdd(&bc.decided, dec_w);
    atomicAdd(&bc.digest, (unsigned long long)dig_w);
    atomicAdd(&bc.active, (unsigned long long)act_w);
    atomicAdd(&bc.live, (unsigned long long)live_w);
  }
  __syncthreads();
  counters_flush(&bc, a.counters, kOtrChecks, R);
}

// Blocks of 256 threads = 4 waves x G rows; grid = the kernel's own resident blocks at most.
template <int P>
static hipError_t launch_p(const KArgs& a, hipStream_t s) {
  static const int resident = [] {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)otr_packed_kernel<P>, 256, 0);
    return (per_cu < 1 ? 1 : per_cu) * (cus < 1 ? 1 : cus);
  }();
  constexpr uint64_t rows = 4 * (64 / P);
  const uint64_t want = (a.count + rows - 1) / rows;
  const int grid = (int)(want < (uint64_t)resident ? (want < 1 ? 1 : want) : (uint64_t)resident);
  hipLaunchKernelGGL(otr_packed_kernel<P>, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

// G: psg_pack_width(PSG_ALG_OTR, a.n), 2..16
hipError_t launch_otr_packed(const KArgs& a, int G, hipStream_t s) {
  switch (G) {
    case 16: return launch_p<4>(a, s);
    case 8: return launch_p<8>(a, s);
    case 4: return launch_p<16>(a, s);
    case 2: return launch_p<32>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace psg
