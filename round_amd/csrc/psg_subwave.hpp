// psg_subwave.hpp — sub-wave packing: G = 64 / P instances of n <= P processes share one
// wave64, each on P adjacent lanes (a "sub-group"); P = 4, 8, 16 or 32.
//
// Lane l is process l % P of sub-group l / P. A set of processes (an HO set, a mailbox, the
// deciders) is a per-lane 32-bit mask in sub-group-local bit positions: bit j = process j of the
// lane's own instance. Every lane of a sub-group holds the same mask, so what is wave-uniform in
// the one-instance-per-wave kernels is here "sub-group-uniform": a VGPR value that agrees on the
// P lanes of a sub-group. The only instruction the sub-groups share is the wave ballot, of which
// each lane keeps its own P-bit slice; everything else stays inside the sub-group. No LDS.
// (Not to be confused with psg_packed.hpp, which packs the W waves of one n > 64 instance into
// one wave.)
#pragma once
#include "psg_device.hpp"

namespace psg {

template <int P>
struct Sub {
  static_assert(P == 4 || P == 8 || P == 16 || P == 32, "sub-group width");
  static constexpr int kG = 64 / P;  // sub-groups (instances) per wave
  static constexpr uint32_t kMask = P == 32 ? 0xFFFFFFFFu : (1u << (P & 31)) - 1u;
  int lane;   // 0..63
  int pid;    // lane % P: the process inside the sub-group
  int sub;    // lane / P: the sub-group
  int shift;  // sub * P: the sub-group's first lane
  PSG_DEV void setup() {
    lane = threadIdx.x & 63;
    pid = lane & (P - 1);
    sub = lane / P;
    shift = lane & ~(P - 1);
  }
  // Processes of the lane's own sub-group for which pred holds (local bit positions). One wave
  // ballot; call from converged control flow. pred must be false on lanes that hold no process.
  PSG_DEV uint32_t ballot(bool pred) const {
    return (uint32_t)(__builtin_amdgcn_ballot_w64(pred) >> shift) & kMask;
  }
  // v of process j of the lane's own sub-group; j is sub-group-uniform, 0 <= j < P
  PSG_DEV int32_t bcast(int32_t v, int j) const { return __shfl(v, shift + j); }
  // sum of v over the sub-group, in every one of its lanes (xor butterfly inside the P lanes)
  PSG_DEV uint64_t sum64(uint64_t v) const {
#pragma unroll
    for (int o = P / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
  }
};

// The set {0..n-1} as a local mask (n <= 32)
PSG_DEV uint32_t sub_full(int n) { return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }

// First-fail record of a sub-group's instance: the 12 first_fail bytes of psg_instance_summary
// in the dwords of lanes pid 0..2 (lane pid p: slots 4p .. 4p+3, byte b = slot 4p + b), as they
// lie in the record. Check points arrive in increasing order and c < PSG_NEVER, so a byte is
// written once: while it still holds PSG_NEVER. `ever` is the OR of all fail words (sub-group-
// uniform), `term` the first check point at which Termination held.
struct SubChecks {
  uint32_t ffw, ever;
  int32_t term;
  PSG_DEV void reset() {
    ffw = 0xFFFFFFFFu;
    ever = 0u;
    term = (int32_t)PSG_NEVER;
  }
  // failbits: bit s set iff slot s is false at check point c (sub-group-uniform)
  PSG_DEV void record(uint32_t failbits, bool termination, int c, int pid) {
    const uint32_t nib = (failbits >> (4 * (pid & 3))) & 0xFu;
    // nibble bit b -> byte b all-ones: the four shifted copies (bits 0-3, 7-10, 14-17, 21-24) do
    // not overlap, so bit 8b of the product is nibble bit b
    const uint32_t hit = ((nib * 0x00204081u) & 0x01010101u) * 0xFFu;
    // bytes still PSG_NEVER: a recorded byte is a check point < 0xFF, so bit 7 & ... & bit 0 is 0
    uint32_t t = ffw & (ffw >> 4);
    t &= t >> 2;
    t &= t >> 1;
    const uint32_t fresh = hit & ((t & 0x01010101u) * 0xFFu);
    ffw = (ffw & ~fresh) | (((uint32_t)c * 0x01010101u) & fresh);
    ever |= failbits;
    term = (termination && term == (int32_t)PSG_NEVER) ? c : term;
  }
};

// Take-G-rows queue over the launch's instance counters (InstanceQueue's slices and counters,
// psg_device.hpp): a wave takes kChunk consecutive batch rows per atomic and hands them out up
// to G at a time; the last hand-out of a chunk or of a queue's slice holds fewer than G rows.
template <int G>
struct RowQueue {
  static constexpr uint64_t kChunk = 4 * G;
  uint64_t cur = 0, lim = 0;  // uniform: [cur, lim) is this wave's current chunk
  int tries = 0;              // queues drained so far
  // rows [base, base + cnt), 1 <= cnt <= G; false when the whole batch is taken. Every lane of
  // the wave, converged.
  PSG_DEV bool take(const KArgs& a, uint64_t& base, int& cnt) {
    if (cur >= lim && !refill(a)) return false;
    base = cur;
    const uint64_t left = lim - cur;
    cnt = left < (uint64_t)G ? (int)left : G;
    cur += (uint64_t)cnt;
    return true;
  }

 private:
  PSG_DEV bool refill(const KArgs& a) {
    const int home = (int)(blockIdx.x % NQUEUES);
    for (; tries < NQUEUES; ++tries) {
      const int q = (home + tries) % NQUEUES;
      const uint64_t lo = a.count * q / NQUEUES, hi = a.count * (q + 1) / NQUEUES;
      if (lo >= hi) continue;
      uint64_t v = 0;
      if ((threadIdx.x & 63) == 0)
        v = atomicAdd(&a.counters[C_QUEUE + q * QUEUE_STRIDE], (unsigned long long)kChunk);
      v = rfl64(v);
      if (lo + v < hi) {  // (v >= hi - lo once the slice is drained: no row index is formed from it)
        cur = lo + v;
        lim = cur + kChunk < hi ? cur + kChunk : hi;
        return true;
      }
    }
    return false;
  }
};

}  // namespace psg
