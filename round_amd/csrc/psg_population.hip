// psg_population.hip — device-resident adversary-search populations
// (psg_population_fresh / psg_population_next, include/psg.h).
//
// The search (round_amd/adversary.py) evaluates populations
// of explicit HO schedules; generating and mutating them on the host made the
// host the bottleneck (10 KB of HO sets per n=64, R=20 schedule over PCIe, numpy
// bit twiddling). Here a generation is four elementwise kernels over HBM:
//   links  — one thread per HO set (instance i, round k, process p): a fresh set
//            (each link present w.p. keep/256: 8 binary digits, x = r | x for a
//            1 digit, r & x for a 0 digit, fresh Philox words r) or a copy of the
//            parent's set; bits >= n cleared;
//   flip   — one thread per (instance, flip): a mutant toggles `flips` random
//            links (64-bit atomic xor: two flips may share a word);
//   repair — one thread per HO set: self bit, then random senders are added
//            until |HO(p)| >= min_size (the Specs' safety predicate, e.g. BenOr's
//            |HO(p)| > n/2, example/BenOr.scala:92);
//   init   — one thread per process: copy, redraw w.p. redraw/256, or fresh.
// Every draw is Philox4x32-10 keyed by the population seed with counter
// (slot, generation, k*n + p, tag | s), so a population is a pure function of its
// parameters (tests recompute them on the host).
//
// Population models (psg_population_fresh_model / _next_model / _read_crash / psg_population_live)
// add wave-level kernels, one wave64 per instance, every draw keyed the same way with tags of
// their own (slot = instance, then generation, index, tag):
//   genome  — the crash family's crash [count][n] + partial [count][n][W]: fresh (f by
//             (0, TAG_CRASH_F); per process q a selection key and a crash round by (q, TAG_CRASH),
//             the f smallest keys crash, found by a ballot radix selection; partial(p) word w by
//             (p, TAG_PARTIAL | 4w + digit pair)), a copy, or a mutant (one crash moved / added /
//             removed by (0, TAG_CRASH_MUT));
//   partial flip — one thread per (instance, flip): a mutant toggles `flips` crash-round
//             deliveries (p, q) by (f, TAG_PFLIP), 64-bit atomic xor as in flip;
//   crash ho — genome -> HO sets by two ballots per (round, word), bits >= n cleared, self bit;
//   force live — omission family, after repair: forced round j is live_at[j] or drawn by
//             (j, TAG_LIVE_AT); a good round's common set by (j, TAG_GOOD | 4w + digit pair) and
//             (j, TAG_GOOD_FILL | 8t + w);
//   live    — the liveness predicate per (instance, round) of the loaded sets, one wave each.
#include <algorithm>

#include "psg_device.hpp"
#include "psg_kernels.hpp"

namespace psg {

constexpr uint32_t TAG_LINKS = 0xA000u << 16, TAG_REPAIR = 0xB000u << 16, TAG_FLIP = 0xC000u << 16,
                   TAG_INIT = 0xD000u << 16;
// population models (below): the crash-family genome and the forced live rounds
constexpr uint32_t TAG_CRASH = 0xE000u << 16, TAG_CRASH_F = 0xE100u << 16, TAG_PARTIAL = 0xE200u << 16,
                   TAG_CRASH_MUT = 0xE300u << 16, TAG_PFLIP = 0xE400u << 16, TAG_LIVE_AT = 0xF000u << 16,
                   TAG_GOOD = 0xF100u << 16, TAG_GOOD_FILL = 0xF200u << 16;

PSG_DEV U4 pop_draw(const PopArgs& a, uint64_t slot, uint32_t c2, uint32_t c3) {
  return philox10((uint32_t)slot, a.gen, c2, c3, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
}

__global__ void __launch_bounds__(256) pop_links_kernel(PopArgs a) {
  const uint64_t sets = a.count * (uint64_t)a.R * (uint64_t)a.n;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < sets; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / ((uint64_t)a.R * a.n);
    const uint32_t kp = (uint32_t)(e - i * (uint64_t)a.R * a.n);  // k * n + p
    const int op = a.op ? a.op[i] : 2;
    uint64_t* dst = a.ho + e * a.W;
    if (op == 2) {
      const uint32_t q = a.keep[i & 3u];  // keep/256, 8 binary digits
      for (int w = 0; w < a.W; ++w) {
        uint64_t x;
        if (q >= 256u) {
          x = ~0ull;
        } else {
          x = 0;
          for (uint32_t j = 0; j < 8; j += 2) {  // digits j, j+1 from one call
            const U4 o = pop_draw(a, i, kp, TAG_LINKS | (uint32_t)(w * 4 + j / 2));
            const uint64_t r0 = (uint64_t)o.x | ((uint64_t)o.y << 32);
            const uint64_t r1 = (uint64_t)o.z | ((uint64_t)o.w << 32);
            x = ((q >> j) & 1u) ? (r0 | x) : (r0 & x);
            x = ((q >> (j + 1)) & 1u) ? (r1 | x) : (r1 & x);
          }
        }
        dst[w] = x & full_word(a.n, w);
      }
    } else {
      const uint64_t* src = a.src + ((uint64_t)a.parent[i] * a.R * a.n + kp) * a.W;
      for (int w = 0; w < a.W; ++w) dst[w] = src[w] & full_word(a.n, w);
    }
  }
}

__global__ void __launch_bounds__(256) pop_flip_kernel(PopArgs a) {
  const uint64_t total = a.count * (uint64_t)a.flips;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / a.flips;
    const uint32_t f = (uint32_t)(e - i * a.flips);
    if (a.op[i] != 1) continue;
    const U4 o = pop_draw(a, i, f, TAG_FLIP);
    const uint32_t k = mulhi32(o.x, (uint32_t)a.R);
    const uint32_t p = mulhi32(o.y, (uint32_t)a.n);
    uint32_t q = mulhi32(o.z, (uint32_t)a.n);
    if (a.self_bit && q == p) q = (q + 1u) % (uint32_t)a.n;
    unsigned long long* word =
        reinterpret_cast<unsigned long long*>(a.ho + ((i * a.R + k) * (uint64_t)a.n + p) * a.W + (q >> 6));
    atomicXor(word, 1ull << (q & 63u));
  }
}

__global__ void __launch_bounds__(256) pop_repair_kernel(PopArgs a) {
  const uint64_t sets = a.count * (uint64_t)a.R * (uint64_t)a.n;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < sets; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / ((uint64_t)a.R * a.n);
    const uint32_t kp = (uint32_t)(e - i * (uint64_t)a.R * a.n);
    const uint32_t p = kp % (uint32_t)a.n;
    uint64_t* s = a.ho + e * a.W;
    if (a.self_bit) s[p >> 6] |= 1ull << (p & 63u);
    if (a.min_size <= 0) continue;
    auto size = [&]() {
      int c = 0;
      for (int w = 0; w < a.W; ++w) c += __popcll(s[w]);
      return c;
    };
    uint32_t t = 0;
    while (size() < a.min_size && t < 64) {  // add random senders (each w.p. 1/2) until large enough
      for (int w = 0; w < a.W; ++w) {
        const U4 o = pop_draw(a, i, kp, TAG_REPAIR | (t * 8u + (uint32_t)w));
        s[w] |= ((uint64_t)o.x | ((uint64_t)o.y << 32)) & full_word(a.n, w);
      }
      ++t;
    }
    if (size() < a.min_size)
      for (int w = 0; w < a.W; ++w) s[w] = full_word(a.n, w);
  }
}

__global__ void __launch_bounds__(256) pop_init_kernel(PopArgs a) {
  const uint64_t cells = a.count * (uint64_t)a.n;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / a.n;
    const uint32_t p = (uint32_t)(e - i * a.n);
    const int op = a.op ? a.op[i] : 2;
    const U4 o = pop_draw(a, i, p, TAG_INIT);
    const int32_t fresh = a.init_kind == POP_INIT_COIN   ? (int32_t)(o.y & 1u)
                          : a.init_kind == POP_INIT_VOTE ? tpc_vote(o.y, (uint32_t)a.V)
                          : a.init_kind == POP_INIT_SET  ? lattice_init(o.y, (uint32_t)a.V)
                                                         : 1 + (int32_t)mulhi32(o.y, (uint32_t)a.V);
    int32_t v = fresh;
    if (op != 2) {
      v = a.src_init[(uint64_t)a.parent[i] * a.n + p];
      if (op == 1 && (o.x >> 24) < a.redraw) v = fresh;
    }
    a.init[e] = v;
  }
}

hipError_t launch_population(const PopArgs& a, hipStream_t s) {
  const uint64_t sets = a.count * (uint64_t)a.R * (uint64_t)a.n;
  auto grid = [](uint64_t work) { return (int)std::min<uint64_t>((work + 255) / 256, 16384); };
  if (sets == 0) return hipSuccess;
  hipLaunchKernelGGL(pop_links_kernel, dim3(grid(sets)), dim3(256), 0, s, a);
  if (a.op && a.flips) hipLaunchKernelGGL(pop_flip_kernel, dim3(grid(a.count * a.flips)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pop_repair_kernel, dim3(grid(sets)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pop_init_kernel, dim3(grid(a.count * (uint64_t)a.n)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------- population models
// The wave-level kernels below run one wave64 per instance (or per (instance, round)), four
// waves per block; lane l holds the processes 64 s + l, s < W.

PSG_DEV uint64_t wave_index() { return (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }
PSG_DEV uint64_t wave_count() { return (uint64_t)gridDim.x * (blockDim.x >> 6); }

// 64 bits, each set w.p. q/256: the digit scheme of pop_links_kernel over the draws
// (slot, gen, c2, tag | 0..3)
PSG_DEV uint64_t density_word(const PopArgs& a, uint64_t slot, uint32_t c2, uint32_t tag, uint32_t q) {
  if (q >= 256u) return ~0ull;
  uint64_t x = 0;
  for (uint32_t j = 0; j < 8; j += 2) {
    const U4 o = pop_draw(a, slot, c2, tag | (j / 2));
    const uint64_t r0 = (uint64_t)o.x | ((uint64_t)o.y << 32);
    const uint64_t r1 = (uint64_t)o.z | ((uint64_t)o.w << 32);
    x = ((q >> j) & 1u) ? (r0 | x) : (r0 & x);
    x = ((q >> (j + 1)) & 1u) ? (r1 | x) : (r1 & x);
  }
  return x;
}

// The crash-family genome of one generation: crash [count][n] and partial [count][n][W].
//   fresh  — f = mulhi(x, fmax + 1) of the draw (i, 0, TAG_CRASH_F); process q draws (i, q, TAG_CRASH):
//            a selection key (x with q in its low byte, so keys are distinct) and a crash round
//            mulhi(y, R); the f smallest keys crash. They are found by a radix selection over the
//            key bits from the top, one ballot + popcount per bit and word: no lane loops over n.
//            partial(p) word w: density_word over the draws (i, p, TAG_PARTIAL | 4w + 0..3).
//   copy   — the parent's genome;
//   mutant — the parent's genome with at most one crash changed, by the draw (i, 0, TAG_CRASH_MUT):
//            u = x >> 24 against the thresholds move / add / drop (an impossible action falls
//            through to the next, as schedules.mutate_crash does), the mulhi(y, pool)-th process
//            of the pool (crashed, or correct for `add`) by ballot rank, new round mulhi(z, R).
//            (Its partial flips: pop_partial_flip_kernel.)
template <int W>
__global__ void __launch_bounds__(256) pop_genome_kernel(PopArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint64_t i = wave_index(); i < a.count; i += wave_count()) {
    const int op = a.op ? a.op[i] : 2;
    int32_t cr[W];
    if (op == 2) {
      uint32_t key[W];
      bool cand[W], sel[W];
#pragma unroll
      for (int s = 0; s < W; ++s) {
        const uint32_t q = 64u * s + lane;
        const U4 o = pop_draw(a, i, q, TAG_CRASH);
        key[s] = (o.x & ~0xFFu) | (q & 0xFFu);
        cr[s] = (int32_t)mulhi32(o.y, (uint32_t)a.R);
        cand[s] = q < (uint32_t)a.n;
        sel[s] = false;
      }
      uint32_t need = mulhi32(pop_draw(a, i, 0, TAG_CRASH_F).x, (uint32_t)a.fmax + 1u);
      for (int b = 31; b >= 0; --b) {  // the `need` smallest keys among cand: at most one is left after bit 0
        bool zero[W];
        uint32_t c = 0;
#pragma unroll
        for (int s = 0; s < W; ++s) {
          zero[s] = cand[s] && !((key[s] >> b) & 1u);
          c += (uint32_t)__popcll(__ballot(zero[s]));
        }
        const bool narrow = c > need;  // wave-uniform
#pragma unroll
        for (int s = 0; s < W; ++s) {
          if (!narrow) sel[s] = sel[s] || zero[s];
          cand[s] = narrow ? zero[s] : (cand[s] && !zero[s]);
        }
        if (!narrow) need -= c;
      }
#pragma unroll
      for (int s = 0; s < W; ++s)
        if (!(sel[s] || (need != 0u && cand[s]))) cr[s] = -1;
    } else {
      const uint64_t pr = a.parent[i];
#pragma unroll
      for (int s = 0; s < W; ++s) {
        const int q = 64 * s + lane;
        cr[s] = q < a.n ? a.src_crash[pr * a.n + q] : -1;
      }
      if (op == 1) {
        const U4 o = pop_draw(a, i, 0, TAG_CRASH_MUT);
        const uint32_t u = o.x >> 24;
        uint64_t pool[W];
        uint32_t ncr = 0;
#pragma unroll
        for (int s = 0; s < W; ++s) {
          pool[s] = __ballot(cr[s] >= 0);
          ncr += (uint32_t)__popcll(pool[s]);
        }
        const int act = (u < a.t_move && ncr > 0u)                    ? 1
                        : (u < a.t_add && ncr < (uint32_t)a.fmax)     ? 2
                        : (u < a.t_drop && ncr > 0u)                  ? 3
                                                                      : 0;
        if (act) {  // wave-uniform
          const uint32_t cnt = act == 2 ? (uint32_t)a.n - ncr : ncr;  // > 0: add only while ncr < fmax <= n
          const uint32_t j = mulhi32(o.y, cnt);
          const int32_t round = act == 3 ? -1 : (int32_t)mulhi32(o.z, (uint32_t)a.R);
          uint32_t before = 0;
#pragma unroll
          for (int s = 0; s < W; ++s) {
            const uint64_t m = act == 2 ? (~pool[s] & full_word(a.n, s)) : pool[s];
            if (((m >> lane) & 1ull) && before + (uint32_t)__popcll(m & below) == j) cr[s] = round;
            before += (uint32_t)__popcll(m);
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < W; ++s) {
      const int p = 64 * s + lane;
      if (p >= a.n) continue;
      a.crash[i * a.n + p] = cr[s];
      uint64_t* dst = a.partial + (i * a.n + p) * W;
      if (op == 2) {
#pragma unroll
        for (int w = 0; w < W; ++w)
          dst[w] = density_word(a, i, (uint32_t)p, TAG_PARTIAL | (uint32_t)(4 * w), a.partial_p[i & 3u]) &
                   full_word(a.n, w);
      } else {
        const uint64_t* src = a.src_partial + ((uint64_t)a.parent[i] * a.n + p) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) dst[w] = src[w];
      }
    }
  }
}

// One thread per (instance, flip): a mutant toggles `flips` crash-round deliveries (p, q) drawn
// by (i, f, TAG_PFLIP) (64-bit atomic xor: two flips may share a word, as in pop_flip_kernel).
__global__ void __launch_bounds__(256) pop_partial_flip_kernel(PopArgs a) {
  const uint64_t total = a.count * (uint64_t)a.flips;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / a.flips;
    const uint32_t f = (uint32_t)(e - i * a.flips);
    if (a.op[i] != 1) continue;
    const U4 o = pop_draw(a, i, f, TAG_PFLIP);
    const uint32_t p = mulhi32(o.x, (uint32_t)a.n);
    const uint32_t q = mulhi32(o.y, (uint32_t)a.n);
    unsigned long long* word =
        reinterpret_cast<unsigned long long*>(a.partial + (i * a.n + p) * (uint64_t)a.W + (q >> 6));
    atomicXor(word, 1ull << (q & 63u));
  }
}

// Genome -> HO sets (schedules.crash_to_ho): per round two ballots per word give the senders
// heard by everyone (correct, or k < crash) and the ones crashing now (heard by partial(p));
// lane p writes the W words of HO(p, k), the wave 512 W contiguous bytes.
template <int W>
__global__ void __launch_bounds__(256) pop_crash_ho_kernel(PopArgs a) {
  const int lane = threadIdx.x & 63;
  for (uint64_t i = wave_index(); i < a.count; i += wave_count()) {
    int32_t cr[W];
    uint64_t part[W][W];
#pragma unroll
    for (int s = 0; s < W; ++s) {
      const int p = 64 * s + lane;
      cr[s] = p < a.n ? a.crash[i * a.n + p] : -1;
#pragma unroll
      for (int w = 0; w < W; ++w) part[s][w] = p < a.n ? a.partial[(i * a.n + p) * W + w] : 0ull;
    }
    for (int k = 0; k < a.R; ++k) {
      uint64_t alive[W], now[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        alive[w] = __ballot(cr[w] < 0 || k < cr[w]);
        now[w] = __ballot(cr[w] == k);
      }
#pragma unroll
      for (int s = 0; s < W; ++s) {
        const int p = 64 * s + lane;
        if (p >= a.n) continue;
        uint64_t* dst = a.ho + ((i * a.R + k) * (uint64_t)a.n + p) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          uint64_t x = (alive[w] | (now[w] & part[s][w])) & full_word(a.n, w);
          if (a.self_bit && w == s) x |= 1ull << lane;
          dst[w] = x;
        }
      }
    }
  }
}

// Forced live rounds of the omission family, after links / flips / repair, one wave per instance,
// the forced rounds in order (two may coincide). Round j is live_at[j], or mulhi(x, R) of the draw
// (i, j, TAG_LIVE_AT).
//   good round — every HO(p, k) := s: everyone with self_bit, else density_word at 230/256 over
//                (i, j, TAG_GOOD | 4w + 0..3), topped up by (i, j, TAG_GOOD_FILL | 8t + w) words
//                (each member w.p. 1/2, t < 64, then everyone) until |s| > 2n/3 and |s| >= min_size
//                (schedules.force_good_round);
//   coord hears all — HO((k' / phase) % n, k') := everyone over the phase containing k;
//   fixed coord — in that phase: slot 1, HO(coord) := everyone; slot 2, coord joins every HO(p).
template <int W>
__global__ void __launch_bounds__(256) pop_force_live_kernel(PopArgs a) {
  const int lane = threadIdx.x & 63;
  for (uint64_t i = wave_index(); i < a.count; i += wave_count()) {
    uint64_t* inst = a.ho + i * a.R * (uint64_t)a.n * W;
    for (int j = 0; j < a.live_rounds; ++j) {
      int k = a.live_at[j];
      if (k < 0) k = (int)mulhi32(pop_draw(a, i, (uint32_t)j, TAG_LIVE_AT).x, (uint32_t)a.R);
      const int base = (k / a.phase) * a.phase, end = min(a.R, base + a.phase);
      if (a.live_kind == PSG_LIVE_GOOD_ROUND) {
        uint64_t s[W];
        auto size = [&]() {
          int c = 0;
#pragma unroll
          for (int w = 0; w < W; ++w) c += __popcll(s[w]);
          return c;
        };
#pragma unroll
        for (int w = 0; w < W; ++w)
          s[w] = (a.self_bit ? ~0ull : density_word(a, i, (uint32_t)j, TAG_GOOD | (uint32_t)(4 * w), 230u)) &
                 full_word(a.n, w);
        const int thr = (2 * a.n) / 3;
        uint32_t t = 0;
        while ((size() <= thr || size() < a.min_size) && t < 64u) {
#pragma unroll
          for (int w = 0; w < W; ++w) {
            const U4 o = pop_draw(a, i, (uint32_t)j, TAG_GOOD_FILL | (t * 8u + (uint32_t)w));
            s[w] |= ((uint64_t)o.x | ((uint64_t)o.y << 32)) & full_word(a.n, w);
          }
          ++t;
        }
        if (size() <= thr || size() < a.min_size) {
#pragma unroll
          for (int w = 0; w < W; ++w) s[w] = full_word(a.n, w);
        }
#pragma unroll
        for (int sl = 0; sl < W; ++sl) {
          const int p = 64 * sl + lane;
          if (p >= a.n) continue;
          uint64_t* dst = inst + ((uint64_t)k * a.n + p) * W;
#pragma unroll
          for (int w = 0; w < W; ++w) dst[w] = s[w];
        }
      } else if (a.live_kind == PSG_LIVE_COORD_HEARS_ALL) {
        for (int kk = base; kk < end; ++kk) {
          const int c = (kk / a.phase) % a.n;
          if (lane < W) inst[((uint64_t)kk * a.n + c) * W + lane] = full_word(a.n, lane);
        }
      } else {  // PSG_LIVE_FIXED_COORD
        if (base + 1 < end && lane < W) inst[((uint64_t)(base + 1) * a.n + a.coord) * W + lane] = full_word(a.n, lane);
        if (base + 2 < end) {
#pragma unroll
          for (int sl = 0; sl < W; ++sl) {
            const int p = 64 * sl + lane;
            if (p < a.n) inst[((uint64_t)(base + 2) * a.n + p) * W + (a.coord >> 6)] |= 1ull << (a.coord & 63);
          }
        }
      }
    }
  }
}

// psg_population_live: one wave per (instance, round), lane p compares the W words of HO(p, k)
// (bits >= n masked off); the verdict is one ballot.
__global__ void __launch_bounds__(256) pop_live_kernel(LiveArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t pairs = a.count * (uint64_t)a.R;
  for (uint64_t e = wave_index(); e < pairs; e += wave_count()) {
    const int k = (int)(e % (uint64_t)a.R);
    const uint64_t* row = a.ho + e * (uint64_t)a.n * a.W;  // HO(0..n-1, k) of the instance
    const int slot = k % a.phase;
    bool ok = true;
    bool extra = true;  // wave-uniform part of the verdict
    if (a.kind == PSG_LIVE_GOOD_ROUND) {
      int size = 0;
      for (int w = 0; w < a.W; ++w) size += __popcll(row[w] & full_word(a.n, w));
      extra = size > (2 * a.n) / 3;
      for (int p = lane; p < a.n; p += 64)
        for (int w = 0; w < a.W; ++w) ok = ok && ((row[(uint64_t)p * a.W + w] ^ row[w]) & full_word(a.n, w)) == 0ull;
    } else if (a.kind == PSG_LIVE_COORD_HEARS_ALL || slot == 1) {
      const int c = a.kind == PSG_LIVE_COORD_HEARS_ALL ? (k / a.phase) % a.n : a.coord;
      if (lane < a.W) ok = (~row[(uint64_t)c * a.W + lane] & full_word(a.n, lane)) == 0ull;
    } else if (slot == 2) {
      for (int p = lane; p < a.n; p += 64) ok = ok && ((row[(uint64_t)p * a.W + (a.coord >> 6)] >> (a.coord & 63)) & 1ull);
    }
    const bool all = __ballot(!ok) == 0ull;
    if (lane == 0) a.live[e] = (all && extra) ? 1 : 0;
  }
}

static int wave_grid(uint64_t waves) { return (int)std::min<uint64_t>((waves + 3) / 4, 16384); }

hipError_t launch_population_live(const PopArgs& a, hipStream_t s) {
  if (a.count == 0 || a.live_rounds == 0 || a.live_kind == PSG_LIVE_NONE) return hipSuccess;
  return with_w<hipError_t>(a.W, hipErrorInvalidValue, [&](auto w) {
    hipLaunchKernelGGL(pop_force_live_kernel<decltype(w)::value>, dim3(wave_grid(a.count)), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_population_crash(const PopArgs& a, hipStream_t s) {
  if (a.count == 0) return hipSuccess;
  auto grid = [](uint64_t work) { return (int)std::min<uint64_t>((work + 255) / 256, 16384); };
  return with_w<hipError_t>(a.W, hipErrorInvalidValue, [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL(pop_genome_kernel<W>, dim3(wave_grid(a.count)), dim3(256), 0, s, a);
    if (a.op && a.flips) hipLaunchKernelGGL(pop_partial_flip_kernel, dim3(grid(a.count * a.flips)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pop_crash_ho_kernel<W>, dim3(wave_grid(a.count)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pop_init_kernel, dim3(grid(a.count * (uint64_t)a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_crash_ho(const PopArgs& a, hipStream_t s) {
  if (a.count == 0) return hipSuccess;
  return with_w<hipError_t>(a.W, hipErrorInvalidValue, [&](auto w) {
    hipLaunchKernelGGL(pop_crash_ho_kernel<decltype(w)::value>, dim3(wave_grid(a.count)), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_live_predicate(const LiveArgs& a, hipStream_t s) {
  if (a.count == 0) return hipSuccess;
  hipLaunchKernelGGL(pop_live_kernel, dim3(wave_grid(a.count * (uint64_t)a.R)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace psg
