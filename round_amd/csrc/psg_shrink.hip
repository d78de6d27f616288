// psg_shrink.hip — the adversary search's shrink step on the device (psg_shrink_*, include/psg.h).
//
// Adversary.shrink (round_amd/adversary.py) simplifies a counterexample by greedy batched delta
// debugging: every candidate of a step is the current schedule (the base, [R][n][W]) with one edit,
// the candidates of a level are enumerated in a fixed order, and the best surviving one becomes the
// next base. Here the base lives in HBM and a step is
//   scan   — per unit of the level (the tail, a round, a set, a crash edit) the number of
//            candidates it contributes, their exclusive prefix and the level's total (one block:
//            at most 250 x 256 units), with LINK's cap: the enumeration stops after the first set
//            whose candidates bring the count above the cap;
//   edits  — one thread per candidate of a chunk: its unit by a binary search of the prefix, its
//            rank inside the unit, and from them the edit (a word range made full, or one bit);
//   fill   — the hot path, a pure write stream: one thread per 64-bit word of the schedule, the
//            base word read once and written to eight candidates (512 contiguous bytes per wave
//            and store), each with its edit applied where it hits;
//   rows   — the per-process rows of every candidate: the base's initial values, its crash rounds
//            (CRASH: with the candidate's edit) and CRASH's crash-round delivery sets;
//   part   — CRASH: who hears q in q's crash round, from the base (the candidates' HO sets are
//            then pop_crash_ho_kernel's, psg_population.hip);
//   links  — one wave64 per loaded instance: the popcount of its R n W words (bits < n).
// Adopting candidate j is the same edits + fill with the base as the destination (an elementwise
// update in place), so it does not need the candidate to be loaded. Plain vector stores only.
#include <algorithm>

#include "psg_device.hpp"
#include "psg_kernels.hpp"

namespace psg {

// Links missing from set u of the base (bits >= n are clear).
PSG_DEV uint32_t set_missing(const ShrinkArgs& a, uint32_t u) {
  uint32_t c = 0;
  for (int w = 0; w < a.W; ++w) c += (uint32_t)__popcll(~a.base[(uint64_t)u * a.W + w] & full_word(a.n, w));
  return c;
}

// Candidates unit u contributes at the level.
PSG_DEV uint32_t unit_count(const ShrinkArgs& a, uint32_t u) {
  switch (a.level) {
    case PSG_SHRINK_TAIL: return 1u;
    case PSG_SHRINK_ROUND: {
      for (uint32_t p = 0; p < (uint32_t)a.n; ++p)
        if (set_missing(a, u * (uint32_t)a.n + p)) return 1u;
      return 0u;
    }
    case PSG_SHRINK_SET: return set_missing(a, u) ? 1u : 0u;
    case PSG_SHRINK_LINK: return set_missing(a, u);
    default: {  // PSG_SHRINK_CRASH: un-crash q (u = q), then crash q a round later (u = n + q)
      const bool later = u >= (uint32_t)a.n;
      const int32_t c = a.base_crash[later ? u - (uint32_t)a.n : u];
      return (c >= 0 && (!later || c + 1 < a.R)) ? 1u : 0u;
    }
  }
}

// One block of 256: a wave scan by shuffles, the four wave totals through LDS, a running carry.
__global__ void __launch_bounds__(256) shrink_scan_kernel(ShrinkArgs a) {
  __shared__ uint32_t wave_total[4];
  __shared__ uint32_t capped;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t cap = a.level == PSG_SHRINK_LINK ? a.arg : 0u;
  if (threadIdx.x == 0) capped = 0xFFFFFFFFu;
  uint32_t carry = 0;
  for (uint32_t b = 0; b < a.units; b += 256u) {
    const uint32_t u = b + threadIdx.x;
    const uint32_t c = u < a.units ? unit_count(a, u) : 0u;
    uint32_t inc = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int j = 0; j < 4; ++j) {
      if (j < wave) before += wave_total[j];
      all += wave_total[j];
    }
    const uint32_t excl = carry + before + inc - c;
    if (u < a.units) {
      a.pre[u] = excl;
      // the first unit whose candidates bring the count above the cap ends the enumeration
      // (counts only grow, so one unit at most sees the cap inside its candidates)
      if (cap && excl <= cap && excl + c > cap) capped = excl + c;
    }
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.pre[a.units] = carry;
    a.pre[a.units + 1] = capped != 0xFFFFFFFFu ? capped : carry;
  }
}

__global__ void __launch_bounds__(256) shrink_edits_kernel(ShrinkArgs a) {
  const uint32_t nW = (uint32_t)a.n * (uint32_t)a.W, per = (uint32_t)a.R * nW;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.count; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t idx = (uint32_t)(a.first + j);  // < the level's total <= pre[units]
    uint32_t u = 0, hi = a.units;                  // the last unit with pre[u] <= idx: it holds idx
    while (hi - u > 1u) {
      const uint32_t mid = (u + hi) >> 1;
      if (a.pre[mid] <= idx) u = mid;
      else hi = mid;
    }
    ShrinkEdit e;
    e.unit = u;
    e.bit = SHRINK_FULL;
    e.lo = e.hi = 0;
    if (a.level == PSG_SHRINK_TAIL) {
      e.lo = std::min(a.arg, (uint32_t)a.R) * nW;
      e.hi = per;
    } else if (a.level == PSG_SHRINK_ROUND) {
      e.lo = u * nW;
      e.hi = e.lo + nW;
    } else if (a.level == PSG_SHRINK_SET) {
      e.lo = u * (uint32_t)a.W;
      e.hi = e.lo + (uint32_t)a.W;
    } else if (a.level == PSG_SHRINK_LINK) {  // the (idx - pre[u])-th missing link of set u
      uint32_t rank = idx - a.pre[u];
      for (int w = 0; w < a.W; ++w) {
        uint64_t z = ~a.base[(uint64_t)u * a.W + w] & full_word(a.n, w);
        const uint32_t c = (uint32_t)__popcll(z);
        if (rank >= c) {
          rank -= c;
          continue;
        }
        for (; rank; --rank) z &= z - 1ull;
        e.lo = u * (uint32_t)a.W + (uint32_t)w;
        e.hi = e.lo + 1u;
        e.bit = (uint32_t)__ffsll((long long)z) - 1u;
        break;
      }
    }
    a.edit[j] = e;
  }
}

// Candidates per base word read: a block column writes kFillRows candidates' copies of its words.
constexpr int kFillRows = 8;

template <int W>
__global__ void __launch_bounds__(256) shrink_fill_kernel(ShrinkArgs a) {
  const uint32_t per = (uint32_t)a.R * (uint32_t)a.n * (uint32_t)W;
  for (uint64_t i0 = (uint64_t)blockIdx.y * kFillRows; i0 < a.count; i0 += (uint64_t)gridDim.y * kFillRows) {
    const int rows = (int)std::min<uint64_t>(kFillRows, a.count - i0);
    ShrinkEdit e[kFillRows];  // wave-uniform, read once per block row: the word loop only stores
#pragma unroll
    for (int j = 0; j < kFillRows; ++j) e[j] = a.edit[i0 + (uint64_t)(j < rows ? j : 0)];
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < per; r += gridDim.x * 256u) {
      const uint64_t b = a.base[r];
      const uint64_t full = full_word(a.n, (int)(r % (uint32_t)W));
#pragma unroll
      for (int j = 0; j < kFillRows; ++j) {
        if (j >= rows) break;
        uint64_t x = b;
        if (r >= e[j].lo && r < e[j].hi) x = e[j].bit == SHRINK_FULL ? full : (b | (1ull << e[j].bit));
        a.ho[(i0 + j) * per + r] = x;
      }
    }
  }
}

// One thread per (candidate, process): the base's initial value and crash round (CRASH: under the
// candidate's edit) and, at CRASH, the W words of the base's crash-round deliveries to p.
__global__ void __launch_bounds__(256) shrink_rows_kernel(ShrinkArgs a) {
  const uint64_t cells = a.count * (uint64_t)a.n;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / (uint64_t)a.n;
    const uint32_t p = (uint32_t)(e - i * (uint64_t)a.n);
    if (a.init) a.init[e] = a.base_init[p];
    if (a.crash && a.base_crash) {
      int32_t c = a.base_crash[p];
      if (a.level == PSG_SHRINK_CRASH) {
        const uint32_t u = a.edit[i].unit;
        if (u == p) c = -1;
        else if (u == (uint32_t)a.n + p) c += 1;
      }
      a.crash[e] = c;
    }
    if (a.partial)
      for (int w = 0; w < a.W; ++w) a.partial[e * a.W + w] = a.part[(uint64_t)p * a.W + w];
  }
}

// part(p) bit q = bit q of HO(p, crash(q)) for every crashed q: one thread per (p, word).
__global__ void __launch_bounds__(256) shrink_part_kernel(ShrinkArgs a) {
  const uint32_t cells = (uint32_t)a.n * (uint32_t)a.W;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < cells; e += gridDim.x * blockDim.x) {
    const uint32_t p = e / (uint32_t)a.W, w = e - p * (uint32_t)a.W;
    uint64_t x = 0;
    for (uint32_t q = 64u * w; q < std::min((uint32_t)a.n, 64u * w + 64u); ++q) {
      const int32_t c = a.base_crash[q];
      if (c >= 0) x |= a.base[((uint64_t)c * a.n + p) * a.W + w] & (1ull << (q & 63u));
    }
    a.part[e] = x;
  }
}

// One wave64 per instance: lane l sums the popcounts of words l, l + 64, ... (512 contiguous bytes
// per wave and load), then a butterfly over the wave.
template <int W>
__global__ void __launch_bounds__(256) links_kernel(const uint64_t* ho, uint32_t* links, uint64_t count, int n, int R) {
  const int lane = threadIdx.x & 63;
  const uint32_t per = (uint32_t)R * (uint32_t)n * (uint32_t)W;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < count; i += waves) {
    const uint64_t* inst = ho + i * per;
    uint32_t c = 0;
#pragma unroll 4
    for (uint32_t r = lane; r < per; r += 64u) c += (uint32_t)__popcll(inst[r] & full_word(n, (int)(r % (uint32_t)W)));
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) links[i] = c;
  }
}

static int flat_grid(uint64_t work) { return (int)std::min<uint64_t>((work + 255) / 256, 16384); }

hipError_t launch_shrink_scan(const ShrinkArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(shrink_scan_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_shrink_edits(const ShrinkArgs& a, hipStream_t s) {
  if (a.count == 0) return hipSuccess;
  hipLaunchKernelGGL(shrink_edits_kernel, dim3(flat_grid(a.count)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_shrink_fill(const ShrinkArgs& a, hipStream_t s) {
  if (a.count == 0) return hipSuccess;
  const uint64_t per = (uint64_t)a.R * a.n * a.W;
  const dim3 grid((unsigned)std::min<uint64_t>((per + 255) / 256, 1024),
                  (unsigned)std::min<uint64_t>((a.count + kFillRows - 1) / kFillRows, 65535));
  return with_w<hipError_t>(a.W, hipErrorInvalidValue, [&](auto w) {
    hipLaunchKernelGGL(shrink_fill_kernel<decltype(w)::value>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_shrink_rows(const ShrinkArgs& a, hipStream_t s) {
  if (a.count == 0) return hipSuccess;
  hipLaunchKernelGGL(shrink_rows_kernel, dim3(flat_grid(a.count * (uint64_t)a.n)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_shrink_part(const ShrinkArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(shrink_part_kernel, dim3(flat_grid((uint64_t)a.n * a.W)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_links(const uint64_t* ho, uint32_t* links, uint64_t count, int n, int R, int W, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const int grid = (int)std::min<uint64_t>((count + 3) / 4, 16384);
  return with_w<hipError_t>(W, hipErrorInvalidValue, [&](auto w) {
    hipLaunchKernelGGL(links_kernel<decltype(w)::value>, dim3(grid), dim3(256), 0, s, ho, links, count, n, R);
    return hipGetLastError();
  });
}

}  // namespace psg
