// psg_kernels.hpp — launcher declarations (one translation unit per algorithm).
#pragma once
#ifndef __HIPCC_RTC__  // (a hiprtc build of a fused Spec module has no host launchers)
#include <hip/hip_runtime.h>

#include <type_traits>

namespace psg {
struct KArgs;
struct VmArgs;
struct PopArgs;
struct LiveArgs;
struct ShrinkArgs;

// Runtime W (mask words, 1..4) -> compile-time constant: f(std::integral_constant<int, W>) for a
// generic callable f, `bad` outside that range.
template <class R, class F>
R with_w(int W, R bad, F&& f) {
  switch (W) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
  }
  return bad;
}

hipError_t launch_otr(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_lv(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_floodmin(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_kset(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_benor(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_otr2(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_slv(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_kset_es(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_epsilon(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_tpc(const KArgs& a, int W, int grid, hipStream_t s);
hipError_t launch_lattice(const KArgs& a, int W, int grid, hipStream_t s);
// OTR with G = psg_pack_width > 1 instances per wave (psg_otr_packed.hip); sizes its own grid
hipError_t launch_otr_packed(const KArgs& a, int G, hipStream_t s);

const void* otr_kernel_ptr(int W);
const void* lv_kernel_ptr(int W);
const void* floodmin_kernel_ptr(int W);
const void* kset_kernel_ptr(int W);
const void* benor_kernel_ptr(int W);
const void* otr2_kernel_ptr(int W);
const void* slv_kernel_ptr(int W);
const void* kset_es_kernel_ptr(int W);
const void* epsilon_kernel_ptr(int W);
const void* tpc_kernel_ptr(int W);
const void* lattice_kernel_ptr(int W);
// the kernels OTR / OTR2 launch a plain schedule with (psg_device.hpp plain_schedule)
const void* otr_plain_kernel_ptr(int W);
const void* otr2_plain_kernel_ptr(int W);

hipError_t launch_champ_selftest(const uint64_t* sets, int count, int tiebreak, int32_t* out, hipStream_t s);
// self-tests of the EpsilonConsensus kernel's building blocks (psg_epsilon.hip, psg_selftest_eps_*)
hipError_t launch_eps_selftest_f64(const double* x, int count, double* out_f64, int64_t* out_key, int32_t* out_i32,
                                   hipStream_t s);
hipError_t launch_eps_selftest_maxr(const double* q, const double* c, int count, int32_t* out, hipStream_t s);
hipError_t launch_eps_selftest_sort(int network, const double* x, const int32_t* ns, int cases, double* out_x,
                                    int32_t* out_pid, int32_t* out_fell, hipStream_t s);
hipError_t launch_eps_selftest_transpose(const uint64_t* rows, int cases, uint64_t* out, hipStream_t s);
hipError_t launch_eps_selftest_select(const uint64_t* masks, int count, int32_t* out, hipStream_t s);
hipError_t launch_eps_selftest_members(const uint64_t* U, const int32_t* spid, int cases, uint64_t* out, hipStream_t s);
hipError_t launch_eps_selftest_reduce(int W, int n, const int64_t* v, const uint8_t* in, int cases, int64_t* out, hipStream_t s);
hipError_t launch_schedule(const KArgs& a, int W, int grid, uint64_t* ho_out, int32_t* crash_out, hipStream_t s);
hipError_t launch_population(const PopArgs& a, hipStream_t s);
// population models: the forced live rounds over a.ho (after launch_population), a crash-family
// generation (genome, its HO sets, initial values), the liveness predicate per (instance, round)
hipError_t launch_population_live(const PopArgs& a, hipStream_t s);
hipError_t launch_population_crash(const PopArgs& a, hipStream_t s);
hipError_t launch_live_predicate(const LiveArgs& a, hipStream_t s);
// genome -> HO sets alone: a.ho [count][R][n][W] from a.crash, a.partial (pop_crash_ho_kernel)
hipError_t launch_crash_ho(const PopArgs& a, hipStream_t s);
// shrinking on the device (psg_shrink.hip): the level's prefix and total over the base; the edits
// of candidates [first, first + count); the candidates' sets (or, ho = base and count = 1, the base
// edited in place); their initial values, crash rounds and (CRASH) delivery sets; the base's
// crash-round deliveries; links of every loaded instance
hipError_t launch_shrink_scan(const ShrinkArgs& a, hipStream_t s);
hipError_t launch_shrink_edits(const ShrinkArgs& a, hipStream_t s);
hipError_t launch_shrink_fill(const ShrinkArgs& a, hipStream_t s);
hipError_t launch_shrink_rows(const ShrinkArgs& a, hipStream_t s);
hipError_t launch_shrink_part(const ShrinkArgs& a, hipStream_t s);
hipError_t launch_links(const uint64_t* ho, uint32_t* links, uint64_t count, int n, int R, int W, hipStream_t s);
hipError_t launch_spec_vm(const VmArgs& a, int grid, hipStream_t s);
hipError_t launch_gen_init(uint64_t inst_begin, uint64_t count, int n, int alg, int V, uint64_t seed, int32_t* out,
                           hipStream_t s);
}  // namespace psg
#endif
