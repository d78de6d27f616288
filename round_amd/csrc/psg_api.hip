// psg_api.hip — C ABI of include/psg.h: context, device buffers, launches.
//
// Replaces, for simulation, the reference's Runtime + InstanceHandler round
// loop (psync/runtime/Runtime.scala:60-93, psync/runtime/InstanceHandler.scala:164-258):
// one psg_run_batch call starts every instance of a range and runs all its
// rounds inside one kernel launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/psg.h"
#include "psg_device.hpp"
#include "psg_kernels.hpp"

namespace psg {

// Seeded synthetic initial values (the ConsensusIO.initialValue of every process).
__global__ void gen_init_kernel(uint64_t inst_begin, uint64_t count, int n, int alg, int V, uint64_t seed,
                                int32_t* out) {
  const uint64_t total = count * (uint64_t)n;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / (uint64_t)n;
    const int p = (int)(e - i * (uint64_t)n);
    const uint64_t w = rword(seed, inst_begin + i, ROUND_INIT, (uint32_t)p, 0);
    out[e] = alg == PSG_ALG_BENOR ? (int32_t)((uint32_t)w & 1u)
             : alg == PSG_ALG_TPC ? tpc_vote((uint32_t)w, (uint32_t)V)
             : alg == PSG_ALG_LATTICE ? lattice_init((uint32_t)w, (uint32_t)V)
                                  : 1 + (int32_t)mulhi32((uint32_t)w, (uint32_t)V);
  }
}

hipError_t launch_gen_init(uint64_t inst_begin, uint64_t count, int n, int alg, int V, uint64_t seed, int32_t* out,
                           hipStream_t s) {
  const uint64_t total = count * (uint64_t)n;
  const int grid = (int)std::min<uint64_t>((total + 255) / 256, 8192);
  if (grid == 0) return hipSuccess;
  hipLaunchKernelGGL(gen_init_kernel, dim3(grid), dim3(256), 0, s, inst_begin, count, n, alg, V, seed, out);
  return hipGetLastError();
}

}  // namespace psg

using namespace psg;

// Owning device buffer: pointer + capacity in elements.
template <class T>
struct DevBuf {
  T* p = nullptr;
  uint64_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {  // (what std::swap of two generations is made of)
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  // Room for count elements: nothing when they already fit, else free and reallocate (the contents go).
  hipError_t grow(uint64_t count) {
    if (count <= cap) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, sizeof(T) * count);
    if (e == hipSuccess) cap = count;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Every device allocation of a context (psg_destroy frees them as one).
struct psg_buffers {
  DevBuf<int32_t> d_init;
  DevBuf<double> d_init_f64;  // EpsilonConsensus: staged host Double inputs
  DevBuf<double> d_dec_f64;
  DevBuf<double> d_rec_f64;   // fetch path: [k][n][2] (decision, final x)
  DevBuf<int32_t> d_trace;    // psg_run_batch_spec: state trace of one chunk
  DevBuf<unsigned long long> d_vm_counters;
  DevBuf<int32_t> d_vm_err;
  DevBuf<int32_t> d_prog;     // code | slot_entry | slot_flags
  // explicit schedule (psg_load_schedule): ho[inst][k][p][W], crash[inst][p]
  DevBuf<uint64_t> d_ho;
  DevBuf<int32_t> d_crash;
  // search populations (psg_population_*): second buffers of the HO sets / inputs
  DevBuf<uint64_t> d_ho2;
  DevBuf<int32_t> d_init2;
  DevBuf<uint32_t> d_parent;
  DevBuf<uint8_t> d_op;
  // population models: the crash family's genome (crash rounds in d_crash, second buffer here;
  // crash-round delivery sets [count][n][W], two generations) and psg_population_live's output
  DevBuf<int32_t> d_crash2;
  DevBuf<uint64_t> d_partial, d_partial2;
  DevBuf<uint8_t> d_live;
  // shrinking (psg_shrink_*): the base schedule [R][n][W], its crash rounds and initial values [n],
  // its crash-round deliveries [n][W], the level's prefix, a chunk's edits; psg_population_links' output
  DevBuf<uint64_t> d_sh_base, d_sh_part;
  DevBuf<int32_t> d_sh_crash, d_sh_init;
  DevBuf<uint32_t> d_sh_pre;
  DevBuf<ShrinkEdit> d_sh_edit;
  DevBuf<uint32_t> d_links;
  DevBuf<int32_t> d_dec;
  DevBuf<uint8_t> d_dround;
  DevBuf<psg_instance_summary> d_inst;
  DevBuf<unsigned long long> d_counters;
  DevBuf<uint64_t> d_ids;
  DevBuf<psg_process_record> d_rec;
  // packed KSet (n > 64): state handed from the general-round kernel to the uniform-t tail
  // kernel, per batch row a header word, 64 lane words and n decisions (psg_kset.hip)
  DevBuf<uint64_t> d_hand;
};

struct psg_ctx : psg_buffers {
  psg_config cfg;
  int W = 1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint64_t cap = 0;
  bool init_f64_host = false;    // false: seeded Doubles generated inside the round kernel
  std::string module_path;       // native Spec code object currently loaded
  hipModule_t module = nullptr;
  hipFunction_t native_fn = nullptr;
  hipFunction_t fused_fn = nullptr, fused_x_fn = nullptr;  // fused Spec module: round kernel + Spec
  int32_t module_alg = 0;        // the module's psg_spec_alg (0: not recorded)
  bool staged = false;
  bool staged_host = false;      // the staged rows came from the host (else seeded values)
  uint64_t staged_begin = 0, staged_count = 0;
  // explicit schedule (psg_load_schedule)
  bool ho_loaded = false, ho_has_crash = false;
  bool pop_crash = false;  // the loaded schedule is a crash-family population (its genome is on the device)
  uint64_t ho_begin = 0, ho_count = 0;
  // shrink base (psg_shrink_begin), and the (level, arg) whose prefix d_sh_pre holds with its total
  bool sh_base = false, sh_has_crash = false, sh_counted = false;
  int32_t sh_level = 0;
  uint32_t sh_arg = 0;
  uint64_t sh_total = 0;
  uint64_t last_count = 0;
  int grid_max = 0;  // resident blocks for the algorithm's kernel
  std::string err;
  // multi-device context (cfg.n_devices > 0): one single-device context per listed
  // device; every call splits its range into contiguous slices, one per device
  std::vector<psg_ctx*> subs;
};

static thread_local std::string g_create_err;

static const char* const k_names_otr[] = {"Safety", "Invariant0", "Invariant1", "Invariant2",
                                          "Agreement", "Validity", "Integrity", "Irrevocability"};
static const char* const k_names_lv[] = {"Safety", "Invariant0", "Invariant1", "Agreement",
                                         "Validity", "Integrity", "Irrevocability"};
static const char* const k_names_benor[] = {"Safety", "Invariant0", "Agreement", "Irrevocability", "SafetyPredicate"};
static const char* const k_names_k[] = {"KAgreement", "KValidity"};
static const char* const k_names_eps[] = {"EpsAgreement", "EpsValidity", "SafetyPredicate"};
static const char* const k_names_tpc[] = {"Safety", "Invariant0", "UniformAgreement", "Validity"};
static const char* const k_names_lattice[] = {"Safety", "Invariant0", "Comparability", "DownwardValidity", "UpwardValidity",
                                              "Irrevocability"};
// the kernels record and flush exactly the named slots (psg_device.hpp)
static_assert(std::size(k_names_otr) == kOtrChecks, "k_names_otr and kOtrChecks disagree");
static_assert(std::size(k_names_lv) == kLvChecks, "k_names_lv and kLvChecks disagree");
static_assert(std::size(k_names_benor) == kBenOrChecks, "k_names_benor and kBenOrChecks disagree");
static_assert(std::size(k_names_k) == kKAgreeChecks, "k_names_k and kKAgreeChecks disagree");
static_assert(std::size(k_names_eps) == kEpsilonChecks, "k_names_eps and kEpsilonChecks disagree");
static_assert(std::size(k_names_tpc) == kTpcChecks, "k_names_tpc and kTpcChecks disagree");
static_assert(std::size(k_names_lattice) == kLatticeChecks, "k_names_lattice and kLatticeChecks disagree");

struct CheckNames {
  const char* const* name;
  int count;
  constexpr CheckNames() : name(nullptr), count(0) {}
  template <int N>
  constexpr CheckNames(const char* const (&a)[N]) : name(a), count(N) {}
};

// Everything the host layer knows about one algorithm; k_algs is indexed by PSG_ALG_*.
struct AlgRow {
  const char* class_name;  // the reference's class
  CheckNames checks;
  void (*defaults)(psg_config& cfg, int n);          // on top of psg_config_default's common part
  const char* (*invalid)(const psg_config& cfg);     // the parameter rule the config breaks, or null
  hipError_t (*launch)(const KArgs& a, int W, int grid, hipStream_t s);
  const void* (*kernel)(int W);                      // the variant the resident-block count is taken from
  // nullable: the variant a plain schedule (plain_schedule) is launched with, where the launcher has one
  const void* (*kernel_plain)(int W) = nullptr;
};

static const char* need_value_range(const psg_config& c) { return c.value_range < 1 ? "value_range must be >= 1" : nullptr; }

static void lv_defaults(psg_config& c, int n) {
  c.value_range = (1 << 15) - 1;
  c.sched.drop_log2 = 4;
  c.sched.good_p32 = 0;
  c.sched.crash_fmax = (n - 1) / 2;
}

static void crash_stop_defaults(psg_config& c, int rounds, int fmax) {  // loss-free links, at most fmax crashes
  c.param = 2;
  c.rounds = rounds;
  c.value_range = 1000000;
  c.sched.drop_log2 = 0;
  c.sched.good_p32 = 0;
  c.sched.crash_fmax = fmax;
}

static const char* otr_invalid(const psg_config& c) {
  if (const char* m = need_value_range(c)) return m;
  return c.param < 1 ? "OTR needs afterDecision >= 1" : nullptr;
}

static const AlgRow k_algs[] = {
    {},  // (PSG_ALG_* start at 1)
    {"example.OTR", k_names_otr, [](psg_config& c, int) { c.param = 2; /* afterDecision (Otr.scala:89) */ }, otr_invalid,
     launch_otr, otr_kernel_ptr, otr_plain_kernel_ptr},
    {"example.LastVoting", k_names_lv, lv_defaults, need_value_range, launch_lv, lv_kernel_ptr},
    {"example.FloodMin", k_names_k, [](psg_config& c, int) { crash_stop_defaults(c, 4, 2); },
     [](const psg_config& c) {
       if (const char* m = need_value_range(c)) return m;
       return c.param < 0 ? "FloodMin needs f >= 0" : nullptr;
     },
     launch_floodmin, floodmin_kernel_ptr},
    {"example.KSetAgreement", k_names_k, [](psg_config& c, int) { crash_stop_defaults(c, 16, 1); },
     [](const psg_config& c) {
       if (const char* m = need_value_range(c)) return m;
       return c.param < 1 ? "KSetAgreement needs k >= 1" : nullptr;
     },
     launch_kset, kset_kernel_ptr},
    {"example.BenOr", k_names_benor,
     [](psg_config& c, int n) {
       c.rounds = 64;
       c.value_range = 2;
       c.sched.drop_log2 = 2;
       c.sched.good_p32 = 0;
       c.sched.ho_min = n / 2;
     },
     [](const psg_config&) -> const char* { return nullptr; }, launch_benor, benor_kernel_ptr},
    {"example.OTR2", k_names_otr, [](psg_config& c, int) { c.param = 2; /* afterDecision (Otr2.scala:69) */ }, otr_invalid,
     launch_otr2, otr2_kernel_ptr, otr2_plain_kernel_ptr},
    {"example.ShortLastVoting", k_names_k,
     [](psg_config& c, int n) {
       lv_defaults(c, n);
       c.rounds = 30;
     },
     need_value_range, launch_slv, slv_kernel_ptr},
    {"example.KSetEarlyStopping", k_names_k,
     [](psg_config& c, int) {  // t = 2, k = 2 (KSetEarlyStopping.scala:63-67)
       crash_stop_defaults(c, 3, 2);
       c.param2 = 2;
     },
     [](const psg_config& c) {
       if (const char* m = need_value_range(c)) return m;
       return c.param < 0 || c.param2 < 1 ? "KSetEarlyStopping needs t >= 0 and k >= 1" : nullptr;
     },
     launch_kset_es, kset_es_kernel_ptr},
    {"example.EpsilonConsensus", k_names_eps,
     [](psg_config& c, int n) {  // f = 1, epsilon = 0.1 (Epsilon.scala:83-89)
       c.param = 1;
       c.real_param = 0.1;
       c.rounds = 12;
       c.sched.drop_log2 = 4;
       c.sched.good_p32 = 0;
       c.sched.ho_min = n - 2;  // |HO(p)| >= n - f
     },
     [](const psg_config& c) {
       return c.param < 1 || !(c.real_param > 0.0) ? "EpsilonConsensus needs f >= 1 and epsilon > 0" : nullptr;
     },
     launch_epsilon, epsilon_kernel_ptr},
    {"example.TwoPhaseCommit", k_names_tpc,
     [](psg_config& c, int n) {  // one phase; votes no w.p. 1/(2n): both outcomes stay common at any n
       c.param = 0;  // coord (TpcRunner: ProcessID(0), TwoPhaseCommit.scala:130)
       c.rounds = 3;
       c.value_range = 2 * n;
       c.sched.drop_log2 = 6;
       c.sched.good_p32 = 0;
     },
     [](const psg_config& c) {
       if (const char* m = need_value_range(c)) return m;
       return c.param < 0 || c.param >= c.n ? "TwoPhaseCommit needs 0 <= coord < n" : nullptr;
     },
     launch_tpc, tpc_kernel_ptr},
    {"example.LatticeAgreement", k_names_lattice,
     [](psg_config& c, int) {  // sets over {0..15}; a quarter of the links lost, no good rounds
       c.rounds = 8;
       c.value_range = 16;
       c.sched.drop_log2 = 2;
       c.sched.good_p32 = 0;
     },
     [](const psg_config& c) -> const char* {  // a set is an int32 bit mask >= 0: elements 0..30
       return c.value_range < 1 || c.value_range > 31 ? "LatticeAgreement needs 1 <= value_range <= 31" : nullptr;
     },
     launch_lattice, lattice_kernel_ptr},
};

constexpr int k_alg_rows = (int)(sizeof(k_algs) / sizeof(k_algs[0]));
static_assert(k_alg_rows == PSG_ALG_LATTICE + 1, "one row per PSG_ALG_*, in the enum's order");

// The row of an algorithm id; null: unknown algorithm.
static const AlgRow* alg_row(int alg) { return alg > 0 && alg < k_alg_rows ? &k_algs[alg] : nullptr; }

static int fail(psg_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

static int hip_fail(psg_ctx* c, hipError_t e, const char* what) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  return fail(c, e == hipErrorOutOfMemory ? PSG_ENOMEM : PSG_EIO, m);
}

#define HIPCHK(ctx, call)                                  \
  do {                                                     \
    hipError_t e_ = (call);                                \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
  } while (0)

// Profiling builds (-DPSG_PHASE_TIMERS=1): per-phase cycles, shader clock, wave lifetimes.
static void print_timers(const unsigned long long* host) {
  if (!PSG_PHASE_TIMERS) return;
  const unsigned long long* t = host + C_TIMER;
  const unsigned long long waves = t[T_WAVES], t0 = ~t[T_RT_MIN], span = t[T_RT_MAX] - ~t[T_RT_MIN];
  unsigned long long cyc = 0;
  std::fprintf(stderr, "psg phase cycles (kernel's own phase map):");
  for (int j = 0; j < NTIMERS; ++j) {
    std::fprintf(stderr, " t%d %llu", j, t[j]);
    cyc += t[j];
  }
  std::fprintf(stderr, "\n");
  std::fprintf(stderr, "psg wave lifetime: waves %llu, sum %llu rt ticks (100 MHz), span %llu ticks, mean/span %.3f, "
               "shader clock %.3f GHz\n", waves, t[T_RT_SUM], span,
               waves ? (double)t[T_RT_SUM] / waves / (double)span : 0.0,
               t[T_RT_SUM] ? 0.1 * cyc / (double)t[T_RT_SUM] : 0.0);
  // deciles of wave start and end times, as fractions of the span
  const size_t m = std::min<unsigned long long>(waves, NSTAMP_WAVES);
  std::vector<double> st(m), en(m);
  for (size_t w = 0; w < m; ++w) {
    st[w] = (double)(t[T_STAMPS + 2 * w] - t0) / span;
    en[w] = (double)(t[T_STAMPS + 1 + 2 * w] - t0) / span;
  }
  std::sort(st.begin(), st.end());
  std::sort(en.begin(), en.end());
  if (!m) return;
  std::fprintf(stderr, "psg wave start deciles:");
  for (int d = 0; d <= 10; ++d) std::fprintf(stderr, " %.3f", st[std::min(m - 1, d * m / 10)]);
  std::fprintf(stderr, "\npsg wave end deciles:  ");
  for (int d = 0; d <= 10; ++d) std::fprintf(stderr, " %.3f", en[std::min(m - 1, d * m / 10)]);
  std::fprintf(stderr, "\n");
}

static KArgs make_args(const psg_ctx* c) {
  KArgs a;
  std::memset(&a, 0, sizeof(a));
  const psg_config& f = c->cfg;
  a.seed = f.seed;
  a.n = f.n;
  a.R = f.rounds;
  a.V = f.value_range;
  a.param = f.param;
  a.param2 = f.param2;
  a.real_param = f.real_param;
  a.variant = f.variant;
  a.tiebreak = f.tiebreak;
  a.drop_log2 = f.sched.drop_log2;
  a.good_p32 = f.sched.good_p32;
  a.good_min = f.sched.good_min;
  // at most 0 crashes: f = mulhi32(w, fmax + 1) = 0 for every instance, so nobody crashes — the
  // kernels skip the instance's crash draws and the per-round crash sets (the same schedule)
  a.crash_fmax = f.sched.crash_fmax == 0 ? -1 : f.sched.crash_fmax;
  a.ho_min = f.sched.ho_min;
  a.self_bit = f.sched.self_bit;
  a.counters = c->d_counters;
  if (c->d_hand) {
    a.hand_hdr = c->d_hand;
    a.hand_meta = c->d_hand + c->cap;
    a.hand_dec = reinterpret_cast<int32_t*>(c->d_hand + c->cap * 65);
  }
  if (c->ho_loaded) {
    a.ho_in = c->d_ho;
    a.crash_in = c->ho_has_crash ? c->d_crash : nullptr;
    a.ho_base = c->ho_begin;
  }
  return a;
}

// Instances [begin, begin+count) must lie inside a loaded explicit schedule.
static int check_sched_range(psg_ctx* c, uint64_t begin, uint64_t count) {
  if (!c->ho_loaded || count == 0) return PSG_OK;
  if (begin < c->ho_begin || begin - c->ho_begin > c->ho_count || count > c->ho_count - (begin - c->ho_begin))
    return fail(c, PSG_ERANGE, "instances outside the loaded explicit schedule");
  return PSG_OK;
}

// Block geometry of the round kernels (Geometry<W>, psg_device.hpp) for the context's W.
static int threads_per_block(int W) { return with_w(W, 0, [](auto w) { return Geometry<w()>::kThreads; }); }
static int groups_per_block(int W) { return with_w(W, 1, [](auto w) { return Geometry<w()>::kGroups; }); }

static bool is_staged(const psg_ctx* c, uint64_t begin, uint64_t count) {
  return c->staged && c->staged_begin == begin && c->staged_count == count;
}

static void set_staged(psg_ctx* c, uint64_t begin, uint64_t count, bool from_host) {
  c->staged = true;
  c->staged_host = from_host;
  c->staged_begin = begin;
  c->staged_count = count;
}

// Counters of one launch -> summary. The Spec VM's counters hold the check slots and the termination
// histogram only (checks_only), which replace those of the round kernel's built-in checks.
static void fill_summary(psg_summary& s, const unsigned long long* host, int rounds, bool checks_only) {
  for (int i = 0; i < PSG_MAX_CHECKS; ++i) s.fail_count[i] = (int64_t)host[C_FAIL + i];
  for (int i = 0; i < rounds + 2; ++i) s.term_hist[i] = (int64_t)host[C_HIST + i];
  if (checks_only) return;
  s.active_process_rounds = (int64_t)host[C_ACTIVE];
  s.live_instance_rounds = (int64_t)host[C_LIVE];
  s.decided_processes = (int64_t)host[C_DECIDED];
  s.digest = (int64_t)host[C_DIGEST];
}

// acc += p, except kernel_ns: devices run side by side, chunks one after the other (the callers' choice)
static void summary_add(psg_summary& acc, const psg_summary& p) {
  acc.instances += p.instances;
  acc.process_rounds += p.process_rounds;
  acc.active_process_rounds += p.active_process_rounds;
  acc.live_instance_rounds += p.live_instance_rounds;
  for (int i = 0; i < PSG_MAX_CHECKS; ++i) acc.fail_count[i] += p.fail_count[i];
  acc.decided_processes += p.decided_processes;
  acc.digest = (int64_t)((uint64_t)acc.digest + (uint64_t)p.digest);
  for (int i = 0; i < PSG_MAX_ROUNDS + 2; ++i) acc.term_hist[i] += p.term_hist[i];
}

// One launch of the round kernel over `count` instances and its readback: zero the counters, launch
// (timed: between the context's events), copy the counters back, synchronise, fill *out (if given).
// The kernel is the algorithm's own (k_algs), or a fused Spec module's `fused` of at most fused_grid blocks.
// packable: the launch may go to a packed kernel (psg_run_batch's seeded built-in-check launch).
static int run_kernel(psg_ctx* c, KArgs& a, uint64_t count, psg_summary* out, bool timed, hipFunction_t fused = nullptr,
                      uint64_t fused_grid = 0, bool packable = false) {
  // several instances per wave: cfg.pack, a packed kernel for (alg, n), no explicit schedule
  const int pack_g = packable && !fused && c->cfg.pack == 1 && !a.ho_in ? psg_pack_width(c->cfg.alg, c->cfg.n) : 1;
  const int G = groups_per_block(c->W);
  const uint64_t want = (count + G - 1) / G;
  const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, fused ? fused_grid : (uint64_t)c->grid_max));
  HIPCHK(c, hipMemsetAsync(c->d_counters, 0, sizeof(unsigned long long) * NCOUNTERS_ALLOC, c->stream));
  if (timed) HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  if (fused) {
    void* params[] = {&a};
    HIPCHK(c, hipModuleLaunchKernel(fused, (unsigned)grid, 1, 1, (unsigned)threads_per_block(c->W), 1, 1, 0, c->stream,
                                    params, nullptr));
  } else if (pack_g > 1) {  // (the packed launcher sizes its own grid: 4 waves x pack_g rows per block)
    HIPCHK(c, launch_otr_packed(a, pack_g, c->stream));
  } else {
    HIPCHK(c, alg_row(c->cfg.alg)->launch(a, c->W, grid, c->stream));
  }
  if (timed) HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  unsigned long long host[NCOUNTERS_ALLOC];
  HIPCHK(c, hipMemcpyAsync(host, c->d_counters, sizeof(host), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // (a fused module shows its timers when it was compiled with -DPSG_PHASE_TIMERS=1 too:
  // formula.compile_native(defines=...))
  if (PSG_PHASE_TIMERS && std::getenv("PSG_PHASE_TIMERS")) print_timers(host);
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->instances = (int64_t)count;
    out->process_rounds = (int64_t)count * c->cfg.n * c->cfg.rounds;
    fill_summary(*out, host, c->cfg.rounds, false);
    if (timed) {
      float ms = 0.f;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
      out->kernel_ns = (int64_t)((double)ms * 1e6);
    }
  }
  return PSG_OK;
}

// psg_selftest_bitset: LongBitSet's operations (LongBitSet.scala:7-23) on Mask<W>, one lane
template <int W>
__global__ void bitset_selftest_kernel(const int32_t* ops, int n_ops, int32_t* out, int n_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Mask<W> m = mzero<W>();
  int o = 0;
  for (int i = 0; i < n_ops; ++i) {
    // index mod 64W on the signed value (Java's shift masks to mod 64 for W = 1; -1 -> 64W - 1)
    const int op = ops[2 * i], pos = ((ops[2 * i + 1] % (64 * W)) + 64 * W) % (64 * W);
    switch (op) {
      case 0: m = mzero<W>(); break;
      case 1: m = mfull<W>(64 * W); break;
      case 2: mset(m, pos); break;
      case 3: mclear(m, pos); break;
      case 4:
        if (mtest(m, pos)) mclear(m, pos);
        else mset(m, pos);
        break;
      case 5: if (o < n_out) out[o++] = mtest(m, pos) ? 1 : 0; break;
      case 6: if (o < n_out) out[o++] = mpopc(m); break;
      default: break;
    }
  }
}

// psg_selftest_eps_*: a self-test's scratch buffer filled from host data, and read back
constexpr int32_t kEpsSelftestMax = 1 << 20;  // items or cases per call
template <class T>
static int st_up(DevBuf<T>& d, const T* h, uint64_t count) {
  if (d.grow(count) != hipSuccess) return PSG_ENOMEM;
  return hipMemcpy(d, h, sizeof(T) * count, hipMemcpyHostToDevice) == hipSuccess ? PSG_OK : PSG_EIO;
}
template <class T>
static int st_down(T* h, const DevBuf<T>& d, uint64_t count) {
  return hipMemcpy(h, d, sizeof(T) * count, hipMemcpyDeviceToHost) == hipSuccess ? PSG_OK : PSG_EIO;
}

extern "C" {

int psg_config_default(psg_config* cfg, int32_t alg, int32_t n) {
  if (!cfg) return PSG_EINVAL;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->abi_version = PSG_ABI_VERSION;
  cfg->alg = alg;
  cfg->n = n;
  cfg->rounds = 20;
  cfg->seed = 1;
  cfg->value_range = 4;
  cfg->param = 0;
  cfg->tiebreak = PSG_TIE_CHAMP;
  cfg->batch_capacity = 1u << 20;
  cfg->sched.drop_log2 = 3;
  cfg->sched.good_p32 = 1u << 30;
  cfg->sched.good_min = -1;
  cfg->sched.crash_fmax = -1;
  cfg->sched.ho_min = -1;
  cfg->sched.self_bit = 1;
  const AlgRow* row = alg_row(alg);
  if (!row) return PSG_EINVAL;
  row->defaults(*cfg, n);
  return PSG_OK;
}

// The one rule of sub-wave packing (psg_subwave.hpp): G = 64 / P instances per wave, P the power
// of two >= n, at least 4, for the algorithms that have a packed kernel (run_kernel asks here).
int psg_pack_width(int32_t alg, int32_t n) {
  if (!alg_row(alg) || n < 1 || n > PSG_MAX_N) return PSG_EINVAL;
  if (alg != PSG_ALG_OTR || n > 32) return 1;
  int P = 4;
  while (P < n) P *= 2;
  return 64 / P;
}

int psg_check_count(int32_t alg) {
  const AlgRow* row = alg_row(alg);
  return row ? row->checks.count : 0;
}

const char* psg_check_name(int32_t alg, int32_t slot) {
  return slot >= 0 && slot < psg_check_count(alg) ? alg_row(alg)->checks.name[slot] : nullptr;
}

int psg_alg_from_class(const char* name) {
  if (!name) return PSG_EINVAL;
  for (int alg = 1; const AlgRow* row = alg_row(alg); ++alg)
    if (std::strcmp(row->class_name, name) == 0) return alg;
  return PSG_EINVAL;
}

const char* psg_create_error(void) { return g_create_err.c_str(); }

// The selftests run on the null stream of `device`; their scratch buffers free themselves.
static int selftest_device(int32_t device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return PSG_ENODEV;
  return hipSetDevice(device) == hipSuccess ? PSG_OK : PSG_ENODEV;
}

int psg_selftest_map_head(int32_t device, const uint64_t* sets, int32_t count, int32_t tiebreak, int32_t* out_first) {
  if (!sets || !out_first || count < 0) return PSG_EINVAL;
  if (tiebreak != PSG_TIE_CHAMP && tiebreak != PSG_TIE_MIN_PID) return PSG_EINVAL;
  if (count == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  DevBuf<uint64_t> d_sets;
  DevBuf<int32_t> d_out;
  if (d_sets.grow(count) != hipSuccess || d_out.grow(count) != hipSuccess) return PSG_ENOMEM;
  if (hipMemcpy(d_sets, sets, sizeof(uint64_t) * count, hipMemcpyHostToDevice) != hipSuccess ||
      launch_champ_selftest(d_sets, count, tiebreak, d_out, nullptr) != hipSuccess ||
      hipMemcpy(out_first, d_out, sizeof(int32_t) * count, hipMemcpyDeviceToHost) != hipSuccess)
    return PSG_EIO;
  return PSG_OK;
}

int psg_selftest_bitset(int32_t device, int32_t W, const int32_t* ops, int32_t n_ops, int32_t* out, int32_t n_out) {
  if (!ops || !out || n_ops < 0 || n_out < 0 || W < 1 || W > 4) return PSG_EINVAL;
  if (n_ops == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  DevBuf<int32_t> d_ops, d_out;
  if (d_ops.grow(2 * (uint64_t)n_ops) != hipSuccess || d_out.grow(n_out > 0 ? n_out : 1) != hipSuccess) return PSG_ENOMEM;
  if (hipMemcpy(d_ops, ops, sizeof(int32_t) * 2 * (size_t)n_ops, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_out, 0xFF, sizeof(int32_t) * d_out.cap) != hipSuccess)
    return PSG_EIO;
  const hipError_t e = with_w(W, hipErrorInvalidValue, [&](auto w) {
    hipLaunchKernelGGL(bitset_selftest_kernel<w()>, dim3(1), dim3(64), 0, nullptr, (const int32_t*)d_ops, n_ops,
                       (int32_t*)d_out, n_out);
    return hipGetLastError();
  });
  if (e != hipSuccess || (n_out > 0 && hipMemcpy(out, d_out, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost) != hipSuccess))
    return PSG_EIO;
  return PSG_OK;
}

// psg_selftest_eps_*: caller data up (st_up), one kernel of psg_epsilon.hip, results down (st_down)
int psg_selftest_eps_f64(int32_t device, const double* x, int32_t count, double* out_f64, int64_t* out_key, int32_t* out_i32) {
  if (!x || !out_f64 || !out_key || !out_i32 || count < 0 || count > kEpsSelftestMax) return PSG_EINVAL;
  if (count == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  const uint64_t c = (uint64_t)count;
  DevBuf<double> d_x, d_f;
  DevBuf<int64_t> d_k;
  DevBuf<int32_t> d_i;
  if (int rc = st_up(d_x, x, c)) return rc;
  if (d_f.grow(3 * c) != hipSuccess || d_k.grow(c) != hipSuccess || d_i.grow(3 * c) != hipSuccess) return PSG_ENOMEM;
  if (launch_eps_selftest_f64(d_x, count, d_f, d_k, d_i, nullptr) != hipSuccess) return PSG_EIO;
  if (int rc = st_down(out_f64, d_f, 3 * c)) return rc;
  if (int rc = st_down(out_key, d_k, c)) return rc;
  return st_down(out_i32, d_i, 3 * c);
}

int psg_selftest_eps_maxr(int32_t device, const double* q, const double* c, int32_t count, int32_t* out) {
  if (!q || !c || !out || count < 0 || count > kEpsSelftestMax) return PSG_EINVAL;
  if (count == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  DevBuf<double> d_q, d_c;
  DevBuf<int32_t> d_o;
  if (int rc = st_up(d_q, q, (uint64_t)count)) return rc;
  if (int rc = st_up(d_c, c, (uint64_t)count)) return rc;
  if (d_o.grow((uint64_t)count) != hipSuccess) return PSG_ENOMEM;
  if (launch_eps_selftest_maxr(d_q, d_c, count, d_o, nullptr) != hipSuccess) return PSG_EIO;
  return st_down(out, d_o, (uint64_t)count);
}

int psg_selftest_eps_sort(int32_t device, int32_t network, const double* x, const int32_t* n, int32_t cases, double* out_x,
                          int32_t* out_pid, int32_t* out_fallback) {
  if (!x || !n || !out_x || !out_pid || !out_fallback || cases < 0 || cases > kEpsSelftestMax) return PSG_EINVAL;
  if (network != 0 && network != 1) return PSG_EINVAL;
  for (int32_t i = 0; i < cases; ++i)
    if (n[i] < 1 || n[i] > 64) return PSG_EINVAL;
  if (cases == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  const uint64_t c = (uint64_t)cases;
  DevBuf<double> d_x, d_ox;
  DevBuf<int32_t> d_n, d_pid, d_fell;
  if (int rc = st_up(d_x, x, 64 * c)) return rc;
  if (int rc = st_up(d_n, n, c)) return rc;
  if (d_ox.grow(64 * c) != hipSuccess || d_pid.grow(64 * c) != hipSuccess || d_fell.grow(c) != hipSuccess) return PSG_ENOMEM;
  if (launch_eps_selftest_sort(network, d_x, d_n, cases, d_ox, d_pid, d_fell, nullptr) != hipSuccess) return PSG_EIO;
  if (int rc = st_down(out_x, d_ox, 64 * c)) return rc;
  if (int rc = st_down(out_pid, d_pid, 64 * c)) return rc;
  return st_down(out_fallback, d_fell, c);
}

int psg_selftest_eps_transpose(int32_t device, const uint64_t* rows, int32_t cases, uint64_t* out) {
  if (!rows || !out || cases < 0 || cases > kEpsSelftestMax) return PSG_EINVAL;
  if (cases == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  const uint64_t c = (uint64_t)cases;
  DevBuf<uint64_t> d_in, d_out;
  if (int rc = st_up(d_in, rows, 64 * c)) return rc;
  if (d_out.grow(64 * c) != hipSuccess) return PSG_ENOMEM;
  if (launch_eps_selftest_transpose(d_in, cases, d_out, nullptr) != hipSuccess) return PSG_EIO;
  return st_down(out, d_out, 64 * c);
}

int psg_selftest_eps_select(int32_t device, const uint64_t* masks, int32_t count, int32_t* out) {
  if (!masks || !out || count < 0 || count > kEpsSelftestMax) return PSG_EINVAL;
  for (int32_t i = 0; i < count; ++i)
    if (masks[i] == 0) return PSG_EINVAL;
  if (count == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  const uint64_t c = (uint64_t)count;
  DevBuf<uint64_t> d_m;
  DevBuf<int32_t> d_out;
  if (int rc = st_up(d_m, masks, c)) return rc;
  if (d_out.grow(64 * c) != hipSuccess) return PSG_ENOMEM;
  if (launch_eps_selftest_select(d_m, count, d_out, nullptr) != hipSuccess) return PSG_EIO;
  return st_down(out, d_out, 64 * c);
}

int psg_selftest_eps_members(int32_t device, const uint64_t* U, const int32_t* spid, int32_t cases, uint64_t* out) {
  if (!U || !spid || !out || cases < 0 || cases > kEpsSelftestMax) return PSG_EINVAL;
  for (int64_t i = 0; i < 64 * (int64_t)cases; ++i)
    if (spid[i] < 0 || spid[i] > 63) return PSG_EINVAL;
  if (cases == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  const uint64_t c = (uint64_t)cases;
  DevBuf<uint64_t> d_u, d_out;
  DevBuf<int32_t> d_p;
  if (int rc = st_up(d_u, U, 64 * c)) return rc;
  if (int rc = st_up(d_p, spid, 64 * c)) return rc;
  if (d_out.grow(64 * c) != hipSuccess) return PSG_ENOMEM;
  if (launch_eps_selftest_members(d_u, d_p, cases, d_out, nullptr) != hipSuccess) return PSG_EIO;
  return st_down(out, d_out, 64 * c);
}

int psg_selftest_eps_reduce(int32_t device, int32_t W, int32_t n, const int64_t* v, const uint8_t* in, int32_t cases,
                            int64_t* out) {
  if (!v || !in || !out || W < 1 || W > 4 || n < 1 || n > 64 * W || cases < 0 || cases > kEpsSelftestMax) return PSG_EINVAL;
  if (cases == 0) return PSG_OK;
  if (int rc = selftest_device(device)) return rc;
  const uint64_t c = (uint64_t)cases, per = 3ull * 64 * (uint64_t)W;
  DevBuf<int64_t> d_v, d_out;
  DevBuf<uint8_t> d_in;
  if (int rc = st_up(d_v, v, per * c)) return rc;
  if (int rc = st_up(d_in, in, per * c)) return rc;
  if (d_out.grow(9ull * (uint64_t)W * c) != hipSuccess) return PSG_ENOMEM;
  if (launch_eps_selftest_reduce(W, n, d_v, d_in, cases, d_out, nullptr) != hipSuccess) return PSG_EIO;
  return st_down(out, d_out, 9ull * (uint64_t)W * c);
}

static int validate(const psg_config* cfg, std::string& m) {
  if (!cfg) { m = "null config"; return PSG_EINVAL; }
  if (cfg->abi_version != PSG_ABI_VERSION) { m = "ABI version mismatch"; return PSG_EINVAL; }
  const AlgRow* row = alg_row(cfg->alg);
  if (!row) { m = "unknown algorithm"; return PSG_EINVAL; }
  if (cfg->n < 1 || cfg->n > PSG_MAX_N) { m = "n out of range 1..256"; return PSG_EINVAL; }
  if (cfg->rounds < 1 || cfg->rounds > PSG_MAX_ROUNDS) { m = "rounds out of range 1..250"; return PSG_EINVAL; }
  if (const char* why = row->invalid(*cfg)) { m = why; return PSG_EINVAL; }
  if (cfg->tiebreak != PSG_TIE_CHAMP && cfg->tiebreak != PSG_TIE_MIN_PID) { m = "bad tiebreak"; return PSG_EINVAL; }
  if (cfg->sched.drop_log2 > 16) { m = "drop_log2 > 16"; return PSG_EINVAL; }
  if (cfg->batch_capacity < 1) { m = "batch_capacity must be >= 1"; return PSG_EINVAL; }
  if (cfg->n_devices < 0 || cfg->n_devices > PSG_MAX_DEVICES) { m = "n_devices out of range 0..16"; return PSG_EINVAL; }
  if (cfg->pack != 0 && cfg->pack != 1) { m = "pack must be 0 or 1"; return PSG_EINVAL; }
  return PSG_OK;
}

// ---------------------------------------------------------------- multi-device contexts
// psg_config.n_devices > 0: the context owns one single-device context per listed
// device. A call over instances [begin, begin+count) gives device d the contiguous
// slice [begin + count*d/nd, begin + count*(d+1)/nd); the devices run concurrently,
// one host thread each, and their summaries are summed (kernel_ns: the maximum).
// Results equal a single-device run bit for bit (every draw is keyed on the global
// instance id). Under a loaded explicit schedule a multi-device run covers exactly
// the loaded range (its slices are the schedule's slices).
extern "C++" {
static void split(uint64_t count, size_t nd, size_t d, uint64_t& off, uint64_t& m) {
  off = count * d / nd;
  m = count * (d + 1) / nd - off;
}

template <class F>
static int par_subs(psg_ctx* c, F&& f) {
  const size_t nd = c->subs.size();
  std::vector<int> rc(nd, PSG_OK);
  std::vector<std::thread> th;
  try {
    th.reserve(nd);
    for (size_t d = 1; d < nd; ++d) th.emplace_back([&rc, &f, d] { rc[d] = f(d); });
  } catch (...) {
    for (auto& t : th) t.join();
    return fail(c, PSG_EIO, "could not start a host thread per device");
  }
  rc[0] = f(0);
  for (auto& t : th) t.join();
  for (size_t d = 0; d < nd; ++d)
    if (rc[d]) return fail(c, rc[d], "device " + std::to_string(c->cfg.devices[d]) + ": " + c->subs[d]->err);
  return PSG_OK;
}

// The slices of the last batch, in device order: f(the device's context, its offset in cells of n)
template <class F>
static int each_last_slice(psg_ctx* c, F&& f) {
  const uint64_t n = (uint64_t)c->cfg.n, nd = c->subs.size();
  for (size_t d = 0; d < nd; ++d) {
    uint64_t off, m;
    split(c->last_count, nd, d, off, m);
    if (!m) continue;  // an empty slice: the device ran nothing (its own last_count is 0)
    if (const int rc = f(c->subs[d], off * n))
      return fail(c, rc, "device " + std::to_string(c->cfg.devices[d]) + ": " + c->subs[d]->err);
  }
  return PSG_OK;
}
}  // extern "C++"

static int create_multi(psg_ctx** out, const psg_config* cfg) {
  psg_ctx* c = new (std::nothrow) psg_ctx();
  if (!c) return PSG_ENOMEM;
  c->cfg = *cfg;
  c->W = (cfg->n + 63) / 64;
  c->cap = cfg->batch_capacity;
  const int nd = cfg->n_devices;
  for (int d = 0; d < nd; ++d) {
    psg_config sc = *cfg;
    sc.n_devices = 0;
    sc.device = cfg->devices[d];
    sc.batch_capacity = (cfg->batch_capacity + nd - 1) / nd;
    psg_ctx* sub = nullptr;
    const int rc = psg_create(&sub, &sc);
    if (rc) {
      g_create_err = "device " + std::to_string(cfg->devices[d]) + ": " + g_create_err;
      psg_destroy(c);
      return rc;
    }
    c->subs.push_back(sub);
  }
  *out = c;
  return PSG_OK;
}

int psg_create(psg_ctx** out, const psg_config* cfg) {
  if (!out) return PSG_EINVAL;
  *out = nullptr;
  std::string m;
  int rc = validate(cfg, m);
  if (rc) { g_create_err = m; return rc; }
  if (cfg->n_devices > 0) return create_multi(out, cfg);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) { g_create_err = "no HIP device"; return PSG_ENODEV; }
  if (cfg->device < 0 || cfg->device >= ndev) { g_create_err = "device ordinal out of range"; return PSG_ENODEV; }
  psg_ctx* c = new (std::nothrow) psg_ctx();
  if (!c) return PSG_ENOMEM;
  c->cfg = *cfg;
  c->W = (cfg->n + 63) / 64;
  c->cap = cfg->batch_capacity;
  auto bail = [&](hipError_t err, const char* what) {
    g_create_err = std::string(what) + ": " + hipGetErrorString(err);
    psg_destroy(c);
    return err == hipErrorOutOfMemory ? PSG_ENOMEM : PSG_EIO;
  };
#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return bail(e_, #call); } while (0)
  CK(hipSetDevice(cfg->device));
  CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  CK(hipEventCreate(&c->ev0));
  CK(hipEventCreate(&c->ev1));
  const uint64_t cells = c->cap * (uint64_t)cfg->n;
  if (cfg->alg == PSG_ALG_EPSILON) {
    CK(c->d_init_f64.grow(cells));
    CK(c->d_dec_f64.grow(cells));
  } else {
    CK(c->d_init.grow(cells));
  }
  CK(c->d_dec.grow(cells));
  CK(c->d_dround.grow(cells));
  CK(c->d_inst.grow(c->cap));
  CK(c->d_counters.grow(NCOUNTERS_ALLOC));
  if (cfg->alg == PSG_ALG_KSET && c->W > 1)  // 520 + 4n bytes per batch row (psg_kset.hip hand-off)
    CK(c->d_hand.grow(65 * c->cap + (cells + 1) / 2));  // (the int32 decisions: two to a word)
  // the grid is sized from the kernel this context's seeded launches go to (the schedule is fixed here)
  const AlgRow* row = alg_row(cfg->alg);
  const bool plain = row->kernel_plain && plain_schedule(make_args(c));
  int per_cu = 0;
  CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, plain ? row->kernel_plain(c->W) : row->kernel(c->W),
                                                  threads_per_block(c->W), 0));
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, cfg->device));
  if (per_cu < 1) per_cu = 1;
  c->grid_max = prop.multiProcessorCount * per_cu;
#undef CK
  *out = c;
  return PSG_OK;
}

// multi-device psg_load_inputs / _f64: each device stages its slice
static int multi_load_inputs(psg_ctx* c, uint64_t inst_begin, uint64_t count, const int32_t* host_init,
                             const double* host_f64, bool f64) {
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  const uint64_t n = (uint64_t)c->cfg.n, nd = c->subs.size();
  const int rc = par_subs(c, [&](size_t d) {
    uint64_t off, m;
    split(count, nd, d, off, m);
    return f64 ? psg_load_inputs_f64(c->subs[d], inst_begin + off, m, host_f64 ? host_f64 + off * n : nullptr)
               : psg_load_inputs(c->subs[d], inst_begin + off, m, host_init ? host_init + off * n : nullptr);
  });
  if (rc) return rc;
  set_staged(c, inst_begin, count, f64 ? host_f64 != nullptr : host_init != nullptr);
  return PSG_OK;
}

int psg_load_inputs(psg_ctx* c, uint64_t inst_begin, uint64_t count, const int32_t* host_init) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty()) {
    if (c->cfg.alg == PSG_ALG_EPSILON && host_init)
      return fail(c, PSG_EINVAL, "EpsilonConsensus takes Double inputs: use psg_load_inputs_f64");
    return multi_load_inputs(c, inst_begin, count, host_init, nullptr, c->cfg.alg == PSG_ALG_EPSILON);
  }
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  if (c->cfg.alg == PSG_ALG_EPSILON) {
    if (host_init) return fail(c, PSG_EINVAL, "EpsilonConsensus takes Double inputs: use psg_load_inputs_f64");
    return psg_load_inputs_f64(c, inst_begin, count, nullptr);
  }
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const uint64_t cells = count * (uint64_t)c->cfg.n;
  if (host_init) {
    HIPCHK(c, hipMemcpyAsync(c->d_init, host_init, sizeof(int32_t) * cells, hipMemcpyHostToDevice, c->stream));
  } else {
    HIPCHK(c, launch_gen_init(inst_begin, count, c->cfg.n, c->cfg.alg, c->cfg.value_range, c->cfg.seed, c->d_init,
                              c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  set_staged(c, inst_begin, count, host_init != nullptr);
  return PSG_OK;
}

int psg_load_inputs_f64(psg_ctx* c, uint64_t inst_begin, uint64_t count, const double* host_init) {
  if (!c) return PSG_EINVAL;
  if (c->cfg.alg != PSG_ALG_EPSILON) return fail(c, PSG_EINVAL, "Double inputs are for EpsilonConsensus only");
  if (!c->subs.empty()) return multi_load_inputs(c, inst_begin, count, nullptr, host_init, true);
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (host_init) {
    const uint64_t cells = count * (uint64_t)c->cfg.n;
    HIPCHK(c, hipMemcpyAsync(c->d_init_f64, host_init, sizeof(double) * cells, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  c->init_f64_host = host_init != nullptr;
  set_staged(c, inst_begin, count, host_init != nullptr);
  return PSG_OK;
}

// multi-device psg_run_batch / psg_run_batch_spec (prog != nullptr)
static int multi_run(psg_ctx* c, uint64_t inst_begin, uint64_t count, const psg_spec_program* prog, psg_summary* out,
                     psg_instance_summary* per_inst) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  if (count == 0) {  // the library's "last batch" is the single source of truth (JNI checks use it)
    c->last_count = 0;
    for (psg_ctx* s : c->subs) s->last_count = 0;
    return PSG_OK;
  }
  if (c->ho_loaded && (inst_begin != c->ho_begin || count != c->ho_count))
    return fail(c, PSG_ERANGE, "a multi-device run under an explicit schedule covers exactly the loaded range");
  if (!is_staged(c, inst_begin, count)) {
    const int rc = psg_load_inputs(c, inst_begin, count, nullptr);  // seeded, like a single device
    if (rc) return rc;
  }
  const size_t nd = c->subs.size();
  std::vector<psg_summary> parts(nd);
  const int rc = par_subs(c, [&](size_t d) {
    uint64_t off, m;
    split(count, nd, d, off, m);
    psg_instance_summary* pi = per_inst ? per_inst + off : nullptr;
    return prog ? psg_run_batch_spec(c->subs[d], inst_begin + off, m, prog, &parts[d], pi)
                : psg_run_batch(c->subs[d], inst_begin + off, m, &parts[d], pi);
  });
  if (rc) return rc;
  if (out)
    for (size_t d = 0; d < nd; ++d) {
      summary_add(*out, parts[d]);
      out->kernel_ns = std::max(out->kernel_ns, parts[d].kernel_ns);  // the devices ran side by side
    }
  c->last_count = count;
  return PSG_OK;
}

// One launch over a whole batch from its staged inputs (seeded ones unless the caller staged this
// range): psg_run_batch, and psg_run_batch_spec through a fused module's round kernel.
static int run_whole_batch(psg_ctx* c, uint64_t inst_begin, uint64_t count, psg_summary* out,
                           psg_instance_summary* per_inst, hipFunction_t fused = nullptr, uint64_t fused_grid = 0,
                           bool packable = false) {
  if (!is_staged(c, inst_begin, count)) {
    int rc = psg_load_inputs(c, inst_begin, count, nullptr);
    if (rc) return rc;
  }
  KArgs a = make_args(c);
  a.inst_begin = inst_begin;
  a.count = count;
  a.init = c->d_init;
  if (c->cfg.alg == PSG_ALG_EPSILON) {
    a.init = nullptr;
    a.init_f64 = c->init_f64_host ? c->d_init_f64 : nullptr;  // else seeded inside the kernel
    a.out_dec_f64 = c->d_dec_f64;
  }
  a.out_decision = c->d_dec;
  a.out_dround = c->d_dround;
  a.out_inst = c->d_inst;
  int rc = run_kernel(c, a, count, out, true, fused, fused_grid, packable);
  if (rc) return rc;
  c->last_count = count;
  if (per_inst) {
    HIPCHK(c, hipMemcpy(per_inst, c->d_inst, sizeof(psg_instance_summary) * count, hipMemcpyDeviceToHost));
  }
  return PSG_OK;
}

int psg_run_batch(psg_ctx* c, uint64_t inst_begin, uint64_t count, psg_summary* out, psg_instance_summary* per_inst) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty()) return multi_run(c, inst_begin, count, nullptr, out, per_inst);
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  if (count == 0) {
    if (out) std::memset(out, 0, sizeof(*out));
    c->last_count = 0;
    return PSG_OK;
  }
  if (int rc = check_sched_range(c, inst_begin, count)) return rc;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  return run_whole_batch(c, inst_begin, count, out, per_inst, nullptr, 0, /*packable=*/true);
}

static int validate_prog(const psg_spec_program* p, std::string& m) {
  if (!p || !p->code || !p->slot_entry || !p->slot_flags) { m = "null spec program"; return PSG_EINVAL; }
  if (p->n_slots < 1 || p->n_slots > PSG_MAX_CHECKS) { m = "spec program needs 1..12 slots"; return PSG_EINVAL; }
  if (p->n_words < 1 || p->n_words > (1 << 20)) { m = "bad spec program length"; return PSG_EINVAL; }
  if (p->n_vars < 0 || p->n_vars > 16) { m = "spec program uses more than 16 bound variables"; return PSG_EINVAL; }
  for (int s = 0; s < p->n_slots; ++s)
    if (p->slot_entry[s] < 0 || p->slot_entry[s] >= p->n_words) { m = "slot entry out of range"; return PSG_EINVAL; }
  if (p->term_entry >= p->n_words) { m = "termination entry out of range"; return PSG_EINVAL; }
  // structural check: opcodes known, quantifier ends in range, variables in range
  for (int pc = 0; pc < p->n_words;) {
    const int32_t w = p->code[pc];
    const int op = w & 0xff, a = (w >> 8) & 0xff;
    if (op > PSG_OP_COORD) { m = "unknown opcode at " + std::to_string(pc); return PSG_EINVAL; }
    if ((op == PSG_OP_VAR || op == PSG_OP_BIND) && a >= 16) { m = "variable out of range"; return PSG_EINVAL; }
    if (op == PSG_OP_FIELD && (a >= PSG_NFIELDS || (w >> 16) < 0 || (w >> 16) > PSG_TAG_INIT)) {
      m = "bad field / tag at " + std::to_string(pc);
      return PSG_EINVAL;
    }
    ++pc;
    if (op == PSG_OP_IMM32) ++pc;
    if (op == PSG_OP_QBEGIN) {
      if (a > PSG_Q_EXISTS_VI || (w >> 16) < 0 || (w >> 16) >= 16 || pc >= p->n_words) {
        m = "bad quantifier at " + std::to_string(pc - 1);
        return PSG_EINVAL;
      }
      const int32_t end = p->code[pc];
      if (end <= pc || end >= p->n_words || (p->code[end] & 0xff) != PSG_OP_QEND) {
        m = "quantifier end mismatch at " + std::to_string(pc - 1);
        return PSG_EINVAL;
      }
      ++pc;
      if (a == PSG_Q_EXISTS_VI) {
        if (pc >= p->n_words) { m = "truncated V.exists"; return PSG_EINVAL; }
        pc += 1 + ((p->code[pc] >> 16) & 0xffff);
      }
    }
  }
  return PSG_OK;
}

// Fields a (validated) program reads: FIELD operands and V.exists field sets.
static uint32_t prog_fields(const psg_spec_program* p) {
  uint32_t m = 0;
  for (int pc = 0; pc < p->n_words;) {
    const int32_t w = p->code[pc];
    const int op = w & 0xff, a = (w >> 8) & 0xff;
    if (op == PSG_OP_FIELD) m |= 1u << a;
    ++pc;
    if (op == PSG_OP_IMM32) ++pc;
    if (op == PSG_OP_QBEGIN) {
      ++pc;
      if (a == PSG_Q_EXISTS_VI) {
        const int nf = (p->code[pc] >> 16) & 0xffff;
        for (int k = 0; k < nf; ++k) m |= 1u << (p->code[pc + 1 + k] & 0xff);
        pc += 1 + nf;
      }
    }
  }
  return m & ((1u << PSG_NFIELDS) - 1u);
}

int psg_last_batch_count(const psg_ctx* c, uint64_t* count) {
  if (!c || !count) return PSG_EINVAL;
  *count = c->last_count;
  return PSG_OK;
}

int psg_copy_decisions(psg_ctx* c, int32_t* decision, int32_t* decision_round) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty())
    return each_last_slice(c, [&](psg_ctx* s, uint64_t at) {
      return psg_copy_decisions(s, decision ? decision + at : nullptr, decision_round ? decision_round + at : nullptr);
    });
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const uint64_t cells = c->last_count * (uint64_t)c->cfg.n;
  if (decision) HIPCHK(c, hipMemcpy(decision, c->d_dec, sizeof(int32_t) * cells, hipMemcpyDeviceToHost));
  if (decision_round) {
    uint8_t* tmp = new (std::nothrow) uint8_t[cells ? cells : 1];
    if (!tmp) return fail(c, PSG_ENOMEM, "host allocation failed");
    hipError_t e = hipMemcpy(tmp, c->d_dround, cells, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { delete[] tmp; return hip_fail(c, e, "hipMemcpy(dround)"); }
    for (uint64_t k = 0; k < cells; ++k) decision_round[k] = tmp[k] == 0xFF ? -1 : (int32_t)tmp[k];
    delete[] tmp;
  }
  return PSG_OK;
}

int psg_run_batch_spec(psg_ctx* c, uint64_t inst_begin, uint64_t count, const psg_spec_program* prog,
                       psg_summary* out, psg_instance_summary* per_inst) {
  if (!c) return PSG_EINVAL;
  if (c->cfg.alg == PSG_ALG_EPSILON) return fail(c, PSG_EINVAL, "Spec programs need integer state (not EpsilonConsensus)");
  std::string m;
  if (validate_prog(prog, m)) return fail(c, PSG_EINVAL, m);
  if (prog->alg != 0 && prog->alg != c->cfg.alg)
    return fail(c, PSG_EINVAL, "spec program was compiled for algorithm " + std::to_string(prog->alg) +
                                   ", the context runs " + std::to_string(c->cfg.alg));
  if (!c->subs.empty()) return multi_run(c, inst_begin, count, prog, out, per_inst);
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  if (int rc = check_sched_range(c, inst_begin, count)) return rc;
  if (out) std::memset(out, 0, sizeof(*out));
  if (count == 0) {
    c->last_count = 0;
    return PSG_OK;
  }
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const int n = c->cfg.n, R = c->cfg.rounds;
  // program: code | slot_entry | slot_flags
  const size_t words = (size_t)prog->n_words + 2 * (size_t)prog->n_slots;
  HIPCHK(c, c->d_prog.grow(words));
  HIPCHK(c, hipMemcpy(c->d_prog, prog->code, sizeof(int32_t) * prog->n_words, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->d_prog + prog->n_words, prog->slot_entry, sizeof(int32_t) * prog->n_slots,
                      hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->d_prog + prog->n_words + prog->n_slots, prog->slot_flags, sizeof(int32_t) * prog->n_slots,
                      hipMemcpyHostToDevice));
  // native lowering of the same Spec (round_amd/formula.py compile_native), if given
  const bool native = prog->module_path != nullptr;
  if (native && c->module_path != prog->module_path) {
    if (c->module) (void)hipModuleUnload(c->module);
    c->module = nullptr;
    c->native_fn = nullptr;
    c->fused_fn = c->fused_x_fn = nullptr;
    c->module_path.clear();
    HIPCHK(c, hipModuleLoad(&c->module, prog->module_path));
    const std::string name = "psg_spec_native_w" + std::to_string(c->W);
    HIPCHK(c, hipModuleGetFunction(&c->native_fn, c->module, name.c_str()));
    // the algorithm the module was generated for (round_amd/formula.py writes psg_spec_alg)
    c->module_alg = 0;
    hipDeviceptr_t gp = nullptr;
    size_t gsz = 0;
    if (hipModuleGetGlobal(&gp, &gsz, c->module, "psg_spec_alg") == hipSuccess && gsz == sizeof(int32_t))
      HIPCHK(c, hipMemcpyDtoH(&c->module_alg, gp, sizeof(int32_t)));
    (void)hipGetLastError();
    // fused modules (compile_native(fused=True)) also hold the round kernel with the Spec as its hook
    const std::string aw = "a" + std::to_string(c->cfg.alg) + "_w" + std::to_string(c->W);
    const std::string fw = "psg_fused_" + aw, fx = "psg_fused_x_" + aw;
    if (hipModuleGetFunction(&c->fused_fn, c->module, fw.c_str()) != hipSuccess) c->fused_fn = nullptr;
    if (hipModuleGetFunction(&c->fused_x_fn, c->module, fx.c_str()) != hipSuccess) c->fused_x_fn = nullptr;
    (void)hipGetLastError();
    c->module_path = prog->module_path;
  }
  if (native && c->module_alg != 0 && c->module_alg != c->cfg.alg)
    return fail(c, PSG_EINVAL, "spec module " + c->module_path + " was generated for algorithm " +
                                   std::to_string(c->module_alg) + ", the context runs " + std::to_string(c->cfg.alg));
  if (native && (c->ho_loaded ? c->fused_x_fn : c->fused_fn)) {
    // one launch: rounds + Spec from registers (no trace, no chunks)
    hipFunction_t fn = c->ho_loaded ? c->fused_x_fn : c->fused_fn;
    int per_cu = 0, cus = 0;
    HIPCHK(c, hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads_per_block(c->W), 0));
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->cfg.device));
    return run_whole_batch(c, inst_begin, count, out, per_inst, fn, (uint64_t)cus * std::max(per_cu, 1));
  }
  // trace chunk: <= PSG_SPEC_TRACE_MB (default 2048) MiB of [R+1][fields][n] int32 rows
  uint64_t budget = 2048ull << 20;
  if (const char* e = std::getenv("PSG_SPEC_TRACE_MB")) {
    const long long mb = std::atoll(e);
    if (mb > 0) budget = (uint64_t)mb << 20;
  }
  const uint64_t per_inst_bytes = (uint64_t)(R + 1) * PSG_NFIELDS * (uint64_t)n * sizeof(int32_t);
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(count, budget / per_inst_bytes));
  HIPCHK(c, c->d_trace.grow(per_inst_bytes / sizeof(int32_t) * chunk));
  HIPCHK(c, c->d_vm_counters.grow(NCOUNTERS));
  HIPCHK(c, c->d_vm_err.grow(1));
  HIPCHK(c, hipMemsetAsync(c->d_vm_err, 0, sizeof(int32_t), c->stream));
  const bool staged = is_staged(c, inst_begin, count);
  const uint32_t fields = prog_fields(prog);
  psg_summary acc;
  std::memset(&acc, 0, sizeof(acc));
  int vm_grid = 0;
  HIPCHK(c, hipDeviceGetAttribute(&vm_grid, hipDeviceAttributeMultiprocessorCount, c->cfg.device));
  vm_grid *= 8;
  for (uint64_t off = 0; off < count; off += chunk) {
    const uint64_t m_cnt = std::min<uint64_t>(chunk, count - off);
    KArgs a = make_args(c);
    a.inst_begin = inst_begin + off;
    a.count = m_cnt;
    a.init = staged ? c->d_init + off * (uint64_t)n : nullptr;  // else seeded by the kernel
    a.out_decision = c->d_dec + off * (uint64_t)n;
    a.out_dround = c->d_dround + off * (uint64_t)n;
    a.out_inst = c->d_inst + off;
    a.trace = c->d_trace;
    a.trace_fields = fields;
    psg_summary part;
    int rc = run_kernel(c, a, m_cnt, &part, true);
    if (rc) return rc;
    VmArgs v;
    v.code = c->d_prog;
    v.slot_entry = c->d_prog + prog->n_words;
    v.slot_flags = c->d_prog + prog->n_words + prog->n_slots;
    v.n_slots = prog->n_slots;
    v.term_entry = prog->term_entry;
    v.n_words = prog->n_words;
    v.trace = c->d_trace;
    v.count = m_cnt;
    v.n = n;
    v.R = R;
    v.out_inst = c->d_inst + off;
    v.counters = c->d_vm_counters;
    v.err = c->d_vm_err;
    HIPCHK(c, hipMemsetAsync(c->d_vm_counters, 0, sizeof(unsigned long long) * NCOUNTERS, c->stream));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (native) {
      const int G = groups_per_block(c->W);
      const unsigned grid = (unsigned)std::min<uint64_t>((m_cnt + G - 1) / G, (uint64_t)vm_grid);
      void* params[] = {&v};
      HIPCHK(c, hipModuleLaunchKernel(c->native_fn, grid, 1, 1, (unsigned)threads_per_block(c->W), 1, 1, 0, c->stream,
                                      params, nullptr));
    } else {
      HIPCHK(c, launch_spec_vm(v, (int)std::min<uint64_t>(m_cnt, (uint64_t)vm_grid), c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    unsigned long long host[NCOUNTERS];
    HIPCHK(c, hipMemcpyAsync(host, c->d_vm_counters, sizeof(host), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    fill_summary(part, host, R, true);  // the Spec's slots and Termination, not the built-in checks'
    summary_add(acc, part);
    acc.kernel_ns += part.kernel_ns + (int64_t)((double)ms * 1e6);  // the chunks ran one after the other
  }
  int32_t verr = 0;
  HIPCHK(c, hipMemcpy(&verr, c->d_vm_err, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (verr) {
    return fail(c, PSG_ERANGE,
                std::string("spec program exceeded interpreter limits (flags ") + std::to_string(verr) +
                    "; 1 stack > 24, 2 nesting > 12, 4 V.exists candidates > 1024 or nesting > 2, 8 bad opcode)");
  }
  c->last_count = count;
  if (per_inst)
    HIPCHK(c, hipMemcpy(per_inst, c->d_inst, sizeof(psg_instance_summary) * count, hipMemcpyDeviceToHost));
  if (out) *out = acc;
  return PSG_OK;
}

int psg_copy_decisions_f64(psg_ctx* c, double* decision, int32_t* decision_round) {
  if (!c) return PSG_EINVAL;
  if (c->cfg.alg != PSG_ALG_EPSILON) return fail(c, PSG_EINVAL, "Double decisions are for EpsilonConsensus only");
  if (!c->subs.empty())
    return each_last_slice(c, [&](psg_ctx* s, uint64_t at) {
      return psg_copy_decisions_f64(s, decision ? decision + at : nullptr, decision_round ? decision_round + at : nullptr);
    });
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const uint64_t cells = c->last_count * (uint64_t)c->cfg.n;
  if (decision) HIPCHK(c, hipMemcpy(decision, c->d_dec_f64, sizeof(double) * cells, hipMemcpyDeviceToHost));
  return decision_round ? psg_copy_decisions(c, nullptr, decision_round) : PSG_OK;
}

static int fetch_impl(psg_ctx* c, const uint64_t* ids, size_t k, psg_instance_summary* sums,
                      psg_process_record* procs, double* fdec, double* fx, bool force_seeded = false);

// multi-device fetch: each id goes to the device holding its schedule slice (explicit
// schedule) or its staged host-input slice; otherwise ids are dealt out in contiguous
// chunks and re-executed from seeded inputs (what staged seeded rows hold anyway).
static int multi_fetch(psg_ctx* c, const uint64_t* ids, size_t k, psg_instance_summary* sums,
                       psg_process_record* procs, double* fdec, double* fx) {
  if (k > c->cap) return fail(c, PSG_ERANGE, "fetch count exceeds batch_capacity");
  const size_t nd = c->subs.size();
  const uint64_t n = (uint64_t)c->cfg.n;
  bool all_staged = c->staged && c->staged_host;
  for (size_t j = 0; j < k && all_staged; ++j)
    all_staged = ids[j] >= c->staged_begin && ids[j] - c->staged_begin < c->staged_count;
  auto owner = [&](uint64_t id, uint64_t begin, uint64_t count) {  // device whose slice holds id
    size_t d = (size_t)((id - begin) * nd / count);
    uint64_t off, m;
    for (;; ++d) {
      split(count, nd, d, off, m);
      if (id - begin < off + m || d + 1 == nd) return d;
    }
  };
  std::vector<std::vector<size_t>> pos(nd);
  for (size_t j = 0; j < k; ++j) {
    size_t d;
    if (c->ho_loaded) {
      if (ids[j] < c->ho_begin || ids[j] - c->ho_begin >= c->ho_count)
        return fail(c, PSG_ERANGE, "instances outside the loaded explicit schedule");
      if (all_staged && (c->staged_begin != c->ho_begin || c->staged_count != c->ho_count))
        return fail(c, PSG_EINVAL, "multi-device fetch: staged host inputs and the explicit schedule cover different ranges");
      d = owner(ids[j], c->ho_begin, c->ho_count);
    } else if (all_staged) {
      d = owner(ids[j], c->staged_begin, c->staged_count);
    } else {
      d = j * nd / k;
    }
    pos[d].push_back(j);
  }
  return par_subs(c, [&](size_t d) {
    psg_ctx* s = c->subs[d];
    const std::vector<size_t>& P = pos[d];
    const size_t chunk = (size_t)std::max<uint64_t>(1, s->cap);
    std::vector<uint64_t> sid;
    std::vector<psg_instance_summary> ss;
    std::vector<psg_process_record> sp;
    std::vector<double> sd, sx;
    for (size_t a = 0; a < P.size(); a += chunk) {
      const size_t m = std::min(chunk, P.size() - a);
      sid.resize(m);
      for (size_t t = 0; t < m; ++t) sid[t] = ids[P[a + t]];
      ss.resize(m);
      if (procs) sp.resize(m * n);
      if (fdec) sd.resize(m * n);
      if (fx) sx.resize(m * n);
      const int rc = fetch_impl(s, sid.data(), m, ss.data(), procs ? sp.data() : nullptr, fdec ? sd.data() : nullptr,
                                fx ? sx.data() : nullptr, !all_staged);
      if (rc) return rc;
      for (size_t t = 0; t < m; ++t) {
        const size_t j = P[a + t];
        if (sums) sums[j] = ss[t];
        if (procs) std::memcpy(procs + j * n, sp.data() + t * n, sizeof(psg_process_record) * n);
        if (fdec) std::memcpy(fdec + j * n, sd.data() + t * n, sizeof(double) * n);
        if (fx) std::memcpy(fx + j * n, sx.data() + t * n, sizeof(double) * n);
      }
    }
    return PSG_OK;
  });
}

int psg_fetch_instances(psg_ctx* c, const uint64_t* ids, size_t k, psg_instance_summary* sums,
                        psg_process_record* procs) {
  if (c && !c->subs.empty()) {
    if (!ids && k) return PSG_EINVAL;
    return multi_fetch(c, ids, k, sums, procs, nullptr, nullptr);
  }
  return fetch_impl(c, ids, k, sums, procs, nullptr, nullptr);
}

int psg_fetch_instances_f64(psg_ctx* c, const uint64_t* ids, size_t k, psg_instance_summary* sums,
                            psg_process_record* procs, double* decision, double* final_x) {
  if (c && c->cfg.alg != PSG_ALG_EPSILON) return fail(c, PSG_EINVAL, "Double records are for EpsilonConsensus only");
  if (c && !c->subs.empty()) {
    if (!ids && k) return PSG_EINVAL;
    return multi_fetch(c, ids, k, sums, procs, decision, final_x);
  }
  return fetch_impl(c, ids, k, sums, procs, decision, final_x);
}

static int fetch_impl(psg_ctx* c, const uint64_t* ids, size_t k, psg_instance_summary* sums,
                      psg_process_record* procs, double* fdec, double* fx, bool force_seeded) {
  if (!c || (!ids && k)) return PSG_EINVAL;
  if (k == 0) return PSG_OK;
  if (k > c->cap) return fail(c, PSG_ERANGE, "fetch count exceeds batch_capacity");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, c->d_ids.grow(k));
  HIPCHK(c, c->d_rec.grow(k * (uint64_t)c->cfg.n));
  if (c->cfg.alg == PSG_ALG_EPSILON) HIPCHK(c, c->d_rec_f64.grow(2 * k * (uint64_t)c->cfg.n));
  bool in_staged = c->staged && !force_seeded;
  for (size_t j = 0; j < k; ++j) {
    if (int rc = check_sched_range(c, ids[j], 1)) return rc;
    if (ids[j] < c->staged_begin || ids[j] - c->staged_begin >= c->staged_count) in_staged = false;
  }
  HIPCHK(c, hipMemcpyAsync(c->d_ids, ids, sizeof(uint64_t) * k, hipMemcpyHostToDevice, c->stream));
  KArgs a = make_args(c);
  a.inst_begin = 0;
  a.count = k;
  a.ids = c->d_ids;
  // inputs of each listed id: the staged rows when all ids are staged, else seeded
  a.init = nullptr;
  if (in_staged) {
    a.init_base = c->staged_begin;
    if (c->cfg.alg == PSG_ALG_EPSILON) a.init_f64 = c->init_f64_host ? c->d_init_f64 : nullptr;
    else a.init = c->d_init;
  }
  a.out_inst = c->d_inst;
  a.out_rec = c->d_rec;
  a.out_rec_f64 = c->d_rec_f64;
  int rc = run_kernel(c, a, k, nullptr, false);
  if (rc) return rc;
  if (fdec || fx) {
    const uint64_t cells = k * (uint64_t)c->cfg.n;
    double* tmp = new (std::nothrow) double[2 * cells];
    if (!tmp) return fail(c, PSG_ENOMEM, "host allocation failed");
    hipError_t e = hipMemcpy(tmp, c->d_rec_f64, sizeof(double) * 2 * cells, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { delete[] tmp; return hip_fail(c, e, "hipMemcpy(rec_f64)"); }
    for (uint64_t j = 0; j < cells; ++j) {
      if (fdec) fdec[j] = tmp[2 * j];
      if (fx) fx[j] = tmp[2 * j + 1];
    }
    delete[] tmp;
  }
  if (sums) HIPCHK(c, hipMemcpy(sums, c->d_inst, sizeof(psg_instance_summary) * k, hipMemcpyDeviceToHost));
  if (procs)
    HIPCHK(c, hipMemcpy(procs, c->d_rec, sizeof(psg_process_record) * k * (uint64_t)c->cfg.n, hipMemcpyDeviceToHost));
  return PSG_OK;
}

// uint64 words of one instance's HO sets, ho[k][p][W]
static uint64_t sched_words(const psg_ctx* c) { return (uint64_t)c->cfg.rounds * (uint64_t)c->cfg.n * (uint64_t)c->W; }

// Room for the explicit schedule of `count` instances (psg_load_schedule, populations). A regrow
// drops the loaded schedule.
static int sched_buffers(psg_ctx* c, uint64_t count) {
  const uint64_t words = count * sched_words(c), crashes = count * (uint64_t)c->cfg.n;
  if (words > c->d_ho.cap || crashes > c->d_crash.cap) c->ho_loaded = false;
  HIPCHK(c, c->d_ho.grow(words));
  HIPCHK(c, c->d_crash.grow(crashes));
  return PSG_OK;
}

int psg_load_schedule(psg_ctx* c, uint64_t inst_begin, uint64_t count, const uint64_t* ho,
                      const int32_t* crash_round) {
  if (!c) return PSG_EINVAL;
  if (!ho && count) return fail(c, PSG_EINVAL, "null schedule");
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  const uint64_t n = (uint64_t)c->cfg.n, per = sched_words(c);
  if (!c->subs.empty()) {
    const uint64_t nd = c->subs.size();
    const int rc = par_subs(c, [&](size_t d) {
      uint64_t off, m;
      split(count, nd, d, off, m);
      return psg_load_schedule(c->subs[d], inst_begin + off, m, ho ? ho + off * per : nullptr,
                               crash_round ? crash_round + off * n : nullptr);
    });
    if (rc) return rc;
  } else {
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = sched_buffers(c, count)) return rc;
    if (count) {
      HIPCHK(c, hipMemcpyAsync(c->d_ho, ho, sizeof(uint64_t) * count * per, hipMemcpyHostToDevice, c->stream));
      if (crash_round)
        HIPCHK(c, hipMemcpyAsync(c->d_crash, crash_round, sizeof(int32_t) * count * n, hipMemcpyHostToDevice,
                                 c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  c->ho_loaded = true;
  c->ho_has_crash = crash_round != nullptr;
  c->pop_crash = false;
  c->ho_begin = inst_begin;
  c->ho_count = count;
  return PSG_OK;
}

int psg_clear_schedule(psg_ctx* c) {
  if (!c) return PSG_EINVAL;
  for (psg_ctx* s : c->subs) (void)psg_clear_schedule(s);
  c->ho_loaded = false;
  c->ho_has_crash = false;
  c->pop_crash = false;
  c->ho_begin = c->ho_count = 0;
  return PSG_OK;
}

int psg_materialize_schedule(psg_ctx* c, uint64_t inst_begin, uint64_t count, uint64_t* ho, int32_t* crash_round) {
  if (!c) return PSG_EINVAL;
  if (!ho && count) return fail(c, PSG_EINVAL, "null output");
  if (count == 0) return PSG_OK;
  const uint64_t n = (uint64_t)c->cfg.n, per = sched_words(c);
  if (!c->subs.empty()) {
    const uint64_t nd = c->subs.size();
    return par_subs(c, [&](size_t d) {
      uint64_t off, m;
      split(count, nd, d, off, m);
      return m ? psg_materialize_schedule(c->subs[d], inst_begin + off, m, ho + off * per,
                                          crash_round ? crash_round + off * n : nullptr)
               : PSG_OK;
    });
  }
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(count, (256ull << 20) / (per * sizeof(uint64_t))));
  DevBuf<uint64_t> d_out;
  DevBuf<int32_t> d_cr;
  hipError_t e = d_out.grow(per * chunk);
  if (e == hipSuccess) e = d_cr.grow(n * chunk);
  KArgs a = make_args(c);
  a.ho_in = nullptr;  // always the seeded generator
  a.crash_in = nullptr;
  const int G = groups_per_block(c->W);
  for (uint64_t off = 0; e == hipSuccess && off < count; off += chunk) {
    const uint64_t m = std::min<uint64_t>(chunk, count - off);
    a.inst_begin = inst_begin + off;
    a.count = m;
    const int grid = (int)std::min<uint64_t>((m + G - 1) / G, (uint64_t)c->grid_max);
    e = launch_schedule(a, c->W, grid, d_out, d_cr, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(ho + off * per, d_out, sizeof(uint64_t) * per * m, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && crash_round)
      e = hipMemcpyAsync(crash_round + off * n, d_cr, sizeof(int32_t) * n * m, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  return e == hipSuccess ? PSG_OK : hip_fail(c, e, "psg_materialize_schedule");
}

// ---------------------------------------------------------------- search populations
// Instances the population's second buffers hold (d_op is grown with d_parent).
static uint64_t pop_capacity(const psg_ctx* c) { return std::min(c->d_ho2.cap / sched_words(c), c->d_parent.cap); }

static int pop_buffers(psg_ctx* c, uint64_t count) {
  if (int rc = sched_buffers(c, count)) return rc;  // the loaded-schedule buffers (psg_load_schedule's)
  if (count > pop_capacity(c)) {
    const uint64_t cap = std::max(count, c->d_ho.cap / sched_words(c));  // at least the instances d_ho holds
    HIPCHK(c, c->d_ho2.grow(cap * sched_words(c)));
    HIPCHK(c, c->d_init2.grow(c->cap * (uint64_t)c->cfg.n));
    HIPCHK(c, c->d_parent.grow(cap));
    HIPCHK(c, c->d_op.grow(cap));
  }
  return PSG_OK;
}

static int pop_check(psg_ctx* c, const psg_population_params* p) {
  if (!p) return fail(c, PSG_EINVAL, "null population parameters");
  if (c->cfg.alg == PSG_ALG_EPSILON) return fail(c, PSG_EINVAL, "populations hold int32 inputs (not EpsilonConsensus)");
  if (c->cfg.alg != PSG_ALG_BENOR && p->value_range < 1) return fail(c, PSG_EINVAL, "value_range must be >= 1");
  if (c->cfg.alg == PSG_ALG_LATTICE && p->value_range > 31)
    return fail(c, PSG_EINVAL, "LatticeAgreement needs 1 <= value_range <= 31");
  if (p->min_size > c->cfg.n) return fail(c, PSG_EINVAL, "min_size > n");
  return PSG_OK;
}

static PopArgs pop_args(const psg_ctx* c, const psg_population_params* p, uint64_t count) {
  PopArgs a;
  std::memset(&a, 0, sizeof(a));
  a.count = count;
  a.n = c->cfg.n;
  a.R = c->cfg.rounds;
  a.W = c->W;
  a.seed = p->seed;
  a.gen = p->generation;
  a.flips = p->flips;
  a.min_size = p->min_size;
  a.self_bit = p->self_bit;
  for (int j = 0; j < 4; ++j) a.keep[j] = p->keep_p256[j];
  a.V = p->value_range;
  a.redraw = p->redraw_p256;
  a.init_kind = c->cfg.alg == PSG_ALG_BENOR     ? POP_INIT_COIN
                : c->cfg.alg == PSG_ALG_TPC     ? POP_INIT_VOTE
                : c->cfg.alg == PSG_ALG_LATTICE ? POP_INIT_SET
                                                : POP_INIT_VALUE;
  return a;
}

// Room for the crash family's genome of `count` instances, both generations (d_crash itself:
// sched_buffers).
static int pop_crash_buffers(psg_ctx* c, uint64_t count) {
  const uint64_t cells = count * (uint64_t)c->cfg.n;
  HIPCHK(c, c->d_crash2.grow(cells));
  HIPCHK(c, c->d_partial.grow(cells * (uint64_t)c->W));
  HIPCHK(c, c->d_partial2.grow(cells * (uint64_t)c->W));
  return PSG_OK;
}

static bool live_kind_known(int32_t k) { return k >= PSG_LIVE_NONE && k <= PSG_LIVE_FIXED_COORD; }

// null model: the plain omission family (psg_population_fresh / _next)
static int model_check(psg_ctx* c, const psg_population_params* p, const psg_population_model* m) {
  if (!m) return PSG_OK;
  const int n = c->cfg.n;
  if (m->family != PSG_POP_OMISSION && m->family != PSG_POP_CRASH) return fail(c, PSG_EINVAL, "unknown population family");
  if (!live_kind_known(m->live_kind)) return fail(c, PSG_EINVAL, "unknown liveness kind");
  if (m->fmax < 0 || m->fmax > n) return fail(c, PSG_EINVAL, "fmax outside 0..n");
  if (m->family == PSG_POP_CRASH && (p->min_size > 0 || m->live_kind != PSG_LIVE_NONE))
    return fail(c, PSG_EINVAL, "the crash family takes neither min_size nor a liveness kind");
  if ((uint64_t)m->move_p256 + m->add_p256 + m->drop_p256 > 256u)
    return fail(c, PSG_EINVAL, "move_p256 + add_p256 + drop_p256 > 256");
  if (m->live_rounds < 0 || m->live_rounds > PSG_POP_MAX_LIVE) return fail(c, PSG_EINVAL, "live_rounds outside 0..PSG_POP_MAX_LIVE");
  for (int j = 0; j < m->live_rounds; ++j)
    if (m->live_at[j] >= c->cfg.rounds) return fail(c, PSG_EINVAL, "live_at beyond the last round");
  if (m->phase < 1) return fail(c, PSG_EINVAL, "phase must be >= 1");
  if (m->coord < 0 || m->coord >= n) return fail(c, PSG_EINVAL, "coord outside 0..n-1");
  return PSG_OK;
}

static void pop_model_args(PopArgs& a, const psg_population_model* m) {
  if (!m) return;
  a.fmax = m->fmax;
  for (int j = 0; j < 4; ++j) a.partial_p[j] = m->partial_p256[j];
  a.t_move = m->move_p256;
  a.t_add = a.t_move + m->add_p256;
  a.t_drop = a.t_add + m->drop_p256;
  a.live_kind = m->live_kind;
  a.live_rounds = m->live_rounds;
  for (int j = 0; j < PSG_POP_MAX_LIVE; ++j) a.live_at[j] = m->live_at[j];
  a.phase = m->phase;
  a.coord = m->coord;
}

static int population_fresh(psg_ctx* c, uint64_t inst_begin, uint64_t count, const psg_population_params* p,
                            const psg_population_model* m) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "device-resident populations need a single-device context");
  if (int rc = pop_check(c, p)) return rc;
  if (int rc = model_check(c, p, m)) return rc;
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  const bool crash = m && m->family == PSG_POP_CRASH;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (int rc = pop_buffers(c, std::max<uint64_t>(count, 1))) return rc;
  if (crash)
    if (int rc = pop_crash_buffers(c, std::max<uint64_t>(count, 1))) return rc;
  PopArgs a = pop_args(c, p, count);
  pop_model_args(a, m);
  a.ho = c->d_ho;
  a.init = c->d_init;
  if (crash) {
    a.crash = c->d_crash;
    a.partial = c->d_partial;
    HIPCHK(c, launch_population_crash(a, c->stream));
  } else {
    HIPCHK(c, launch_population(a, c->stream));
    HIPCHK(c, launch_population_live(a, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ho_loaded = true;
  c->ho_has_crash = crash;
  c->pop_crash = crash;
  c->ho_begin = inst_begin;
  c->ho_count = count;
  set_staged(c, inst_begin, count, false);
  return PSG_OK;
}

static int population_next(psg_ctx* c, const uint32_t* parent, const uint8_t* op, const psg_population_params* p,
                           const psg_population_model* m) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "device-resident populations need a single-device context");
  if (int rc = pop_check(c, p)) return rc;
  if (int rc = model_check(c, p, m)) return rc;
  if (!(c->ho_loaded && is_staged(c, c->ho_begin, c->ho_count)) || pop_capacity(c) < c->ho_count)
    return fail(c, PSG_EINVAL, "no population loaded (psg_population_fresh first)");
  const bool crash = m && m->family == PSG_POP_CRASH;
  if (crash != c->pop_crash) return fail(c, PSG_EINVAL, "the loaded population is of the other fault family");
  const uint64_t count = c->ho_count;
  if (count && (!parent || !op)) return fail(c, PSG_EINVAL, "null parent / op");
  for (uint64_t i = 0; i < count; ++i) {
    if (op[i] > 2) return fail(c, PSG_EINVAL, "op must be 0 (copy), 1 (mutate) or 2 (fresh)");
    if (op[i] != 2 && parent[i] >= count) return fail(c, PSG_ERANGE, "parent index outside the population");
  }
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipMemcpyAsync(c->d_parent, parent, sizeof(uint32_t) * count, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_op, op, count, hipMemcpyHostToDevice, c->stream));
  PopArgs a = pop_args(c, p, count);
  pop_model_args(a, m);
  a.src = c->d_ho;
  a.ho = c->d_ho2;
  a.src_init = c->d_init;
  a.init = c->d_init2;
  a.parent = c->d_parent;
  a.op = c->d_op;
  if (crash) {
    a.src_crash = c->d_crash;
    a.crash = c->d_crash2;
    a.src_partial = c->d_partial;
    a.partial = c->d_partial2;
    HIPCHK(c, launch_population_crash(a, c->stream));
  } else {
    HIPCHK(c, launch_population(a, c->stream));
    HIPCHK(c, launch_population_live(a, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::swap(c->d_ho, c->d_ho2);  // the new generation is the loaded schedule / staged inputs; the
  std::swap(c->d_init, c->d_init2);  // capacities go with the buffers
  if (crash) {
    std::swap(c->d_crash, c->d_crash2);
    std::swap(c->d_partial, c->d_partial2);
  }
  return PSG_OK;
}

int psg_population_fresh(psg_ctx* c, uint64_t inst_begin, uint64_t count, const psg_population_params* p) {
  return population_fresh(c, inst_begin, count, p, nullptr);
}

int psg_population_next(psg_ctx* c, const uint32_t* parent, const uint8_t* op, const psg_population_params* p) {
  return population_next(c, parent, op, p, nullptr);
}

int psg_population_fresh_model(psg_ctx* c, uint64_t inst_begin, uint64_t count, const psg_population_params* p,
                               const psg_population_model* m) {
  if (!c) return PSG_EINVAL;
  if (!m) return fail(c, PSG_EINVAL, "null population model");
  return population_fresh(c, inst_begin, count, p, m);
}

int psg_population_next_model(psg_ctx* c, const uint32_t* parent, const uint8_t* op, const psg_population_params* p,
                              const psg_population_model* m) {
  if (!c) return PSG_EINVAL;
  if (!m) return fail(c, PSG_EINVAL, "null population model");
  return population_next(c, parent, op, p, m);
}

int psg_population_read_crash(psg_ctx* c, const uint32_t* rows, size_t k, int32_t* crash, uint64_t* partial) {
  if (!c || (!rows && k) || (!crash && k)) return PSG_EINVAL;
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "device-resident populations need a single-device context");
  if (!c->ho_loaded || !c->pop_crash) return fail(c, PSG_EINVAL, "no crash-family population loaded");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const uint64_t n = (uint64_t)c->cfg.n, W = (uint64_t)c->W;
  for (size_t j = 0; j < k; ++j) {
    if (rows[j] >= c->ho_count) return fail(c, PSG_ERANGE, "row outside the population");
    HIPCHK(c, hipMemcpy(crash + j * n, c->d_crash + (uint64_t)rows[j] * n, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (partial)
      HIPCHK(c, hipMemcpy(partial + j * n * W, c->d_partial + (uint64_t)rows[j] * n * W, sizeof(uint64_t) * n * W,
                          hipMemcpyDeviceToHost));
  }
  return PSG_OK;
}

int psg_population_live(psg_ctx* c, int32_t live_kind, int32_t phase, int32_t coord, uint8_t* live) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "device-resident populations need a single-device context");
  if (c->cfg.alg == PSG_ALG_EPSILON) return fail(c, PSG_EINVAL, "populations hold int32 inputs (not EpsilonConsensus)");
  if (!c->ho_loaded) return fail(c, PSG_EINVAL, "no explicit schedule loaded");
  if (!live_kind_known(live_kind) || live_kind == PSG_LIVE_NONE) return fail(c, PSG_EINVAL, "unknown liveness kind");
  if (phase < 1) return fail(c, PSG_EINVAL, "phase must be >= 1");
  if (coord < 0 || coord >= c->cfg.n) return fail(c, PSG_EINVAL, "coord outside 0..n-1");
  const uint64_t cells = c->ho_count * (uint64_t)c->cfg.rounds;
  if (cells == 0) return PSG_OK;
  if (!live) return fail(c, PSG_EINVAL, "null output");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, c->d_live.grow(cells));
  LiveArgs a;
  a.ho = c->d_ho;
  a.live = c->d_live;
  a.count = c->ho_count;
  a.n = c->cfg.n;
  a.R = c->cfg.rounds;
  a.W = c->W;
  a.kind = live_kind;
  a.phase = phase;
  a.coord = coord;
  HIPCHK(c, launch_live_predicate(a, c->stream));
  HIPCHK(c, hipMemcpyAsync(live, c->d_live, cells, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PSG_OK;
}

int psg_population_read(psg_ctx* c, const uint32_t* rows, size_t k, uint64_t* ho, int32_t* init) {
  if (!c || (!rows && k) || (!ho && k)) return PSG_EINVAL;
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "device-resident populations need a single-device context");
  if (!c->ho_loaded) return fail(c, PSG_EINVAL, "no population loaded");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const uint64_t n = (uint64_t)c->cfg.n, R = (uint64_t)c->cfg.rounds, W = (uint64_t)c->W;
  for (size_t j = 0; j < k; ++j) {
    if (rows[j] >= c->ho_count) return fail(c, PSG_ERANGE, "row outside the population");
    HIPCHK(c, hipMemcpy(ho + j * R * n * W, c->d_ho + (uint64_t)rows[j] * R * n * W, sizeof(uint64_t) * R * n * W,
                        hipMemcpyDeviceToHost));
    if (init && c->staged)
      HIPCHK(c, hipMemcpy(init + j * n, c->d_init + (uint64_t)rows[j] * n, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  }
  return PSG_OK;
}

int psg_population_links(psg_ctx* c, uint32_t* links) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "device-resident populations need a single-device context");
  if (!c->ho_loaded) return fail(c, PSG_EINVAL, "no explicit schedule loaded");
  if (c->ho_count == 0) return PSG_OK;
  if (!links) return fail(c, PSG_EINVAL, "null output");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, c->d_links.grow(c->ho_count));
  HIPCHK(c, launch_links(c->d_ho, c->d_links, c->ho_count, c->cfg.n, c->cfg.rounds, c->W, c->stream));
  HIPCHK(c, hipMemcpyAsync(links, c->d_links, sizeof(uint32_t) * c->ho_count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PSG_OK;
}

// ---------------------------------------------------------------- shrinking on the device
// Units of a level: what its prefix runs over (ShrinkArgs::pre).
static uint32_t shrink_units(const psg_ctx* c, int32_t level) {
  const uint32_t n = (uint32_t)c->cfg.n, R = (uint32_t)c->cfg.rounds;
  return level == PSG_SHRINK_TAIL ? 1u : level == PSG_SHRINK_ROUND ? R : level == PSG_SHRINK_CRASH ? 2u * n : R * n;
}

static ShrinkArgs shrink_args(const psg_ctx* c, int32_t level, uint32_t arg) {
  ShrinkArgs a;
  std::memset(&a, 0, sizeof(a));
  a.base = c->d_sh_base;
  a.base_crash = c->sh_has_crash ? (int32_t*)c->d_sh_crash : nullptr;
  a.base_init = c->d_sh_init;
  a.part = c->d_sh_part;
  a.pre = c->d_sh_pre;
  a.edit = c->d_sh_edit;
  a.n = c->cfg.n;
  a.R = c->cfg.rounds;
  a.W = c->W;
  a.level = level;
  a.arg = arg;
  a.units = shrink_units(c, level);
  return a;
}

// The checks every psg_shrink_* call over a level shares, then the level's prefix (d_sh_pre) and
// total over the base: computed once per (level, arg) and base.
static int shrink_level(psg_ctx* c, int32_t level, uint32_t arg, uint64_t* total) {
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "shrinking on the device needs a single-device context");
  if (c->cfg.alg == PSG_ALG_EPSILON) return fail(c, PSG_EINVAL, "shrink bases hold int32 inputs (not EpsilonConsensus)");
  if (!c->sh_base) return fail(c, PSG_EINVAL, "no shrink base (psg_shrink_begin first)");
  if (level < PSG_SHRINK_TAIL || level > PSG_SHRINK_CRASH) return fail(c, PSG_EINVAL, "unknown shrink level");
  if (level == PSG_SHRINK_CRASH && !c->sh_has_crash)
    return fail(c, PSG_EINVAL, "PSG_SHRINK_CRASH needs a base with crash rounds");
  if (level == PSG_SHRINK_CRASH) arg &= 1u;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (!(c->sh_counted && c->sh_level == level && c->sh_arg == arg)) {
    const ShrinkArgs a = shrink_args(c, level, arg);
    uint32_t t = 0;
    c->sh_counted = false;
    HIPCHK(c, launch_shrink_scan(a, c->stream));
    HIPCHK(c, hipMemcpyAsync(&t, c->d_sh_pre + a.units + 1, sizeof(t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sh_counted = true;
    c->sh_level = level;
    c->sh_arg = arg;
    c->sh_total = t;
  }
  *total = c->sh_total;
  return PSG_OK;
}

// CRASH: the base's crash-round deliveries, then the HO sets of `count` genomes (a.crash, partial).
static int shrink_crash_sets(psg_ctx* c, const ShrinkArgs& a, uint64_t count, int32_t* crash, uint64_t* partial,
                             uint64_t* ho) {
  PopArgs p;
  std::memset(&p, 0, sizeof(p));
  p.count = count;
  p.n = a.n;
  p.R = a.R;
  p.W = a.W;
  p.self_bit = a.arg & 1u;
  p.crash = crash;
  p.partial = partial;
  p.ho = ho;
  HIPCHK(c, launch_crash_ho(p, c->stream));
  return PSG_OK;
}

int psg_shrink_begin(psg_ctx* c, const uint64_t* ho, const int32_t* crash_round, const int32_t* init) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "shrinking on the device needs a single-device context");
  if (c->cfg.alg == PSG_ALG_EPSILON) return fail(c, PSG_EINVAL, "shrink bases hold int32 inputs (not EpsilonConsensus)");
  if (!ho || !init) return fail(c, PSG_EINVAL, "null schedule / initial values");
  const uint64_t n = (uint64_t)c->cfg.n, W = (uint64_t)c->W, per = sched_words(c);
  for (uint64_t q = 0; crash_round && q < n; ++q)
    if (crash_round[q] < -1 || crash_round[q] >= c->cfg.rounds) return fail(c, PSG_EINVAL, "crash round outside -1..R-1");
  std::vector<uint64_t> clean(ho, ho + per);  // bits >= n cleared
  if (c->cfg.n % 64)
    for (uint64_t r = W - 1; r < per; r += W) clean[r] &= (1ull << (c->cfg.n % 64)) - 1ull;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  c->sh_base = c->sh_counted = false;
  HIPCHK(c, c->d_sh_base.grow(per));
  HIPCHK(c, c->d_sh_part.grow(n * W));
  HIPCHK(c, c->d_sh_crash.grow(n));
  HIPCHK(c, c->d_sh_init.grow(n));
  HIPCHK(c, c->d_sh_pre.grow(std::max<uint64_t>((uint64_t)c->cfg.rounds * n, 2 * n) + 2));
  HIPCHK(c, c->d_sh_edit.grow(1));
  HIPCHK(c, hipMemcpyAsync(c->d_sh_base, clean.data(), sizeof(uint64_t) * per, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_sh_init, init, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
  if (crash_round)
    HIPCHK(c, hipMemcpyAsync(c->d_sh_crash, crash_round, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->sh_base = true;
  c->sh_has_crash = crash_round != nullptr;
  return PSG_OK;
}

int psg_shrink_count(psg_ctx* c, int32_t level, uint32_t arg, uint64_t* total) {
  if (!c || !total) return PSG_EINVAL;
  return shrink_level(c, level, arg, total);
}

int psg_shrink_load(psg_ctx* c, int32_t level, uint32_t arg, uint64_t first, uint64_t count, uint64_t inst_begin) {
  if (!c) return PSG_EINVAL;
  uint64_t total = 0;
  if (int rc = shrink_level(c, level, arg, &total)) return rc;
  if (count > c->cap) return fail(c, PSG_ERANGE, "inst_count exceeds batch_capacity");
  if (first > total || count > total - first) return fail(c, PSG_ERANGE, "candidates beyond the level's total");
  const bool crash = level == PSG_SHRINK_CRASH;
  if (int rc = sched_buffers(c, std::max<uint64_t>(count, 1))) return rc;
  if (crash) HIPCHK(c, c->d_partial.grow(std::max<uint64_t>(count, 1) * (uint64_t)c->cfg.n * (uint64_t)c->W));
  HIPCHK(c, c->d_sh_edit.grow(std::max<uint64_t>(count, 1)));
  ShrinkArgs a = shrink_args(c, level, crash ? (arg & 1u) : arg);
  a.first = first;
  a.count = count;
  a.ho = c->d_ho;
  a.init = c->d_init;
  a.crash = c->sh_has_crash ? (int32_t*)c->d_crash : nullptr;
  a.partial = crash ? (uint64_t*)c->d_partial : nullptr;
  HIPCHK(c, launch_shrink_edits(a, c->stream));
  if (crash) {
    HIPCHK(c, launch_shrink_part(a, c->stream));
    HIPCHK(c, launch_shrink_rows(a, c->stream));
    if (int rc = shrink_crash_sets(c, a, count, c->d_crash, c->d_partial, c->d_ho)) return rc;
  } else {
    HIPCHK(c, launch_shrink_fill(a, c->stream));
    HIPCHK(c, launch_shrink_rows(a, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ho_loaded = true;
  c->ho_has_crash = c->sh_has_crash;
  c->pop_crash = false;
  c->ho_begin = inst_begin;
  c->ho_count = count;
  set_staged(c, inst_begin, count, true);
  return PSG_OK;
}

int psg_shrink_adopt(psg_ctx* c, int32_t level, uint32_t arg, uint64_t j) {
  if (!c) return PSG_EINVAL;
  uint64_t total = 0;
  if (int rc = shrink_level(c, level, arg, &total)) return rc;
  if (j >= total) return fail(c, PSG_ERANGE, "candidate beyond the level's total");
  const bool crash = level == PSG_SHRINK_CRASH;
  ShrinkArgs a = shrink_args(c, level, crash ? (arg & 1u) : arg);
  a.first = j;
  a.count = 1;
  a.ho = c->d_sh_base;  // the edit in place: every word depends on its own old value only
  c->sh_counted = false;
  HIPCHK(c, launch_shrink_edits(a, c->stream));
  if (crash) {
    a.crash = c->d_sh_crash;
    HIPCHK(c, launch_shrink_part(a, c->stream));  // from the old base, before its crash rounds move
    HIPCHK(c, launch_shrink_rows(a, c->stream));
    if (int rc = shrink_crash_sets(c, a, 1, c->d_sh_crash, c->d_sh_part, c->d_sh_base)) return rc;
  } else {
    HIPCHK(c, launch_shrink_fill(a, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PSG_OK;
}

int psg_shrink_read(psg_ctx* c, uint64_t* ho, int32_t* crash_round) {
  if (!c) return PSG_EINVAL;
  if (!c->subs.empty()) return fail(c, PSG_EINVAL, "shrinking on the device needs a single-device context");
  if (!c->sh_base) return fail(c, PSG_EINVAL, "no shrink base (psg_shrink_begin first)");
  if (!ho) return fail(c, PSG_EINVAL, "null output");
  const uint64_t n = (uint64_t)c->cfg.n;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipMemcpyAsync(ho, c->d_sh_base, sizeof(uint64_t) * sched_words(c), hipMemcpyDeviceToHost, c->stream));
  if (crash_round && c->sh_has_crash)
    HIPCHK(c, hipMemcpyAsync(crash_round, c->d_sh_crash, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (crash_round && !c->sh_has_crash) std::fill(crash_round, crash_round + n, -1);
  return PSG_OK;
}

const char* psg_last_error(const psg_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

void psg_destroy(psg_ctx* c) {
  if (!c) return;
  if (!c->subs.empty() || c->cfg.n_devices > 0) {  // multi-device: the per-device contexts own everything
    for (psg_ctx* s : c->subs) psg_destroy(s);
    delete c;
    return;
  }
  (void)hipSetDevice(c->cfg.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  static_cast<psg_buffers&>(*c) = psg_buffers();  // frees every device buffer, before the stream goes
  if (c->module) (void)hipModuleUnload(c->module);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

}  // extern "C"
