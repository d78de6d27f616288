// psg_otr.hip — OTR (one-third rule) and OTR2 on gfx950.
//
// Reference: example/Otr.scala:13-128 (OtrProcess, OTR.spec); example/Otr2.scala:9-104
// (Otr2Process: the same round with decision: Option[Int]; OTR2.spec has no
// keepInit conjunct, Invariant0's first disjunct is "everyone decided" and
// Invariant2 is "all decisions equal").
// One wave64 per instance, lane = process (n <= 64); W waves per instance for
// n > 64. Per round: HO(p) from Philox, mailbox M(p) = HO(p) & alive,
// mmor (Otr.scala:44-49) as a loop over the distinct values v of the alive
// senders: E_v = ballot(x == v), count(p, v) = popc(M(p) & E_v), keep the max
// count, ties to the smaller value. The Spec (Otr.scala:95-120) is evaluated
// after every round with ballots over the same distinct-value structure.
#include "psg_device.hpp"
#include "psg_kernels.hpp"

namespace psg {

template <int W>
struct OtrLds {
  int32_t xs[W > 1 ? 64 * W : 1];
  int32_t ds[W > 1 ? 64 * W : 1];
};

// Per-lane thresholds of a check point in the settled state (otr_check_settled, W == 1), where a
// lane records iff the vote count cnt <= its threshold (Checks::record_le): lane 1 (Invariant0)
// 2n/3, for OTR2 never (its Invariant0 holds by term); lane 2 (Invariant1) n - 1; lane
// PSG_MAX_CHECKS (Termination) always; every other lane never (-1 < 0 <= cnt). A function of n
// and the lane alone: formed once per kernel.
template <bool V2>
PSG_DEV int32_t otr_check_thresholds(int n, int lane) {
  int32_t t = -1;
  if (!V2 && lane == 1) t = (2 * n) / 3;
  if (lane == 2) t = n - 1;
  if (lane == PSG_MAX_CHECKS) t = INT32_MAX;
  return t;
}

// Spec check at check point c (spec r = c). Slots: 0 Safety (some invariant
// holds), 1..3 invariants, 4 Agreement, 5 Validity, 6 Integrity, 7 Irrevocability.
// Every formula is evaluated from scratch at every check point. The universally
// quantified parts are per-process witnesses:
//   !(i.x == init(j.x) for some j)                  keepInit   (X0-set probe)
//   i.decided && i.decision not initial             Validity
//   i.decided && i.decision != d0                   Agreement  (d0 = a decided value)
//   old(i.decided) && !(i.decided && old(i.decision) == i.decision)  Irrevocability
// Fast path: one VALU word per process holds a bit per witness, where the two X0
// probes only look at the value's two home slots ("maybe not initial"); one ballot
// of "some bit set" settles all four when no process is even a possible witness
// (the common case). Otherwise each is resolved exactly with its own ballot and
// the full probe. (OR-reducing such a word with a DPP chain was measured 28 %
// slower, profiles/s2_ab/ab5.log: the chain's latency; a compare + ballot has none.)
// V.exists(v => |{i : i.x == v}| > 2n/3 && all decisions == v): with decisions only
// v = d0 can qualify; without, v must be a strict majority (Boyer-Moore candidate).
// otr_check (below) is a check point: otr_check_settled, else otr_check_general.

// The check outside the settled state (arguments as otr_check's; irr01 is the per-process
// Irrevocability witness bit).
template <int W, bool V2>
PSG_DEV void otr_check_general(Grp<W>& g, OtrLds<W>& L, const X0Set<W>& X0, Checks& ck, int c, bool has_old, int n,
                               const Mask<W>& full, int32_t x, uint32_t dec01, int32_t decision, uint32_t old01,
                               int32_t old_decision, uint32_t valid01, uint32_t od, uint32_t ox, uint32_t irr01) {
  const int sthr = (2 * n) / 3;  // 2*n/3 in the Spec (Otr.scala:101)
  // dec01 and the witness word are 0 on lanes past n: ballots without the valid-lane mask
  const Mask<W> D = g.ballot_any(dec01 != 0u);
  const bool anyD = many(D);
  const int32_t d0 = anyD ? g.bcast(decision, L.ds, mfirst(D)) : 0;
  uint32_t wit = od | ne01(decision, d0);
  if constexpr (!V2) wit = (wit & dec01) | ox;  // keepInit (OTR only)
  else wit &= dec01;
  wit |= irr01;
  const Mask<W> Wm = g.ballot_any((wit & valid01) != 0u);
  const bool term = meq(D, full);
  const bool wany = many(Wm);
  // the vote count's value: d0 once someone decided; before that OTR reads the count only as
  // cnt == n (Invariant1; Invariant0 is keepInit alone with no decision), which holds iff every
  // x equals process 0's — the majority candidate is needed only for OTR2's e0 (and W > 1)
  auto vote_count = [&]() -> int {
    const int32_t ref = anyD ? d0 : ((!V2 && W == 1) ? readlane32(x, 0) : majority_candidate<W>(g, x));
    return mpopc(g.ballot((valid01 & eq01(x, ref)) != 0u));
  };
  // W == 1 counts before the two arms, which share it; W > 1 keeps the one general form below,
  // with the count after the witness ballots (the no-witness arm costs it an occupancy step)
  int cnt = 0;
  if constexpr (W == 1) cnt = vote_count();
  if (W == 1 && !wany) {
    // No witness (the usual state before everyone has decided): keepInit, Validity, Agreement
    // ("same") and Irrevocability hold, and the formulas of the exact arm below reduce to
    // functions of anyD, term and cnt. OTR: Invariant0 = !anyD || cnt > 2n/3, Invariant1 =
    // (cnt == n), Invariant2 = term, Safety their disjunction (cnt <= 2n/3 implies cnt < n);
    // OTR2: Invariant0 = term || cnt > 2n/3, Invariant1 = (cnt == n), Invariant2 and Safety hold;
    // Integrity holds in both. Every one is evaluated here, as 0/1 integers behind opaque copies:
    // a uniform bool the compiler recognises is a 64-bit lane mask (opaque_uniform).
    const uint32_t les = opaque_uniform((uint32_t)(cnt - sthr - 1));  // sign bit: cnt <= 2n/3
    const uint32_t ne = opaque_uniform((uint32_t)(cnt - n)) >> 31;    // cnt != n (cnt <= n always)
    uint32_t fb;
    if constexpr (V2) {
      const uint32_t t = opaque_uniform(term ? 1u : 0u);
      fb = (t << PSG_MAX_CHECKS) | (((t ^ 1u) & (les >> 31)) << 1) | (ne << 2);
    } else {
      // Termination's bit when term holds, else Invariant2's fail bit (slot 3)
      const uint32_t tk = opaque_uniform(term ? (1u << PSG_MAX_CHECKS) : (1u << 3));
      // anyD && cnt <= 2n/3: the AND of two sign bits (-|D| < 0 iff someone decided)
      const uint32_t f1 = (les & opaque_uniform((uint32_t)-mpopc(D))) >> 31;
      fb = tk | (f1 & (tk >> 3)) | (f1 << 1) | (ne << 2);
    }
    ck.record(fb, false, c, g.lane);
    return;
  }
  bool keep = true, validity = true, same = true, irrev = true;
  if (wany) {  // some process is a possible witness: exact resolution, one ballot per formula
    if constexpr (!V2) keep = X0.all_in(g, full, x);
    validity = X0.all_in(g, D, decision);
    same = !many(mand(D, g.ballot(decision != d0)));
    if (has_old) irrev = !many(mandn(g.ballot(old01 != 0u), mand(D, g.ballot(old_decision == decision))));
  }
  if constexpr (W > 1) cnt = vote_count();
  const bool condv = !anyD || same;
  const bool e0 = condv && cnt > sthr;
  const bool e1 = condv && cnt == n;
  const bool d0in = same && validity;  // all decisions equal d0 and are initial values
  // OTR: Otr.scala:99-110; OTR2: Otr2.scala:75-87
  const bool inv0 = V2 ? (term || e0) : ((!anyD || e0) && keep);
  const bool inv1 = V2 ? e1 : (e1 && keep);
  const bool inv2 = V2 ? same : (term && d0in);
  const bool integrity = !anyD || d0in;
  const uint32_t fb = fbit(inv0 || inv1 || inv2, 0) | fbit(inv0, 1) | fbit(inv1, 2) | fbit(inv2, 3) |
                      fbit(same, 4) | fbit(validity, 5) | fbit(integrity, 6) | fbit(irrev, 7);
  ck.record(fb, term, c, g.lane);
}

// The check in the settled state: every process decided, every decision equal to process 0's,
// no witness: one ballot of a per-process word, with process 0's decision as d0 (when all
// decided, process 0 is the first decider). Then keepInit, Validity, Agreement and
// Irrevocability hold, so Invariant2 (OTR: term && all decisions equal and initial; OTR2: all
// decisions equal), Safety and Integrity hold; Invariant0 reduces to e0 (OTR2: term),
// Invariant1 to e1, with the vote count taken at v = d0: the same values as the general path,
// in a few instructions (most check points of a run are in this state). The results depend on
// the count alone and are recorded per lane against ckthr (no scalar fail word): slot 1 fails
// iff cnt <= 2n/3 (OTR), slot 2 iff cnt <= n - 1 (cnt <= n always), Termination holds, no
// other slot fails. Returns false, with nothing recorded, when the state is not settled.
template <int W, bool V2>
PSG_DEV bool otr_check_settled(Grp<W>& g, OtrLds<W>& L, Checks& ck, int c, int n, int32_t x, uint32_t dec01,
                               int32_t decision, uint32_t valid01, uint32_t od, uint32_t ox, uint32_t irr01,
                               int32_t ckthr) {
  if constexpr (W > 1) {
    L.ds[g.pid] = decision;
    __syncthreads();
  }
  const int32_t p0 = g.bcast(decision, L.ds, 0);
  uint32_t u = (1u - dec01) | od | ne01(decision, p0) | irr01;
  if constexpr (!V2) u |= ox;  // keepInit (OTR only)
  if (g.any((u & valid01) != 0u)) return false;
  const int cnt = mpopc(g.ballot(x == p0));  // (a compare and the valid-lane mask)
  if constexpr (W == 1) {
    ck.record_le(cnt, ckthr, c);
  } else {  // the same results as a scalar fail word (W > 1: one VGPR fewer, it sits at an occupancy step)
    const int sthr = (2 * n) / 3;
    ck.record((V2 ? 0u : fbit(cnt > sthr, 1)) | fbit(cnt == n, 2), true, c, g.lane);
  }
  return true;
}

// Group size of the frozen tail in otr_body: 2, 4, 8 and 4 with a 2 for the remainder were
// measured, 8 is the fastest.
constexpr int kFrozenGroup = 8;

// U check points of the frozen tail, c0 .. c0 + U - 1 (W == 1), as one straight-line group:
// otr_check_settled with the frozen tail's irr01 = 0 at each of them — its own read of process
// 0's decision, its own witness word and ballot, its own vote count and its own record — with
// one branch for the group on the OR of the U witness ballots. The U chains do not depend on
// one another, so they interleave. Returns false, with nothing recorded, when some check point
// of the group is not settled (the frozen state is the same at all of them: then none is).
// Each check point reads process 0's decision from an opaque copy of the decision that takes the
// check-point number as an input: otherwise the U chains are one common subexpression. The
// copies are made one from the other and the last is handed back as the decision (the same
// value), so each copy's source dies where the copy is made and the copy is no instruction.
template <int U, bool V2>
PSG_DEV bool otr_check_frozen_group(Grp<1>& g, Checks& ck, int c0, int32_t x, uint32_t dec01, int32_t& decision,
                                    uint32_t valid01, uint32_t od, uint32_t ox, int32_t ckthr) {
  int32_t p0[U];
  int32_t d = decision;
#pragma unroll
  for (int j = 0; j < U; ++j) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(d) : "s"(c0 + j));
#endif
    p0[j] = readlane32(d, 0);
  }
  decision = d;
  uint32_t u0 = (1u - dec01) | od;
  if constexpr (!V2) u0 |= ox;  // keepInit (OTR only)
  uint64_t wit = 0;
#pragma unroll
  for (int j = 0; j < U; ++j) wit |= g.ballot(((u0 | ne01(d, p0[j])) & valid01) != 0u).w[0];
  if (wit != 0) return false;
#pragma unroll
  for (int j = 0; j < U; ++j) ck.record_le(mpopc(g.ballot(x == p0[j])), ckthr, c0 + j);
  return true;
}

template <int W, bool V2, bool FROZEN = false>
// od / ox: "decision / x maybe not initial" (X0Set::maybe_out01_2 of the current values), probed
// by the caller when the values change (round 0 and executed updates) instead of at every check
// point: the memoized probe of the fused lowering; every formula is still evaluated.
// FROZEN: a check point of the frozen tail, where the pre-round state is the current one, so the
// Irrevocability witness old.decided && !(decided && old.decision == decision) is 0 by algebra.
// ckthr: the settled state's per-lane record thresholds (otr_check_thresholds), formed once per kernel.
PSG_DEV void otr_check(Grp<W>& g, OtrLds<W>& L, const X0Set<W>& X0, Checks& ck, int c, bool has_old, int n,
                       const Mask<W>& full, int32_t x, uint32_t dec01, int32_t decision, uint32_t old01,
                       int32_t old_decision, uint32_t valid01, uint32_t od, uint32_t ox, int32_t ckthr) {
  const uint32_t irr01 = (has_old && !FROZEN) ? old01 & (1u - (dec01 & eq01(old_decision, decision))) : 0u;
  if (!otr_check_settled<W, V2>(g, L, ck, c, n, x, dec01, decision, valid01, od, ox, irr01, ckthr))
    otr_check_general<W, V2>(g, L, X0, ck, c, has_old, n, full, x, dec01, decision, old01, old_decision, valid01, od,
                             ox, irr01);
}

// Check point 0 for W == 1, from the state after init(io) (Otr.scala:15-26): no process has
// decided and every x is an initial value. Each line is otr_check_general's with dec01 = 0 on
// every lane and has_old = false: D is empty, so anyD = false and term = (D == full) is false
// (n >= 1); the witness word is ox for OTR and 0 for OTR2, and where ox is set (a value outside
// its two home slots of the hash table) the exact arm finds keep = all_in(x) true, as every x is
// in the set built from these very values; validity and same range over the empty D and irrev
// needs has_old, so all four hold, and condv = true. Hence
//   OTR:  Invariant0 = (!anyD || e0) && keep holds, Invariant1 = e1 = (cnt == n), Invariant2 =
//         term && d0in is false, Safety holds by Invariant0;
//   OTR2: Invariant0 = term || e0 = (cnt > 2n/3), Invariant1 = (cnt == n), Invariant2 = same
//         holds, Safety holds by Invariant2;
//   Agreement, Validity, Integrity (!anyD) and Irrevocability hold, Termination does not.
// cnt is otr_check_general's vote_count with anyD = false: against process 0's x for OTR,
// against the majority candidate for OTR2. The fail word is a 32-bit scalar integer formed from
// sign bits behind opaque copies, as in otr_check_general's no-witness arm.
template <bool V2>
PSG_DEV void otr_check_initial(Grp<1>& g, Checks& ck, int n, int32_t x, uint32_t valid01) {
  const int32_t ref = V2 ? majority_candidate<1>(g, x) : readlane32(x, 0);
  const int cnt = mpopc(g.ballot((valid01 & eq01(x, ref)) != 0u));
  const uint32_t ne = opaque_uniform((uint32_t)(cnt - n)) >> 31;  // cnt != n (cnt <= n always)
  uint32_t fb = ne << 2;
  if constexpr (V2) fb |= (opaque_uniform((uint32_t)(cnt - (2 * n) / 3 - 1)) >> 31) << 1;  // cnt <= 2n/3
  else fb |= 1u << 3;
  ck.record(fb, false, 0, g.lane);
}

// mmor (max multiplicity, ties to the smaller value: OtrExample.scala:67-75) of one W == 1 round
// in bitmap mode (X0.bmode): every initial value lies in [lo, lo + 64), and every later x is a
// value some process received, i.e. the x of a sender, so by induction over the rounds every
// alive process's x stays in that window. best_c / best_v: the winning count and value of this
// lane's mailbox M (meaningful on the updating lanes, whose mailbox is not empty).
// - A value v is named by its complement slot c = 63 - (v - lo) in 0..63, and the running best is
//   one 32-bit key, count << 6 | c (count <= 64): a larger key has a larger count, or the same
//   count and a smaller value, so folding a value is one unsigned max. The one uniform c serves
//   the compare that finds the value's holders E and the key's low bits; count and value are
//   decoded once after the loop. (Unsigned arithmetic throughout: lo + 63 may pass INT32_MAX.)
//   Lanes past n hold x = 0 and may match a c; E is only ever intersected with M, inside act.
// - Round 0: every process is alive and holds its initial value, so the distinct values are
//   exactly the bits of X0.bm. They are walked on the scalar pipe (find first bit, clear it): no
//   lane is read and no ballot feeds the walk, so the trips depend on one another only through
//   the max. One value a trip: two a trip (the last bit folded twice when one is left) measured
//   0.9 % slower on the headline.
//   With more than 8 distinct values (V = 64: ~40 of 64) they are folded by decreasing holder
//   classes, as value bitmaps: a value held by h alive senders counts at most h in any mailbox,
//   so h >= 3 goes first, then h = 2, then h = 1, and a class is skipped when every updating
//   lane's best count already exceeds its h (it can neither win nor tie). Holders are counted in
//   LDS (cnt: 64 words, the X0 table, free in bitmap mode), lane b reads the count of value lo + b
//   behind a wave-scope fence.
// - Rounds k > 0 have few values and no bitmap of them: the walk over the alive lanes' values
//   (read the first remaining lane's c, drop its holders), with the same key.
PSG_DEV void otr_mmor_bitmap(Grp<1>& g, const X0Set<1>& X0, int32_t* cnt, int k, int32_t x, const Mask<1>& M,
                             const Mask<1>& act, uint32_t upd, uint32_t halted01, int32_t& best_c, int32_t& best_v) {
  const uint32_t cs = 63u - ((uint32_t)x - (uint32_t)X0.lo);
  const uint64_t m = M.w[0];
  auto key = [&](uint32_t c) -> uint32_t {
    const uint64_t E = __builtin_amdgcn_ballot_w64(cs == c);
    return ((uint32_t)__builtin_popcountll(m & E) << 6) | c;
  };
  auto umax = [](uint32_t p, uint32_t q) -> uint32_t { return p > q ? p : q; };
  uint32_t best = 0;
  if (k == 0) {
    uint64_t B = X0.bm, passB = 0, passS = 0;
    int stage = 2;  // 2: a single pass over every value
    if (__builtin_popcountll(B) > 8) {
      cnt[g.lane] = 0;
      if (!halted01) atomicAdd(&cnt[63u - cs], 1);
      lds_sync<1>();  // lane b reads what the other lanes added (without it its own 0 is forwarded)
      const int32_t h = cnt[g.lane];
      B = __builtin_amdgcn_ballot_w64(h >= 3);
      passB = __builtin_amdgcn_ballot_w64(h == 2);
      passS = X0.bm & ~(B | passB);
      stage = 0;
    }
    while (true) {
      while (B != 0) {
        const uint32_t b = (uint32_t)__builtin_ctzll(B);
        B &= ~(1ull << b);  // (shift and and-not: B & (B - 1) is three scalar instructions)
        // c behind an opaque copy: folded into the key's arithmetic it costs a VALU a value
        best = umax(key(opaque_uniform(63u ^ b)), best);
      }
      if (stage == 2) break;
      const uint32_t beat = stage == 0 ? 3u : 2u;  // the next class's values count < beat
      if (!g.any(upd != 0u && best < (beat << 6))) break;
      B = stage == 0 ? passB : passS;
      ++stage;
    }
  } else {
    uint64_t rem = act.w[0];
    while (rem != 0) {
      const uint32_t c = (uint32_t)readlane32((int32_t)cs, __builtin_ctzll(rem));
      const uint64_t E = __builtin_amdgcn_ballot_w64(cs == c);
      rem &= ~E;
      best = umax(((uint32_t)__builtin_popcountll(m & E) << 6) | c, best);
    }
  }
  best_c = (int32_t)(best >> 6);
  best_v = (int32_t)((uint32_t)X0.lo + 63u - (best & 63u));
}

// Kernel body; SH: the Spec hook (NoHook in psg_device.hpp). TR = false: the launch has no
// Spec-program trace (a.trace == nullptr), known at compile time.
// W == 1 takes its own forms of the per-instance setup and finish: X0Set::build_window,
// otr_check_initial, and finish_instance_w1 with the WaveTally. W > 1 keeps the general forms.
// The seeded, trace-free W == 1 forms with the built-in checker (kFront) read their good rounds
// from a GoodFront (psg_device.hpp): rounds 0..3 of eight batch rows from one Philox pass, later
// rounds 32 a pass. The traced and fused forms keep Sched::prep_good.
// The kFront forms also run mmor through otr_mmor_bitmap when the instance's values fit a 64-value
// window (X0.bmode); hash mode and the other forms keep the loop in the body.
// PLAIN (kFront forms only): the launch's schedule has no crashes and no ho_min (launch_w), the
// default HOSchedule. The HO sets come from Sched::ho_plain — the same words of the same Philox
// calls as Sched::ho, drawn straight-line — and the crash draw, the crash sets and their terms
// are not compiled.
template <int W, bool V2, bool XHO, class SH = NoHook, bool TR = true, bool PLAIN = false>
PSG_DEV void otr_body(const KArgs& a) {
  const bool tracing_on = SH::kFused || (TR && a.trace != nullptr);
  constexpr bool kFront = W == 1 && !XHO && !SH::kFused && !TR;
  static_assert(!PLAIN || kFront, "the plain-schedule form is a seeded, trace-free W == 1 form");
  __shared__ BlockCounters bc;
  __shared__ uint64_t xb[Grp<W>::kXb];
  __shared__ int32_t crl[W > 1 ? 64 * W : 1];
  __shared__ int64_t red[2 * W];
  __shared__ OtrLds<W> L;
  __shared__ int32_t x0tab[Geometry<W>::kGroups][X0Set<W>::kSlots];
  counters_init(&bc);
  __syncthreads();
  Grp<W> g;
  grp_setup(g, a, xb, red);
  const int grp = W == 1 ? (int)(threadIdx.x >> 6) : 0;
  const int n = a.n;
  const int thr = a.variant == 1 ? n / 2 : (2 * n) / 3;  // Otr.scala:64, 67 (variant 1: mutation)
  const Mask<W> full = mfull<W>(n);
  const uint32_t valid01 = g.valid ? 1u : 0u;
  const int32_t ckthr = W == 1 ? otr_check_thresholds<V2>(n, g.lane) : 0;  // (W > 1: unused)
  // PLAIN: the lane's self bit as a word of the HO set, 0 when the schedule has none
  const uint64_t selfw = PLAIN && a.self_bit ? 1ull << (g.pid & 63) : 0ull;
  // W == 1: the launch-constant predicates of the setup and the finish as bits of one scalar
  // word (LaunchBits, psg_device.hpp)
  uint32_t lb = W == 1 ? launch_bits(a) : 0u;
  auto has_ids = [&]() -> bool {
    if constexpr (W == 1) return launch_bit01(lb, LaunchBits::kIds) != 0u;
    else return a.ids != nullptr;
  };
  auto has_init = [&]() -> bool {
    if constexpr (W == 1) return launch_bit01(lb, LaunchBits::kInit) != 0u;
    else return a.init != nullptr;
  };

  // profiling builds only: t1 active round, t2 frozen round; the setup is t4 queue take, t5 begin +
  // initial value, t6 X0 set, t0 check point 0; the finish t7 digest and its sum, t3 the rest.
  // Inside an active round: t8 the settled test and the good-round lookup, t9 HO draw + mailbox,
  // t10 mmor, t11 update + countdown, and t1 is left with the round's check point.
  PhaseTimers pt;
  pt.start();
  InstanceQueue<W, 0, W == 1 ? PSG_QUEUE_CHUNK_LANE : 0> Q;  // dynamic instance distribution (psg_device.hpp)
  StepTally tally;     // per-lane process-round steps, reduced once per wave
  WaveTally wtally;    // W == 1: the other counters' sums, flushed once per wave
  GoodFront gf;        // kFront: the good rounds of the current eight batch rows
  // Host-supplied initial values are loaded one instance ahead: the next row's load is
  // issued when an instance starts and consumed when the next one does, so its latency
  // overlaps the current instance's rounds instead of stalling its setup.
  auto load_x0 = [&](uint64_t ii) -> int32_t {
    if (ii == Q.kDone || !has_init() || !g.valid) return 0;
    return a.init[init_row(a, ii, instance_id(a, ii, has_ids()), has_ids()) * (uint64_t)n + g.pid];
  };
  uint64_t inext = Q.take(a);
  int32_t x0next = load_x0(inext);
  while (inext != Q.kDone) {
    const uint64_t i = inext;
    const int32_t x0host = x0next;
    if constexpr (W == 1) lb = launch_bits_carry(lb);
    inext = Q.take(a);
    x0next = load_x0(inext);
    pt.mark(4);
    Inst<W, XHO> in;
    if constexpr (kFront) {
      if constexpr (PLAIN) in.begin_plain(a, i, has_ids());
      else in.begin_front(g, a, i, crl, has_ids());
      if (launch_bit01(lb, LaunchBits::kGood)) gf.start(in.sc, a, i, g.lane, has_ids());
    } else {
      in.begin(g, a, i, crl);
    }
    Sched<W, XHO>& sc = in.sc;
    int32_t x0 = 0;
    if (g.valid) x0 = has_init() ? x0host : sc.init_value(g.pid, PSG_ALG_OTR);
    pt.mark(5);
    X0Set<W> X0;
    if constexpr (W == 1)
      X0.build_window(g, x0tab[grp], x0, launch_bit01(lb, LaunchBits::kWideV) != 0u);
    else X0.build(g, x0tab[grp], x0);
    pt.mark(6);
    // OtrProcess state after init(io) (Otr.scala:15-26); flags are 0/1 lane words
    int32_t x = x0, decision = -1, after = a.param;
    uint32_t od, ox;  // memoized X0 probes of decision / x (otr_check)
    X0.maybe_out01_2(decision, x, od, ox);
    uint32_t dec01 = 0, halted01 = 1u - valid01;
    int32_t dec_val = 0, dec_round = -1, halt_round = -1;
    Checks ck;
    ck.reset();
    typename SH::template State<W> sh(g, grp, n);  // fused Spec evaluation state (NoHook: empty)
    if constexpr (!SH::kFused) {
      if constexpr (W == 1) otr_check_initial<V2>(g, ck, n, x, valid01);
      else otr_check<W, V2>(g, L, X0, ck, 0, false, n, full, x, dec01, decision, 0u, -1, valid01, od, ox, ckthr);
    }
    // OTR2's decision is an Option (PSG_NONE32 when empty)
    auto trace = [&](int c, int32_t hs, bool frozen = false) {
      emit_state<W, SH>(sh, g, a, i, c, x, (int32_t)dec01, V2 && !dec01 ? PSG_NONE32 : decision, 0, 0, 0, 0, 0, hs,
                        frozen);
    };
    if (tracing_on) trace(0, n);
    pt.mark(0);

    // does a trace or the fused Spec read |mailbox| (psg.h PSG_FIELD_HOSIZE)?
    const bool hs_needed = SH::kFused ? ((SH::kFields >> PSG_FIELD_HOSIZE) & 1u) != 0u
                                      : (TR && a.trace != nullptr && ((a.trace_fields >> PSG_FIELD_HOSIZE) & 1u));
    int32_t live_rounds = 0;  // rounds in which some process took a step
    bool good_read = false;   // (event build only)
    int kf = a.R;             // first round in which every process had halted (the state is final)
    for (int k = 0; k < a.R; ++k) {
      const uint32_t old01 = dec01;
      const int32_t old_decision = decision;
      const Mask<W> act = g.ballot_any(halted01 == 0u);  // lanes past n are halted
      int32_t hs = n;  // |mailbox| of this round (Spec field HOSIZE)
      if (!many(act)) {  // every process halted: the frozen tail below (25.3 -> 24.8 ms)
        kf = k;
        break;
      }
      {
        live_rounds = k + 1;
        // Settled round: every live process has decided d and holds x = d. Then every mailbox
        // holds only d, so mmor is d (OtrExample.scala:67-75) and a mailbox above 2n/3 re-decides
        // the d it holds (Otr.scala:63-73): no process's x, decision or decided changes whatever
        // its HO set is, and only `after` counts down (Otr.scala:75-80). The round's HO sets are
        // then not drawn and mmor not run (the schedule is a pure function of (instance, round,
        // pid), so no other draw moves); the check point after it is evaluated as every other.
        // Not taken when a trace or the fused Spec reads |mailbox|.
        bool settled = false;
        if constexpr (W == 1) {
          if (!hs_needed) {
            const int32_t d0 = readlane32(decision, mfirst(act));
            settled = !g.any_raw(halted01 == 0u && !(dec01 != 0u && decision == d0 && x == d0));
          }
        }
        if (!settled) {
        Mask<W> goodS;
        bool good;
        if constexpr (kFront) good = gf.good_round(sc, i, k, g.lane, a.R, goodS);
        else good = sc.good_round(k, g.lane, a.R, goodS);
        pt.add(4, good ? 1u : 0u);  // event build: good rounds executed unsettled
        pt.add(5, good && !good_read ? 1u : 0u);  // ... the first of them in an instance
        if (PSG_PHASE_TIMERS == 2) good_read = good_read || good;
        pt.mark(8);
        // mailbox: broadcast(x) from every alive sender in HO(p)
        Mask<W> M;
        if constexpr (PLAIN) {
          M = mand(sc.ho_plain((uint32_t)k, (uint32_t)g.pid, good, goodS, selfw), act);
        } else {
          Mask<W> CB = mzero<W>(), CN = mzero<W>();
          if (sc.crash_on) in.cs.sets(g, k, CB, CN);
          M = mand(sc.ho(k, g.pid, good, goodS, CB, CN), act);
        }
        const int32_t msize = mpopc(M);
        pt.mark(9);
        if (tracing_on) hs = halted01 ? n : msize;
        const uint32_t upd = (1u - halted01) & gt01(msize, thr);
        if (g.any(upd != 0u)) {
          int32_t best_c = 0, best_v = 0;
          bool folded = false;
          if constexpr (kFront) {
            if (X0.bmode) {
              otr_mmor_bitmap(g, X0, x0tab[grp], k, x, M, act, upd, halted01, best_c, best_v);
              folded = true;
            }
          }
          if (!folded) {
          // mmor: max multiplicity, ties -> smaller value (OtrExample.scala:67-75).
          // The running best is one 64-bit key (count << 32 | v ^ 0x7FFFFFFF): a larger
          // key has a larger count, or the same count and a smaller v, so one 64-bit
          // compare keeps it. The loop walks xv = x ^ 0x7FFFFFFF (the key's low word).
          // E needs neither `& act` nor the valid-lane mask: M lies inside act and rem
          // only loses bits.
          const int32_t xv = x ^ 0x7FFFFFFF;
          if constexpr (W > 1) {
            L.xs[g.pid] = xv;
            __syncthreads();
          }
          uint64_t best = (uint64_t)(uint32_t)(INT32_MAX ^ 0x7FFFFFFF);  // count 0, v = INT32_MAX
          Mask<W> rem = act, passB = mzero<W>(), passS = mzero<W>();
          int stage = 2;  // 2: a single pass over every value
          if constexpr (W == 1) {
            // Round 0 with many distinct values (V = 64: ~40 of 64): a value held by h alive
            // senders counts at most h in any mailbox, so values are folded by decreasing
            // holder classes — h >= 3, then h = 2, then h = 1 — and a class is skipped when
            // every updating lane's best count already exceeds its h (it can neither win
            // nor tie). Holders are counted in LDS (the X0 table is free in bitmap mode:
            // every x is an initial value, x - lo < 64). With few distinct initial values
            // the single pass is already short and the counting is skipped.
            if (k == 0 && X0.bmode && __builtin_popcountll(X0.bm) > 8) {
              int32_t* cnt = x0tab[grp];
              cnt[g.lane] = 0;
              const uint32_t slot = (uint32_t)(x - X0.lo) & 63u;
              if (!halted01) atomicAdd(&cnt[slot], 1);
              const int32_t h = cnt[slot];
              rem = mand(act, g.ballot_any(h >= 3));  // every holder of such a value
              passB = mand(act, g.ballot_any(h == 2));
              passS = mandn(act, mor(rem, passB));
              stage = 0;
            }
          }
          while (true) {
            while (many(rem)) {
              const int32_t kv = g.bcast(xv, L.xs, mfirst(rem));
              const Mask<W> E = g.ballot_any(xv == kv);
              rem = mandn(rem, E);
              const uint64_t key = ((uint64_t)(uint32_t)mpopc(mand(M, E)) << 32) | (uint32_t)kv;
              best = key > best ? key : best;
            }
            if (stage == 2) break;
            const uint32_t beat = stage == 0 ? 3u : 2u;  // the next class's values count < beat
            if (!g.any(upd != 0u && (uint32_t)(best >> 32) < beat)) break;
            rem = stage == 0 ? passB : passS;
            ++stage;
          }
          best_c = (int32_t)(best >> 32);
          best_v = (int32_t)((uint32_t)best ^ 0x7FFFFFFFu);
          }  // !folded
          pt.mark(10);
          // x = mmor; decide on > 2n/3 copies, callback only the first time (Otr.scala:64-73)
          x = upd ? best_v : x;
          const uint32_t newdec = upd & gt01(best_c, thr);
          const uint32_t first = newdec & (1u - dec01);
          dec_val = first ? best_v : dec_val;
          dec_round = first ? k : dec_round;
          decision = newdec ? best_v : decision;
          dec01 |= newdec;
          if constexpr (!SH::kFused) X0.maybe_out01_2(decision, x, od, ox);
        }
        }  // !settled
        // after -= 1 once decided; exitAtEndOfRound when it reaches 0 (Otr.scala:75-80)
        const uint32_t ad = (1u - halted01) & dec01;
        after -= (int32_t)ad;
        const uint32_t h = ad & gt01(1, after);
        halt_round = h ? k : halt_round;
        halted01 |= h;
      }
      pt.mark(11);
      if constexpr (!SH::kFused)
        otr_check<W, V2>(g, L, X0, ck, k + 1, true, n, full, x, dec01, decision, old01, old_decision, valid01, od, ox, ckthr);
      if (tracing_on) trace(k + 1, hs);
      pt.mark(1);
    }
    // Rounds kf .. R-1: every process has halted, so no process takes a step and the state, the
    // pre-round (old) state included, is the final one; the Spec is still evaluated at each of
    // these check points, kf + 1 .. R (Otr.scala:95-120 over the frozen state).
    // W == 1 with the built-in checker and no trace: in groups of kFrozenGroup check points
    // (otr_check_frozen_group) while that many are left and the state is settled; the rest of the
    // tail — the remainder, or all of it from a group that found the state unsettled, which a
    // frozen state then stays — goes through the loop below. The seeded TR form is not among
    // them: launch_w sends it traced launches only, and it keeps the code it had (with the groups
    // compiled in and never run, its G1 row measured 0.6 % slower).
    int kt = kf;
    if constexpr (W == 1 && !SH::kFused && (XHO || !TR)) {
      if (!tracing_on) {
        while (kt + kFrozenGroup <= a.R &&
               otr_check_frozen_group<kFrozenGroup, V2>(g, ck, kt + 1, x, dec01, decision, valid01, od, ox, ckthr)) {
          kt += kFrozenGroup;
          pt.mark(2);
        }
      }
    }
    for (int k = kt; k < a.R; ++k) {
      if constexpr (!SH::kFused)
        otr_check<W, V2, true>(g, L, X0, ck, k + 1, true, n, full, x, dec01, decision, dec01, decision, valid01, od, ox, ckthr);
      if (tracing_on) trace(k + 1, n, true);
      pt.mark(2);
    }
    pt.add(6, 1u);  // event build: instances
    if constexpr (W == 1)
      finish_instance_w1(g, a, i, hook_checks<SH>(sh, ck), hook_slots<SH>(kOtrChecks), dec_val, dec_round, halt_round, x,
                         &bc, &tally, &wtally, live_rounds, lb, &pt);
    else
      finish_instance<W>(g, a, i, hook_checks<SH>(sh, ck), hook_slots<SH>(kOtrChecks), dec_val, dec_round, halt_round, x,
                         &bc, &tally, live_rounds, &pt);
    pt.mark(3);
  }
  pt.flush(a.counters, threadIdx.x & 63);
  tally.flush(&bc);
  if constexpr (W == 1) wtally.flush(&bc, hook_slots<SH>(kOtrChecks));
  __syncthreads();
  counters_flush(&bc, a.counters, hook_slots<SH>(kOtrChecks), a.R);
}

#ifndef PSG_OTR_WPE
#define PSG_OTR_WPE 6
#endif
template <int W, bool V2, bool XHO, class SH = NoHook, bool TR = true>
__global__ void __launch_bounds__(Geometry<W>::kThreads) __attribute__((amdgpu_waves_per_eu(W == 1 ? PSG_OTR_WPE : 1)))
otr_kernel(KArgs a) {
  otr_body<W, V2, XHO, SH, TR>(a);
}

// otr_kernel<1, V2, false, NoHook, false> for a plain schedule (otr_body's PLAIN); a kernel of its
// own name, so that every other instantiation keeps its symbol. 7 waves per SIMD: the interleaved
// pair of Sched::and_words fits the step at 72 VGPRs
template <bool V2>
__global__ void __launch_bounds__(Geometry<1>::kThreads) __attribute__((amdgpu_waves_per_eu(7)))
otr_plain_kernel(KArgs a) {
  otr_body<1, V2, false, NoHook, false, true>(a);
}

#ifndef PSG_FUSED_MODULE  // host launchers (not part of a fused Spec module)
template <int W, bool V2>
static hipError_t launch_w(const KArgs& a, int grid, hipStream_t s) {
  if (a.ho_in) return launch_grp<W>(otr_kernel<W, V2, true>, a, grid, s);
  if (a.trace) return launch_grp<W>(otr_kernel<W, V2, false>, a, grid, s);
  if constexpr (W == 1) {  // the default HOSchedule: no crashes, no ho_min
    if (plain_schedule(a)) return launch_grp<W>(otr_plain_kernel<V2>, a, grid, s);
  }
  return launch_grp<W>(otr_kernel<W, V2, false, NoHook, false>, a, grid, s);
}

template <bool V2>
static hipError_t launch_v(const KArgs& a, int W, int grid, hipStream_t s) {
  return with_w(W, hipErrorInvalidValue, [&](auto w) { return launch_w<w(), V2>(a, grid, s); });
}

// The kernel a seeded, trace-free launch of this schedule goes to (launch_w's choice): the one
// the resident-block count is taken from.
template <bool V2>
static const void* ptr_v(int W, bool plain) {
  if (W == 1 && plain) return (const void*)otr_plain_kernel<V2>;
  return with_w(W, (const void*)nullptr, [](auto w) { return (const void*)otr_kernel<w(), V2, false, NoHook, false>; });
}

hipError_t launch_otr(const KArgs& a, int W, int grid, hipStream_t s) { return launch_v<false>(a, W, grid, s); }
hipError_t launch_otr2(const KArgs& a, int W, int grid, hipStream_t s) { return launch_v<true>(a, W, grid, s); }
const void* otr_kernel_ptr(int W) { return ptr_v<false>(W, false); }
const void* otr2_kernel_ptr(int W) { return ptr_v<true>(W, false); }
const void* otr_plain_kernel_ptr(int W) { return ptr_v<false>(W, true); }
const void* otr2_plain_kernel_ptr(int W) { return ptr_v<true>(W, true); }

#endif  // PSG_FUSED_MODULE

}  // namespace psg
