// short_kernel_impl.h -- the kernel of tier 5 (several alignments per wavefront, rings in registers) and its tables, for ONE gap extension E.
// Included by short_kernel.hip (E = 1: BASELINE configs[1], and everything around the kernels) and by short_kernel_e2/3/4.hip: a
// translation unit -- a code object, compiled in parallel, loaded at its first launch -- per gap extension.
#pragma once
#include <array>
#include <utility>

#include "wfa_device.h"
#include "pack_device.h"

namespace {

constexpr int S_NULL = -(1 << 28);

// value of the lane one diagonal below (k - 1) / above (k + 1) within the group; lanes without such a neighbour get NULL
// (L == 64: the whole wavefront is one group -- a DPP wave shift by one lane, NULL entering at lane 0 / lane 63)
template <int L> __device__ __forceinline__ int from_below(int v, int j) {
  if constexpr (L == 64) return __builtin_amdgcn_update_dpp(S_NULL, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
  else if constexpr (L == 16) return __builtin_amdgcn_update_dpp(S_NULL, v, 0x111 /* row_shr:1 */, 0xF, 0xF, false);
  else if constexpr (L == 8) { const int r = __builtin_amdgcn_update_dpp(S_NULL, v, 0x111, 0xF, 0xF, false); return j == 0 ? S_NULL : r; }      // (a DPP row holds two groups)
  else { const int r = __shfl_up(v, 1, L); return j == 0 ? S_NULL : r; }
}
template <int L> __device__ __forceinline__ int from_above(int v, int j) {
  if constexpr (L == 64) return __builtin_amdgcn_update_dpp(S_NULL, v, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
  else if constexpr (L == 16) return __builtin_amdgcn_update_dpp(S_NULL, v, 0x101 /* row_shl:1 */, 0xF, 0xF, false);
  else if constexpr (L == 8) { const int r = __builtin_amdgcn_update_dpp(S_NULL, v, 0x101, 0xF, 0xF, false); return j == L - 1 ? S_NULL : r; }
  else { const int r = __shfl_down(v, 1, L); return j == L - 1 ? S_NULL : r; }
}

// Two pieces (TP2, short_kernel_2p.hip).  Depth of the M ring: max(x, o1 + e1, o2 + e2) scores back, rounded up to a multiple of e1 and
// of e2 -- the score loop is unrolled once around the M ring, and the I1 / D1 (I2 / D2) rings of e1 (e2) registers must come round to
// their first slot with it, or their indices would not be constants.
constexpr int short2p_ring_depth(int x, int oe1, int e1, int oe2, int e2) {
  int d = x > oe1 ? x : oe1;
  if (oe2 > d) d = oe2;
  while (d % e1 || d % e2) ++d;
  return d;
}
// Its neighbour shifts: as above for 16 lanes; for 32 a DPP wave shift by one lane (the wavefront holds two groups: lane 0 / 31 of a
// group takes NONE instead of what crossed the seam) where from_below / from_above go through the LDS crossbar (ds_bpermute_b32, an
// address register and a round trip per shift: six shifts per score here).
template <int L, int NONE = S_NULL> __device__ __forceinline__ int short2p_from_below(int v, int j) {
  if constexpr (L == 16) return __builtin_amdgcn_update_dpp(NONE, v, 0x111 /* row_shr:1 */, 0xF, 0xF, false);
  else { const int r = __builtin_amdgcn_update_dpp(NONE, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false); return j == 0 ? NONE : r; }
}
template <int L, int NONE = S_NULL> __device__ __forceinline__ int short2p_from_above(int v, int j) {
  if constexpr (L == 16) return __builtin_amdgcn_update_dpp(NONE, v, 0x101 /* row_shl:1 */, 0xF, 0xF, false);
  else { const int r = __builtin_amdgcn_update_dpp(NONE, v, 0x130 /* wave_shl:1 */, 0xF, 0xF, false); return j == L - 1 ? NONE : r; }
}

// X = mismatch, OE = gap open + extend, E = gap extend.  L lanes per alignment.  The history a cell reads -- M of the last
// D = max(X, OE) scores -- is a ring of D registers per lane; the score loop is unrolled D times so that every ring index is a
// compile-time constant (round 3 had the two instantiations of the benchmark penalties; round 4 every set with e == 1 and
// max(x, o + e) <= 8 after the common-factor reduction; round 6 gap extensions to 4: 26 (o + e, e) x 8 x sets, picked from tables,
// one translation unit per gap extension).
// BT (round 4): with CIGARs.  Every cell also leaves its origin byte (wfa_device.h: source of M with WFA2's priority on equal
// offsets -- mismatch, then deletion, then insertion --, gap extension over gap open) in a row of L bytes per score; the rows
// collect in LDS and go out, with the row table, when the alignment is done, into a slot of the arena the work item owns
// without any atomic (a few hundred bytes: budgets are <= 35 here); the backtrace kernels (trace_kernel.hip) read them like
// any other tier's.
// Is it WFA2's CIGAR?  This kernel has no per-row limits and turns every I / D value that ran past a sequence end into NULL
// at once, where WFA2 keeps such values inside a row and trims them at its ends only (wavefront_compute.c:570-603).  The
// two differ only in cells that no optimal alignment passes through (a value past an end cannot lie on a path to the corner,
// and every candidate of a valid cell is itself valid or NULL: a nulled value never was the winning candidate of a cell that
// stays valid in WFA2), so scores, tie-breaks along the optimal path and hence the CIGAR are the same: argued in DESIGN.md
// section 4.2b, searched with scratch/short_cigar_semantics.py (oracle with that one change: 0 of 240 000 indel-heavy short
// pairs differ), and held by the parity tests, which compare every CIGAR of this tier with WFA2's.
// ASCII: the batch has not been packed (WfaAlignParams::ascii): the sixteen bytes of a word are what is requested ahead, and the word
// is made when it is staged -- to LDS and to the packed buffer, where the backtrace kernels look for it.  (A pack kernel in front of a
// launch of 100k configs[1] pairs was 18 us + the gap between two launches of a 168 us step; here it is ~80 vector instructions per
// iteration in a kernel whose vector pipe is half idle.)  A pair with a byte outside ACGT leaves with status ALPHABET like in the
// wavefront kernels that pack while staging (align_kernel.hip).
// (register budget: the CIGAR variants came out one and three registers above a step of the occupancy table -- 81 and 99 for x, o, e =
// 2, 3, 1 -- and are compiled for the step below: 1M configs[1] pairs with CIGARs 1.096 -> 1.045 ms per step, 100k the same; the
// score-only variants sit on their steps, 72 and 80, by themselves)
// E > 1 (round 6; the reference's kernels take any penalties, lib/kernels/sequence_distance_kernel.cu:57-160, and its own tests run
// (5,3,2), (3,5,2) and (3,1,4): tests/test_api.c:59-219): I and D of the last D scores are rings of registers like M -- I[s-E] and
// D[s-E] are what a gap extension reads --, 3 D registers of history instead of D + 2; E == 1 keeps its two registers.
// LIN (short_kernel_lin.hip: a code object of its own): the one-component metrics -- edit, indel, gap-linear.  Every gap base costs
// OE == E == g and nothing opens; X == 0 is indel, which has no mismatch move.  M[s][k] = max(M[s-x][k] + 1, M[s-g][k-1] + 1, M[s-g][k+1])
// (the cells of align/loop_careful_lin.inc): the ring of D = max(x, g) registers of M is the whole history -- there is no I or D, so
// nothing is nulled early and the note above does not arise --, two neighbour shifts per cell instead of four; under edit the mismatch
// and both shifts read the one register there is.  Origin bytes are BTL_* (what trace_kernel_lin.hip reads), window, feasibility and
// the worst score per pair are the LINEAR formulas of align_kernel.hip.  L == 8 (LIN only): eight alignments per wavefront, two groups
// per DPP row -- the shifts' boundary lanes are forced to NULL --, a row of origin bytes padded to one 16-byte unit.
// Everything around the cells -- the software pipeline, the staging, the partial sums -- is one body for both: short_kernel_body.inc.
template <int L, int X, int OE, int E, bool BT, bool ASCII>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((BT && E == 1) ? (ASCII ? 5 : 6) : 1, 8)))
wfa_short_kernel(const WfaAlignParams p) {
  constexpr bool LIN = false, EF = false, TP2 = false;
  constexpr int OE2 = OE, E2 = E;      // (two pieces only: short_kernel_2p.hip)
#include "short_kernel_body.inc"
}

template <int L, int X, int OE, int E, bool BT, bool ASCII>
void launch_short(const WfaAlignParams& p, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const size_t lds = wfa_short_lds_bytes(p, L, BT);
  wfa_launch_timed(wfa_short_kernel<L, X, OE, E, BT, ASCII>, dim3(grid), dim3(64), lds, stream, ev0, ev1, p);
}

// wavefronts of this instantiation a CU holds (registers and LDS)
template <int L, int X, int OE, int E, bool BT, bool ASCII>
int occ_short(size_t lds) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(wfa_short_kernel<L, X, OE, E, BT, ASCII>), 64, lds) != hipSuccess) { nb = 0; (void)hipGetLastError(); }
  return nb;
}

// [x - 1][oe - 1], one table per group width, mode and input (packed words / ASCII); sets with o + e < e do not exist (null entries)
template <int L, int E, bool BT, bool ASCII, int I> constexpr WfaShortEntry short_entry() {
  if constexpr (I % 8 + 1 >= E) return {&launch_short<L, I / 8 + 1, I % 8 + 1, E, BT, ASCII>, &occ_short<L, I / 8 + 1, I % 8 + 1, E, BT, ASCII>};
  else return {nullptr, nullptr};
}
template <int L, int E, bool BT, bool ASCII, int... Is> constexpr std::array<WfaShortEntry, 64> short_table(std::integer_sequence<int, Is...>) { return {short_entry<L, E, BT, ASCII, Is>()...}; }
// [ASCII][BT][L == 32]
template <int E> struct ShortTables {
  static const WfaShortEntry* pick(int ascii, int bt, int l32, int idx) {
    static const std::array<WfaShortEntry, 64> t[2][2][2] = {
        {{short_table<16, E, false, false>(std::make_integer_sequence<int, 64>{}), short_table<32, E, false, false>(std::make_integer_sequence<int, 64>{})},
         {short_table<16, E, true, false>(std::make_integer_sequence<int, 64>{}), short_table<32, E, true, false>(std::make_integer_sequence<int, 64>{})}},
        {{short_table<16, E, false, true>(std::make_integer_sequence<int, 64>{}), short_table<32, E, false, true>(std::make_integer_sequence<int, 64>{})},
         {short_table<16, E, true, true>(std::make_integer_sequence<int, 64>{}), short_table<32, E, true, true>(std::make_integer_sequence<int, 64>{})}}};
    return &t[ascii][bt][l32][idx];
  }
};

}  // namespace
