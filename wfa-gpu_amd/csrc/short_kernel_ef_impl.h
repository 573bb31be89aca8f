// short_kernel_ef_impl.h -- tier 5 for gap-affine alignment under an ends-free span, for ONE gap extension E: the kernel and its tables.
// Included by short_kernel_ef.hip (E = 1, and the functions the host calls) and by short_kernel_ef_e2/3/4.hip: a translation unit -- a
// code object, compiled in parallel, loaded at its first launch -- per gap extension, like the end-to-end units (short_kernel_impl.h).
//
// What the path is used for: a short read placed in a candidate window, a primer or adapter at a read's end, an overlap of two short
// reads -- tens to 150 bases, a handful of errors, a few free bases -- under real gap-affine penalties.  The one-wave kernels
// (align_kernel_ef.hip) give every such pair a wavefront, an LDS ring of M, I and D rows and a row book.  Here:
//   work split  lane j of a group of L = 16, 32 or 64 lanes is diagonal wlo + j for the whole alignment; 64 / L alignments per wavefront.
//   history     M of the last D = max(x, o + e) scores in D registers of the lane; I and D of the last score (e == 1: two registers) or
//               of the last D scores (e > 1: rings like M's); the score loop unrolled D times, every ring index a constant.
//   neighbours  M[s-o-e][k-1], I[s-e][k-1], M[s-o-e][k+1], D[s-e][k+1]: four lane shifts per cell -- DPP row shifts for L == 16, DPP
//               wave shifts (wave_shr:1 / wave_shl:1, NULL entering at lanes 0 and 63) for L == 64: the wavefront is then ONE alignment
//               whose window runs across all four DPP rows, still without an LDS ring, a row book or a cross-lane LDS permute.
//   LDS         the packed sequences of this iteration's and the next one's pairs (the staging pipeline of short_kernel_body.inc) and,
//               with CIGARs, the group's rows of L origin bytes (BT_*), which go to the pair's static arena slot in 16-byte pieces.
// What the span changes in the shared body (EF; the one-component metrics have run under it since short_kernel_linef.hip):
//   window      the hull of the start diagonals [-pbf, tbf] and the end diagonals [kend - tef, kend + pef], widened by what the budget
//               affords for one gap out and one gap back: (S - 2o + (tbf + kend + pef) e) / 2e above, symmetric below (align_kernel.hip,
//               ENDSFREE); feasible: o + gap e <= S for the gap between the two intervals.
//   score 0     every lane of [-pbf, tbf] extends M from its border cell max(k, 0); I and D start NULL (wavefront_unialign.c:137-178).
//   the end     an M cell on a lane of [kend - tef, kend + pef] that reached the end of its diagonal ends the alignment; the lowest such
//               lane of the group wins (WFA2 scans the M wavefront from its lowest diagonal: wavefront_extend.c:124-170) and goes to
//               WfaAlignParams::ends.  I and D values never end an alignment.
// The backtrace (trace_kernel.hip) reads the row table {unit of the row, its lower diagonal} and BT_* rows as from any tier; under a span
// it starts from ends[1], stops at a border and prints the free runs -- nothing there depends on the tier that wrote the rows.
// BAND, SCORE and NOMEM failures and the byte-compare class go on to the one-wave kernels of align_kernel_ef.hip.
#pragma once
#include "short_kernel_impl.h"

namespace {

// (register budget: no occupancy step is forced.  The end-to-end unit compiles its e == 1 CIGAR kernels for 6 (from ASCII: 5) waves per
// SIMD; the same rule here, A/B'd on one MI355X with CIGARs under (2,3,1): 16 and 32 lanes within the run-to-run spread -- 1M barcodes
// 0.549-0.557 against 0.554-0.562 ms and 0.854-0.857 against 0.849-0.853 ms --, 64 lanes, which sit at 62-68 VGPRs by themselves, 4 % and
// 1 % slower -- 1.292 against 1.234-1.243 ms, 100k x 150 bp at 5 % 0.753 against 0.740-0.749 ms: profiles/r16/waves_per_eu_ab.txt.  The
// e > 1 CIGAR kernels carry three rings of up to eight registers and reach 125 VGPRs at 32 lanes: four waves per SIMD, no spill.)
template <int L, int X, int OE, int E, bool BT, bool ASCII>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8)))
wfa_short_ef_kernel(const WfaAlignParams p) {
  constexpr bool LIN = false, EF = true, TP2 = false;
  constexpr int OE2 = OE, E2 = E;      // (two pieces only: short_kernel_2p.hip)
#include "short_kernel_body.inc"
}

template <int L, int X, int OE, int E, bool BT, bool ASCII>
void launch_short_ef(const WfaAlignParams& p, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const size_t lds = wfa_short_lds_bytes(p, L, BT);
  wfa_launch_timed(wfa_short_ef_kernel<L, X, OE, E, BT, ASCII>, dim3(grid), dim3(64), lds, stream, ev0, ev1, p);
}

template <int L, int X, int OE, int E, bool BT, bool ASCII>
int occ_short_ef(size_t lds) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(wfa_short_ef_kernel<L, X, OE, E, BT, ASCII>), 64, lds) != hipSuccess) { nb = 0; (void)hipGetLastError(); }
  return nb;
}

// [x - 1][oe - 1] like the end-to-end tables; sets with o + e < e do not exist (null entries)
template <int L, int E, bool BT, bool ASCII, int I> constexpr WfaShortEntry short_ef_entry() {
  if constexpr (I % 8 + 1 >= E) return {&launch_short_ef<L, I / 8 + 1, I % 8 + 1, E, BT, ASCII>, &occ_short_ef<L, I / 8 + 1, I % 8 + 1, E, BT, ASCII>};
  else return {nullptr, nullptr};
}
template <int L, int E, bool BT, bool ASCII, int... Is> constexpr std::array<WfaShortEntry, 64> short_ef_table(std::integer_sequence<int, Is...>) { return {short_ef_entry<L, E, BT, ASCII, Is>()...}; }
template <int E, bool BT, bool ASCII> constexpr std::array<std::array<WfaShortEntry, 64>, 3> short_ef_widths() {
  return {short_ef_table<16, E, BT, ASCII>(std::make_integer_sequence<int, 64>{}), short_ef_table<32, E, BT, ASCII>(std::make_integer_sequence<int, 64>{}),
          short_ef_table<64, E, BT, ASCII>(std::make_integer_sequence<int, 64>{})};
}
// [ASCII][BT][lanes: 16, 32, 64]
template <int E> struct ShortEfTables {
  static const WfaShortEntry* pick(int ascii, int bt, int li, int idx) {
    static const std::array<std::array<WfaShortEntry, 64>, 3> t[2][2] = {{short_ef_widths<E, false, false>(), short_ef_widths<E, true, false>()},
                                                                         {short_ef_widths<E, false, true>(), short_ef_widths<E, true, true>()}};
    return &t[ascii][bt][li][idx];
  }
};

}  // namespace
