// Edit, indel and gap-linear distances under an ends-free span for SHORT wavefronts (tier 5 for a metric with a span): the M ring in
// registers, a group of lanes per alignment -- a code object of its own, loaded by the first metric-with-span call whose window bound
// fits a group (or by wfagpu_amd_prime once a metric is configured with a span).
//
// What the path is used for -- a barcode, UMI or primer in a window, a short read placed in a candidate region -- is 16 to 150 bases, a
// handful of errors and a few free bases at the text's ends; the one-wave kernels (align_kernel_linef.hip) give every such pair a
// wavefront, an LDS ring and a row book.  Here the work split is short_kernel_lin.hip's: lane j is diagonal wlo + j for the whole
// alignment, the history is M of the last D = max(x, g) scores in D registers, the loop is unrolled D times, two lane shifts per cell.
// What the span changes (short_kernel_body.inc, EF):
//   window   the hull of the start diagonals [-pbf, tbf] and the end diagonals [kend - tef, kend + pef] and what the budget affords
//            beyond it (align_kernel.hip, LINEAR && ENDSFREE) -- rarely 8 wide, often more than 32: groups of L = 16, 32 or 64 lanes.
//            L == 64 is the whole wavefront: one alignment per wavefront like the one-wave kernels, but no LDS ring, no row book, the
//            staging pipeline and the arena slots without atomics of this tier; its neighbour shifts are DPP wave shifts.
//   score 0  every lane of [-pbf, tbf] extends from its border cell max(k, 0)
//   the end  a lane of [kend - tef, kend + pef] whose cell has reached the end of its diagonal (h >= min(tlen, plen + k), the lane
//            constant of the validity test) ends the alignment; the lowest such lane of the group wins and goes to
//            WfaAlignParams::ends with the score (ends[2 pair] is the backtrace's, as in the one-wave kernels)
// Rows of origin bytes, row table and arena slots are the tier's; trace_kernel_lin.hip reads them under a span as from any tier.
// BAND, SCORE and NOMEM failures and the byte-compare class go on to the one-wave kernels of align_kernel_linef.hip.
#include "short_kernel_impl.h"

namespace {

// X == 0: indel
template <int L, int X, int GAP, bool BT, bool ASCII>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8)))
wfa_short_linef_kernel(const WfaAlignParams p) {
  constexpr bool LIN = true, EF = true, TP2 = false;
  constexpr int OE = GAP, E = GAP, OE2 = GAP, E2 = GAP;      // (every gap base costs g, nothing opens; OE2 / E2: two pieces only)
#include "short_kernel_body.inc"
}

template <int L, int X, int G, bool BT, bool ASCII>
void launch_short_linef(const WfaAlignParams& p, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const size_t lds = wfa_short_lds_bytes(p, L, BT);
  wfa_launch_timed(wfa_short_linef_kernel<L, X, G, BT, ASCII>, dim3(grid), dim3(64), lds, stream, ev0, ev1, p);
}

template <int L, int X, int G, bool BT, bool ASCII>
int occ_short_linef(size_t lds) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(wfa_short_linef_kernel<L, X, G, BT, ASCII>), 64, lds) != hipSuccess) { nb = 0; (void)hipGetLastError(); }
  return nb;
}

// [x][g - 1], x = 0 for indel (g == 1 only), x = 1..8, g = 1..4 (short_kernel_lin.hip's table): one per group width, mode and input.
// No groups of 8: a span adds pbf + tbf diagonals before any error, and a span of zeros belongs on the end-to-end call.
template <int L, bool BT, bool ASCII, int I> constexpr WfaShortEntry short_linef_entry() {
  if constexpr (I / 4 > 0 || I % 4 == 0) return {&launch_short_linef<L, I / 4, I % 4 + 1, BT, ASCII>, &occ_short_linef<L, I / 4, I % 4 + 1, BT, ASCII>};
  else return {nullptr, nullptr};
}
template <int L, bool BT, bool ASCII, int... Is> constexpr std::array<WfaShortEntry, 36> short_linef_table(std::integer_sequence<int, Is...>) { return {short_linef_entry<L, BT, ASCII, Is>()...}; }
template <bool BT, bool ASCII> constexpr std::array<std::array<WfaShortEntry, 36>, 3> short_linef_widths() {
  return {short_linef_table<16, BT, ASCII>(std::make_integer_sequence<int, 36>{}), short_linef_table<32, BT, ASCII>(std::make_integer_sequence<int, 36>{}),
          short_linef_table<64, BT, ASCII>(std::make_integer_sequence<int, 36>{})};
}

const WfaShortEntry& short_linef_pick(const WfaAlignParams& p, int lanes, bool with_bt) {
  // [ASCII][BT][lanes: 16, 32, 64]
  static const std::array<std::array<WfaShortEntry, 36>, 3> t[2][2] = {{short_linef_widths<false, false>(), short_linef_widths<true, false>()},
                                                                       {short_linef_widths<false, true>(), short_linef_widths<true, true>()}};
  const int xi = p.x >= WFA_LIN_NO_MISMATCH ? 0 : p.x;
  wfa_unit_entered(WFA_UNIT_SHORT_LINEF);
  return t[p.ascii ? 1 : 0][with_bt ? 1 : 0][lanes == 16 ? 0 : lanes == 32 ? 1 : 2][xi * 4 + (p.e - 1)];
}

}  // namespace

// (the penalties are judged by wfa_short_lin_supported: the same table)
void wfa_launch_short_linef(const WfaAlignParams& p, int lanes, bool with_bt, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  short_linef_pick(p, lanes, with_bt).launch(p, grid, stream, ev0, ev1);
}

int wfa_short_linef_max_blocks_per_cu(const WfaAlignParams& p, int lanes, bool with_bt) { return short_linef_pick(p, lanes, with_bt).occ(wfa_short_lds_bytes(p, lanes, with_bt)); }

namespace { __global__ void k_prime_short_linef() {} }
void wfa_prime_short_linef(hipStream_t stream) { wfa_unit_entered(WFA_UNIT_SHORT_LINEF); hipLaunchKernelGGL(k_prime_short_linef, dim3(1), dim3(64), 0, stream); }
