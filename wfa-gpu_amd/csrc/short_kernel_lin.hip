// Edit, indel and gap-linear distances for SHORT wavefronts (tier 5 under a metric): several alignments per 64-lane wavefront, the M
// ring in registers -- a code object of its own, loaded by the first metric call whose score budget fits it (or by wfagpu_amd_prime
// once a metric is configured).
//
// The one-wave metric kernels (align_kernel_lin.hip) give every alignment a wavefront and an LDS ring, even where a row is five
// diagonals wide: read-to-candidate filtering, deduplication, barcode and UMI matching -- what these metrics are used for.  Here a
// group of L = 8, 16 or 32 lanes is one alignment and lane j is diagonal wlo + j for the whole alignment, as in short_kernel.hip; the
// history is M of the last D = max(x, g) scores (g under indel) and nothing else: D registers per lane, one under edit, and two DPP
// row shifts per cell.  The kernel is the LIN specialisation of short_kernel_impl.h (staging pipeline, ASCII variants and partial
// sums are the gap-affine kernel's own); the origin bytes are BTL_*, the rows and the row table what trace_kernel_lin.hip reads from
// any tier.  Pairs whose window does not fit a group (BAND), whose score exceeds the budget (SCORE) or that find the arena full
// (NOMEM) go on to the one-wave metric tiers like the failures of any tier.
#include "short_kernel_impl.h"

namespace {

// X == 0: indel
template <int L, int X, int GAP, bool BT, bool ASCII>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8)))
wfa_short_lin_kernel(const WfaAlignParams p) {
  constexpr bool LIN = true, EF = false, TP2 = false;
  constexpr int OE = GAP, E = GAP, OE2 = GAP, E2 = GAP;      // (every gap base costs g, nothing opens; OE2 / E2: two pieces only)
#include "short_kernel_body.inc"
}

template <int L, int X, int G, bool BT, bool ASCII>
void launch_short_lin(const WfaAlignParams& p, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const size_t lds = wfa_short_lds_bytes(p, L, BT);
  wfa_launch_timed(wfa_short_lin_kernel<L, X, G, BT, ASCII>, dim3(grid), dim3(64), lds, stream, ev0, ev1, p);
}

template <int L, int X, int G, bool BT, bool ASCII>
int occ_short_lin(size_t lds) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(wfa_short_lin_kernel<L, X, G, BT, ASCII>), 64, lds) != hipSuccess) { nb = 0; (void)hipGetLastError(); }
  return nb;
}

// [x][g - 1], x = 0 for indel (g == 1 only), x = 1..8, g = 1..4: one table per group width, mode and input
template <int L, bool BT, bool ASCII, int I> constexpr WfaShortEntry short_lin_entry() {
  if constexpr (I / 4 > 0 || I % 4 == 0) return {&launch_short_lin<L, I / 4, I % 4 + 1, BT, ASCII>, &occ_short_lin<L, I / 4, I % 4 + 1, BT, ASCII>};
  else return {nullptr, nullptr};
}
template <int L, bool BT, bool ASCII, int... Is> constexpr std::array<WfaShortEntry, 36> short_lin_table(std::integer_sequence<int, Is...>) { return {short_lin_entry<L, BT, ASCII, Is>()...}; }
template <bool BT, bool ASCII> constexpr std::array<std::array<WfaShortEntry, 36>, 3> short_lin_widths() {
  return {short_lin_table<8, BT, ASCII>(std::make_integer_sequence<int, 36>{}), short_lin_table<16, BT, ASCII>(std::make_integer_sequence<int, 36>{}),
          short_lin_table<32, BT, ASCII>(std::make_integer_sequence<int, 36>{})};
}

const WfaShortEntry& short_lin_pick(const WfaAlignParams& p, int lanes, bool with_bt) {
  // [ASCII][BT][lanes: 8, 16, 32]
  static const std::array<std::array<WfaShortEntry, 36>, 3> t[2][2] = {{short_lin_widths<false, false>(), short_lin_widths<true, false>()},
                                                                       {short_lin_widths<false, true>(), short_lin_widths<true, true>()}};
  const int xi = p.x >= WFA_LIN_NO_MISMATCH ? 0 : p.x;
  wfa_unit_entered(WFA_UNIT_SHORT_LIN);
  return t[p.ascii ? 1 : 0][with_bt ? 1 : 0][lanes == 8 ? 0 : lanes == 16 ? 1 : 2][xi * 4 + (p.e - 1)];
}

}  // namespace

// (after the common-factor reduction; x = WFA_LIN_NO_MISMATCH: indel, whose gap base is 1)
bool wfa_short_lin_supported(int x, int g) { return g >= 1 && g <= 4 && ((x >= 1 && x <= 8) || (x >= WFA_LIN_NO_MISMATCH && g == 1)); }

void wfa_launch_short_lin(const WfaAlignParams& p, int lanes, bool with_bt, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  short_lin_pick(p, lanes, with_bt).launch(p, grid, stream, ev0, ev1);
}

int wfa_short_lin_max_blocks_per_cu(const WfaAlignParams& p, int lanes, bool with_bt) { return short_lin_pick(p, lanes, with_bt).occ(wfa_short_lds_bytes(p, lanes, with_bt)); }

namespace { __global__ void k_prime_short_lin() {} }
void wfa_prime_short_lin(hipStream_t stream) { wfa_unit_entered(WFA_UNIT_SHORT_LIN); hipLaunchKernelGGL(k_prime_short_lin, dim3(1), dim3(64), 0, stream); }
