// Two-piece gap-affine alignment (WFA2's gap_affine_2p), end to end, for SHORT wavefronts: tier 5 under two-piece penalties -- a code
// object of its own, loaded by the first two-piece call whose window bound fits a group (or by wfagpu_amd_prime once two-piece
// penalties are configured without a span).
//
// Who meets it: short reads whose long indels are priced by the flat piece -- a 20 to 30 base indel in a 150 bp read costs 44 to 54 under
// WFA2's defaults (4,6,2,24,1), 46 to 66 on the first piece alone -- and anyone who runs one penalty model over mixed read lengths.  The
// one-wave kernels (align_kernel_2p.hip) give each such pair a wavefront, an LDS ring of max(x, o1 + e1, o2 + e2) + 1 rows of M and
// e1 + 1 / e2 + 1 rows of four gap components, and two row books, on their careful loop only.  Here:
//   work split  lane j of a group of L = 16 or 32 lanes is diagonal wlo + j for the whole alignment: four or two alignments per wavefront
//               (no 64-lane groups end to end, as under gap-affine).
//   history     five rings per lane, all in registers: M of the last D scores (D = max(x, o1 + e1, o2 + e2), rounded up to a multiple of
//               e1 and e2: short2p_ring_depth), I1 and D1 of the last e1, I2 and D2 of the last e2 -- 32 registers at WFA2's defaults.
//               The score loop is unrolled D times; every ring index is a constant.
//   cells       align/loop_careful_2p.inc's: I1 = max(M[s-o1-e1], I1[s-e1])[k-1] + 1, I2 likewise, D1 = max(M[s-o1-e1], D1[s-e1])[k+1], D2
//               likewise, M = max(M[s-x] + 1, I1, I2, D1, D2), then the validity compare and the extend out of the staged words.
//   neighbours  the max of opening and extension is taken on the SOURCE lane and crosses once per component: four DPP shifts per score
//               (row shifts for 16 lanes, wave shifts with the seam lane forced to NULL for 32), two more for the extension flags with CIGARs.
//   origin      the 7-bit BT2_* byte of wfa_device.h -- four extension flags, the source of M by WFA2's priority (M, D2, D1, I2, I1) --, rows
//               of L bytes per score in LDS, stored with the row table {unit, wlo} into the pair's static arena slot: what
//               trace_kernel_2p.hip reads from any ROWS producer.
//   window      g(t + |kend|) + g(t) <= S on either side of [min(0, kend), max(0, kend)], feasible iff g(|kend|) <= S (wfa_gap2p,
//               wfa_stray2p: align_kernel.hip's); wider than the group: BAND, unaffordable: SCORE -- on to the one-wave two-piece tiers.
// I and D values past a sequence's end are NULL at once, where WFA2 keeps them inside the row: DESIGN.md section 4.16 restates the
// argument of section 4.2b for four gap components.  Everything around the cells -- the three-stage pipeline, the two LDS sets, the ASCII
// variants, the partial sums, the static arena slots -- is short_kernel_body.inc as it is (TP2).
#include "short_kernel_impl.h"

namespace {

// (register budget: no occupancy step is forced; the figures are in profiles/r19/short_2p_kernels.txt)
template <int L, int X, int OE1, int E1, int OE2, int E2, bool BT, bool ASCII>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8)))
wfa_short_2p_kernel(const WfaAlignParams p) {
  constexpr bool LIN = false, EF = false, TP2 = true;
  constexpr int OE = OE1, E = E1;
#include "short_kernel_body.inc"
}

template <int L, int X, int OE1, int E1, int OE2, int E2, bool BT, bool ASCII>
void launch_short_2p(const WfaAlignParams& p, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const size_t lds = wfa_short_lds_bytes(p, L, BT);
  wfa_launch_timed(wfa_short_2p_kernel<L, X, OE1, E1, OE2, E2, BT, ASCII>, dim3(grid), dim3(64), lds, stream, ev0, ev1, p);
}

template <int L, int X, int OE1, int E1, int OE2, int E2, bool BT, bool ASCII>
int occ_short_2p(size_t lds) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(wfa_short_2p_kernel<L, X, OE1, E1, OE2, E2, BT, ASCII>), 64, lds) != hipSuccess) { nb = 0; (void)hipGetLastError(); }
  return nb;
}

// One penalty set (after the common-factor reduction; written x, o1, e1, o2, e2) and its eight kernels: [ASCII][BT][L == 32]
struct Short2pSet { int x, oe1, e1, oe2, e2; WfaShortEntry k[2][2][2]; };
template <int L, int X, int OE1, int E1, int OE2, int E2, bool BT, bool ASCII> constexpr WfaShortEntry short_2p_entry() {
  return {&launch_short_2p<L, X, OE1, E1, OE2, E2, BT, ASCII>, &occ_short_2p<L, X, OE1, E1, OE2, E2, BT, ASCII>};
}
template <int X, int O1, int E1, int O2, int E2> constexpr Short2pSet short_2p_set() {
  constexpr int A = O1 + E1, B = O2 + E2;
  static_assert(short2p_ring_depth(X, A, E1, B, E2) <= 32, "an M ring of at most 32 registers");
  return {X, A, E1, B, E2,
          {{{short_2p_entry<16, X, A, E1, B, E2, false, false>(), short_2p_entry<32, X, A, E1, B, E2, false, false>()},
            {short_2p_entry<16, X, A, E1, B, E2, true, false>(), short_2p_entry<32, X, A, E1, B, E2, true, false>()}},
           {{short_2p_entry<16, X, A, E1, B, E2, false, true>(), short_2p_entry<32, X, A, E1, B, E2, false, true>()},
            {short_2p_entry<16, X, A, E1, B, E2, true, true>(), short_2p_entry<32, X, A, E1, B, E2, true, true>()}}}};
}

// THE table.  WFA2's defaults and the other concave pair of the goldens; then the sets the goldens already cover: a steep first piece;
// (4,6,2,24,2) halved; equal pieces; two cheap sets; (6,9,3,30,3) divided by 3; a second piece that always wins; one that never does;
// the pieces swapped.  Each kernel: no VGPR spill, no scratch (profiles/r19/short_2p_kernels.txt).  Not here: (5,2,6,20,5) -- rings of
// 30 + 12 + 10 registers -- and every set whose M ring is deeper than 32 rows: they stay on the one-wave tiers.
const Short2pSet k_sets[] = {short_2p_set<4, 6, 2, 24, 1>(), short_2p_set<2, 4, 2, 12, 1>(), short_2p_set<5, 3, 4, 10, 1>(), short_2p_set<2, 3, 1, 12, 1>(),
                             short_2p_set<3, 8, 2, 8, 2>(),  short_2p_set<1, 1, 2, 4, 1>(),  short_2p_set<3, 2, 3, 9, 1>(),  short_2p_set<2, 3, 1, 10, 1>(),
                             short_2p_set<4, 6, 2, 3, 1>(),  short_2p_set<2, 1, 1, 1, 3>(),  short_2p_set<4, 24, 1, 6, 2>()};

const Short2pSet* short_2p_find(int x, int oe1, int e1, int oe2, int e2) {
  for (const Short2pSet& s : k_sets)
    if (s.x == x && s.oe1 == oe1 && s.e1 == e1 && s.oe2 == oe2 && s.e2 == e2) return &s;
  return nullptr;
}

// (the caller asked wfa_short_2p_supported first)
const WfaShortEntry& short_2p_pick(const WfaAlignParams& p, int lanes, bool with_bt) {
  wfa_unit_entered(WFA_UNIT_SHORT_2P);
  return short_2p_find(p.x, p.oe, p.e, p.oe2, p.e2)->k[p.ascii ? 1 : 0][with_bt ? 1 : 0][lanes == 16 ? 0 : 1];
}

}  // namespace

// (after the common-factor reduction; oe1 = o1 + e1, oe2 = o2 + e2, as WfaAlignParams carries them.  A look at the table: loads nothing)
bool wfa_short_2p_supported(int x, int oe1, int e1, int oe2, int e2) { return short_2p_find(x, oe1, e1, oe2, e2) != nullptr; }

void wfa_launch_short_2p(const WfaAlignParams& p, int lanes, bool with_bt, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  short_2p_pick(p, lanes, with_bt).launch(p, grid, stream, ev0, ev1);
}

int wfa_short_2p_max_blocks_per_cu(const WfaAlignParams& p, int lanes, bool with_bt) { return short_2p_pick(p, lanes, with_bt).occ(wfa_short_lds_bytes(p, lanes, with_bt)); }

namespace { __global__ void k_prime_short_2p() {} }
void wfa_prime_short_2p(hipStream_t stream) { wfa_unit_entered(WFA_UNIT_SHORT_2P); hipLaunchKernelGGL(k_prime_short_2p, dim3(1), dim3(64), 0, stream); }
