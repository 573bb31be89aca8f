// Gap-affine alignment under an ends-free span for SHORT wavefronts (tier 5 for the gap-affine span): groups of 16, 32 or 64 lanes, the
// M, I and D rings in registers -- short_kernel_ef_impl.h is the kernel.  This unit holds gap extension 1 and what the host calls;
// short_kernel_ef_e2/3/4.hip hold the other gap extensions.  Code objects of their own, loaded by the first gap-affine span call whose
// window bound fits a group (or by wfagpu_amd_prime once a span is configured without a metric).
#include "short_kernel_ef_impl.h"

namespace {
const WfaShortEntry& short_ef_pick(const WfaAlignParams& p, int lanes, bool with_bt) {
  const int idx = (p.x - 1) * 8 + (p.oe - 1), a = p.ascii ? 1 : 0, b = with_bt ? 1 : 0, l = lanes == 16 ? 0 : lanes == 32 ? 1 : 2;
  wfa_unit_entered(WFA_UNIT_SHORT_EF);
  switch (p.e) {
    case 1: return *ShortEfTables<1>::pick(a, b, l, idx);
    case 2: return *wfa_short_ef_entry_e2(a, b, l, idx);
    case 3: return *wfa_short_ef_entry_e3(a, b, l, idx);
    default: return *wfa_short_ef_entry_e4(a, b, l, idx);
  }
}
}  // namespace

// (the penalties are judged by wfa_short_supported: the same tables)
void wfa_launch_short_ef(const WfaAlignParams& p, int lanes, bool with_bt, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  short_ef_pick(p, lanes, with_bt).launch(p, grid, stream, ev0, ev1);
}

int wfa_short_ef_max_blocks_per_cu(const WfaAlignParams& p, int lanes, bool with_bt) { return short_ef_pick(p, lanes, with_bt).occ(wfa_short_lds_bytes(p, lanes, with_bt)); }

// (this unit's code object; the other gap extensions' are loaded by the first call that launches one of their kernels)
namespace { __global__ void k_prime_short_ef() {} }
void wfa_prime_short_ef(hipStream_t stream) { wfa_unit_entered(WFA_UNIT_SHORT_EF); hipLaunchKernelGGL(k_prime_short_ef, dim3(1), dim3(64), 0, stream); }
