// The two-piece gap-affine instantiations of the wavefront kernel (WFA2's gap_affine_2p): a translation unit (and so a code object)
// of their own, so that gap-affine callers never load them.  The kernel is align_kernel.hip; with this macro it defines the launchers
// of the TWOPIECE instantiations instead of those of the gap-affine ones.
#define WFA_ALIGN_TWOPIECE_UNIT 1
#include "align_kernel.hip"
