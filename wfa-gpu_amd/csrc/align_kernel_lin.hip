// The one-component instantiations of the wavefront kernel (WFA2's edit, indel and gap_linear distances): a translation unit (and so a
// code object) of their own, so that gap-affine callers never load them.  The kernel is align_kernel.hip; with this macro it defines
// the launchers of the LINEAR instantiations instead of those of the gap-affine ones.
#define WFA_ALIGN_LINEAR_UNIT 1
#include "align_kernel.hip"
