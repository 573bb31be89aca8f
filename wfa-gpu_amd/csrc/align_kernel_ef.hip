// The ends-free instantiations of the wavefront kernel: a translation unit (and so a code object) of their own, so that end-to-end
// callers never load them.  The kernel is align_kernel.hip; with this macro it defines the launchers of the ENDSFREE instantiations
// instead of those of the end-to-end ones.
#define WFA_ALIGN_ENDSFREE_UNIT 1
#include "align_kernel.hip"
