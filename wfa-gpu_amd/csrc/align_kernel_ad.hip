// The wf-adaptive instantiations of the wavefront kernel (WFA2's default heuristic, wavefront_heuristic.c): a translation unit (and so a
// code object) of their own, so that callers of the exact searches never load them.  The kernel is align_kernel.hip; with this macro it
// defines the launchers of the ADAPTIVE instantiations instead of those of the gap-affine ones.
#define WFA_ALIGN_ADAPTIVE_UNIT 1
#include "align_kernel.hip"
