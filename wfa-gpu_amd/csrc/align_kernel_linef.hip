// The instantiations of the wavefront kernel for a one-component metric (edit, indel, gap-linear) under an ends-free span: a translation
// unit (and so a code object) of their own, so that no other caller loads them.  The kernel is align_kernel.hip; with this macro it
// defines the launchers of the LINEAR && ENDSFREE instantiations instead of those of the gap-affine ones.
#define WFA_ALIGN_LINEF_UNIT 1
#include "align_kernel.hip"
