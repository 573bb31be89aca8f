// The wf-adaptive instantiations of the wavefront kernel under two-piece penalties (WFA2's default heuristic on gap_affine_2p): a
// translation unit (and so a code object) of their own, so that nobody else loads them.  The kernel is align_kernel.hip; with this
// macro it defines the launchers of the ADAPTIVE && TWOPIECE instantiations instead of those of the gap-affine ones.
#define WFA_ALIGN_2PAD_UNIT 1
#include "align_kernel.hip"
