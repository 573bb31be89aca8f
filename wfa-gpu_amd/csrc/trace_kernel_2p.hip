// The two-piece gap-affine backtrace: trace_kernel.hip compiled with TRACE_2P set -- a translation unit (and so a code object) of
// its own behind wfa_launch_trace_2p, so that the gap-affine backtrace kernels carry none of it and gap-affine callers never load it.
#define WFA_TRACE_TWOPIECE_UNIT 1
#include "trace_kernel.hip"
