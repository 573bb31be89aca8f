// The backtrace of edit, indel and gap-linear alignments: trace_kernel.hip compiled with one walk state and BTL_* origin bytes -- a
// translation unit (and so a code object) of its own behind wfa_launch_trace_lin, so that the gap-affine and two-piece backtrace
// kernels carry none of it and their callers never load it.
#define WFA_TRACE_LINEAR_UNIT 1
#include "trace_kernel.hip"
