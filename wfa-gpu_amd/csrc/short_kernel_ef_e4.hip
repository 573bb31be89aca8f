// Tier 5 under an ends-free span (short_kernel_ef_impl.h) for gap extension 4: a translation unit of its own (compiled in parallel with
// the others; its code object is loaded when a span call with such penalties first takes the tier).
#include "short_kernel_ef_impl.h"

const WfaShortEntry* wfa_short_ef_entry_e4(int ascii, int bt, int li, int idx) { return ShortEfTables<4>::pick(ascii, bt, li, idx); }
