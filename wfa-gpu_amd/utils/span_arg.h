/* The argument of --metric-ends-free: "pb,pe,tb,te" -- four non-negative integers with nothing behind them.
 * Kept apart from the tool so that a test program can run it under the sanitizers. */
#ifndef WFAGPU_SPAN_ARG_H
#define WFAGPU_SPAN_ARG_H
#include <stdbool.h>
#include <stdio.h>

/* -> true and out4 = {pb, pe, tb, te}; false (out4 untouched): fewer or more than four fields, a field that is no integer, a
 * negative one, or anything behind the fourth. */
static inline bool span_arg_parse(const char* s, int out4[4]) {
    int v[4] = {0, 0, 0, 0};
    char tail = 0;
    if (!s || sscanf(s, "%d,%d,%d,%d%c", &v[0], &v[1], &v[2], &v[3], &tail) != 4) return false;
    for (int i = 0; i < 4; ++i) if (v[i] < 0) return false;
    for (int i = 0; i < 4; ++i) out4[i] = v[i];
    return true;
}
#endif
