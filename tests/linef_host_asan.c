/* AddressSanitizer + UBSan over the host code of a metric under an ends-free span: the -c checkers of utils/verification.c
 * (check_linear_distance_span, verification_cpu_score_linear_span) and the parser of --metric-ends-free (utils/span_arg.h).
 * A stand-alone program: tests/test_linear_endsfree_cpu.py compiles it with -fsanitize=address,undefined and runs it. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "utils/span_arg.h"
#include "utils/verification.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "linef_host_asan: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static unsigned long long rng_state = 20261021ull;
static unsigned rnd(void) { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(rng_state >> 33); }

int main(void) {
    int sp[4] = {-1, -1, -1, -1};
    /* ---- the option's argument */
    CHECK(span_arg_parse("0,0,50,50", sp) && sp[0] == 0 && sp[1] == 0 && sp[2] == 50 && sp[3] == 50);
    CHECK(span_arg_parse("7,13,21,2147483647", sp) && sp[3] == INT_MAX);
    const int before[4] = {sp[0], sp[1], sp[2], sp[3]};
    CHECK(!span_arg_parse("0,0,50", sp) && !span_arg_parse("0,0,50,50x", sp) && !span_arg_parse("0,0,50,50,1", sp));
    CHECK(!span_arg_parse("0,0,-5,50", sp) && !span_arg_parse("", sp) && !span_arg_parse(NULL, sp) && !span_arg_parse("a,b,c,d", sp));
    CHECK(!span_arg_parse("0,0,50,", sp) && !span_arg_parse(",,,", sp));
    CHECK(memcmp(before, sp, sizeof before) == 0);      /* (a rejected argument leaves the output alone) */

    /* ---- the checkers: a read inside a window.  text = 3 free bases + the pattern with one mismatch and one inserted G + 2 free bases */
    const char* p = "ACGTACGTAC";
    const char* t = "TTTACCTACGGTACAA";
    const size_t pl = strlen(p), tl = strlen(t);
    const int free55[4] = {0, 0, 5, 5}, free21[4] = {0, 0, 2, 1}, zeros[4] = {0, 0, 0, 0}, all[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    const char* cg = "3I2M1X4M1I3M2I";
    CHECK(check_linear_distance_span(t, p, tl, pl, 2, 1, 0, 0, cg, free55));            /* edit: 1 + 1, the runs at the ends free */
    CHECK(!check_linear_distance_span(t, p, tl, pl, 3, 1, 0, 0, cg, free55));
    CHECK(check_linear_distance_span(t, p, tl, pl, 4, 1, 0, 0, cg, free21));            /* free runs longer than allowed: 1 + 1 bases paid */
    CHECK(!check_linear_distance_span(t, p, tl, pl, 2, 1, 0, 0, cg, free21));
    CHECK(check_linear_distance_span(t, p, tl, pl, 7, 1, 0, 0, cg, zeros) && check_linear_distance_span(t, p, tl, pl, 7, 1, 0, 0, cg, NULL));
    CHECK(check_linear_distance_span(t, p, tl, pl, 6, 2, 4, 2, cg, free55) && check_linear_distance_span(t, p, tl, pl, 10, 2, 4, 2, cg, free21));
    CHECK(!check_linear_distance_span(t, p, tl, pl, 2, 0, 0, 0, cg, free55));           /* indel: an X is a failure */
    CHECK(check_linear_distance_span(t, p, tl, pl, 3, 0, 0, 0, "3I2M1I1D4M1I3M2I", free55));
    CHECK(!check_linear_distance_span(t, p, tl, pl, 2, 1, 0, 0, "3I2M1Y4M1I3M2I", free55) && !check_linear_distance_span(t, p, tl, pl, 2, 3, 1, 1, cg, free55));
    CHECK(!check_linear_distance_span(t, p, tl, pl, 2, 1, 0, 0, "3I2M1X4M1I3M2", free55));      /* (malformed) */
    CHECK(check_linear_distance_span(t, p, 4, 0, 0, 1, 0, 0, "4I", all) && check_linear_distance_span(t, p, 4, 0, 1, 1, 0, 0, "4I", free21));   /* one run, both ends */
    CHECK(verification_cpu_score_linear_span(p, t, pl, tl, 1, 0, 0, free55) == 2 && verification_cpu_score_linear_span(p, t, pl, tl, 0, 0, 0, free55) == 3);
    CHECK(verification_cpu_score_linear_span(p, t, pl, tl, 2, 4, 2, free55) == 6 && verification_cpu_score_linear_span(p, t, pl, tl, 1, 0, 0, free21) == 4);
    CHECK(verification_cpu_score_linear_span(p, t, pl, tl, 1, 0, 0, zeros) == verification_cpu_score_linear(p, t, pl, tl, 1, 0, 0));
    CHECK(verification_cpu_score_linear_span(p, t, pl, tl, 1, 0, 0, NULL) == verification_cpu_score_linear(p, t, pl, tl, 1, 0, 0));
    CHECK(verification_cpu_score_linear_span(p, t, pl, tl, 3, 1, 1, free55) == -1 && verification_cpu_score_linear_span(p, t, pl, tl, 2, 0, 1, free55) == -1);
    CHECK(verification_cpu_score_linear_span("", t, 0, tl, 1, 0, 0, free55) == (int)tl - 10 && verification_cpu_score_linear_span(p, "", pl, 0, 1, 0, 0, all) == 0);
    CHECK(verification_cpu_score_linear_span("", "", 0, 0, 0, 0, 0, all) == 0);

    /* ---- random pairs, every metric, spans of every shape (the sequences are exact-size heap blocks: an overrun is seen) */
    static const int spans[6][4] = {{0, 0, 0, 0}, {0, 0, 9, 9}, {9, 9, 0, 0}, {3, 0, 0, 7}, {INT_MAX, INT_MAX, INT_MAX, INT_MAX}, {0, 40, 40, 0}};
    static const int metrics[5][3] = {{1, 0, 0}, {0, 0, 0}, {2, 4, 2}, {2, 1, 3}, {2, 5, 1}};
    for (int it = 0; it < 300; ++it) {
        const size_t a = rnd() % 40, b = rnd() % 40;
        char* pp = (char*)malloc(a ? a : 1); char* tt = (char*)malloc(b ? b : 1);
        CHECK(pp && tt);
        for (size_t i = 0; i < a; ++i) pp[i] = "ACGT"[rnd() & 3];
        for (size_t i = 0; i < b; ++i) tt[i] = (i < a && (rnd() % 8)) ? pp[i] : "ACGT"[rnd() & 3];
        const int* m = metrics[it % 5];
        const int e2e = verification_cpu_score_linear(pp, tt, a, b, m[0], m[1], m[2]);
        int prev = e2e;
        CHECK(e2e >= 0);
        for (int k = 0; k < 6; ++k) {
            const int s = verification_cpu_score_linear_span(pp, tt, a, b, m[0], m[1], m[2], spans[k]);
            CHECK(s >= 0 && s <= e2e);                      /* (the end-to-end alignment is a candidate) */
            if (k == 0) CHECK(s == e2e);
            if (k == 4) CHECK(s == 0);                      /* (everything free: nothing has to be aligned) */
            prev = s;
        }
        (void)prev;
        free(pp); free(tt);
    }
    printf("linef_host_asan ok\n");
    return 0;
}
