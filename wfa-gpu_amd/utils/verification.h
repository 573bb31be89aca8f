/* Checkers behind the CLI's -c flag.  They restate what the reference's -c
 * path verifies (lib/align.cu:258-326, utils/verification.c:27-146): the
 * CIGAR replays onto both sequences, its gap-affine cost equals the reported
 * score, and the score equals an independent CPU computation.  Checker
 * only: nothing here ever produces a result the library returns. */
#ifndef WFAGPU_VERIFICATION_H
#define WFAGPU_VERIFICATION_H

#include <stdbool.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* RLE CIGAR ("12M1X3I...") replays exactly onto pattern and text. */
bool check_cigar_edit(const char* text, const char* pattern, size_t tlen, size_t plen,
                      const char* cigar);

/* Sum of penalties of the CIGAR equals `distance`. */
bool check_affine_distance(const char* text, const char* pattern, size_t tlen, size_t plen,
                           int distance, int x, int o, int e, const char* cigar);

/* Optimal gap-affine score by a scalar dynamic program over (score,
 * diagonal); O(score * width) time.  Independent of the GPU kernels.
 * The working memory belongs to the caller: one zero-initialised
 * verification_scratch_t per worker thread, reused across pairs (it only
 * grows) and released with verification_scratch_free -- nothing is kept in
 * thread-local storage, so short-lived worker threads leak nothing. */
typedef struct { int* buf; size_t cap; } verification_scratch_t;
int verification_cpu_score_scratch(const char* pattern, const char* text, size_t plen, size_t tlen,
                                   int x, int o, int e, verification_scratch_t* scratch);
void verification_scratch_free(verification_scratch_t* scratch);
/* One-off form: allocates and frees its own scratch. */
int verification_cpu_score(const char* pattern, const char* text, size_t plen, size_t tlen,
                           int x, int o, int e);

/* Ends-free alignment (wfagpu_amd_span_t; include/wfa_gpu_device.h).  span = {pattern_begin_free, pattern_end_free,
 * text_begin_free, text_end_free}, each clamped to its sequence here; NULL: end to end.
 * The CIGAR of an ends-free alignment covers both whole sequences (check_cigar_edit as it is); its cost is taken
 * WITHOUT the free bases: a leading D (I) run is free for as many bases as pattern_begin_free (text_begin_free)
 * allows, a trailing one for pattern_end_free (text_end_free).  The score itself is checked against the dynamic
 * program below, which starts on the free part of the first row / column and stops at the first score whose
 * wavefront reaches the free part of the last ones. */
bool check_affine_distance_span(const char* text, const char* pattern, size_t tlen, size_t plen,
                                int distance, int x, int o, int e, const char* cigar, const int* span);
int verification_cpu_score_span_scratch(const char* pattern, const char* text, size_t plen, size_t tlen,
                                        int x, int o, int e, const int* span, verification_scratch_t* scratch);
int verification_cpu_score_span(const char* pattern, const char* text, size_t plen, size_t tlen,
                                int x, int o, int e, const int* span);

/* Two-piece gap-affine (wfagpu_amd_penalties2p_t; include/wfa_gpu_device.h): a gap run of n bases is priced
 * min(o1 + n e1, o2 + n e2) -- a CIGAR does not say which piece a gap used; the score is checked against the
 * program of verification_cpu_score_scratch with five tables (M, and I / D once per piece). */
bool check_affine2p_distance(const char* text, const char* pattern, size_t tlen, size_t plen,
                             int distance, int x, int o1, int e1, int o2, int e2, const char* cigar);
int verification_cpu_score_2p_scratch(const char* pattern, const char* text, size_t plen, size_t tlen,
                                      int x, int o1, int e1, int o2, int e2, verification_scratch_t* scratch);
int verification_cpu_score_2p(const char* pattern, const char* text, size_t plen, size_t tlen,
                              int x, int o1, int e1, int o2, int e2);

/* Under a heuristic (wfagpu_amd_wfadaptive_t; include/wfa_gpu_device.h) the CIGAR is checked as always -- it replays, its cost
 * is the score -- but the score may lie above the optimum.  The verdict on a score against the CPU scorer's optimum: 0 equal,
 * > 0 the excess of a score above the optimum (counted and said by -c, no failure), -1 a score BELOW the optimum (a failure). */
int verification_heuristic_verdict(int distance, int optimum);

/* Edit, indel and gap-linear distances (wfagpu_amd_linear_t; include/wfa_gpu_device.h): metric 0 indel, 1 edit, 2 gap-linear with
 * mismatch x and gap base g (x and g are read under gap-linear only).  The CIGAR is priced under the metric -- an X under indel is a
 * failure --, the score checked against a one-table scalar program (-1: a bad metric, or no memory). */
bool check_linear_distance(const char* text, const char* pattern, size_t tlen, size_t plen,
                           int distance, int metric, int x, int g, const char* cigar);
int verification_cpu_score_linear(const char* pattern, const char* text, size_t plen, size_t tlen, int metric, int x, int g);

/* A one-component metric under an ends-free span (wfagpu_amd_align_device_linear_span, --metric-ends-free): span as above.  The CIGAR
 * is priced under the metric WITHOUT its free bases -- a leading D (I) run is free for as many bases as pattern_begin_free
 * (text_begin_free) allows, a trailing one for pattern_end_free (text_end_free); an X under indel is a failure --, the score checked
 * against the one-table scalar program with free borders. */
bool check_linear_distance_span(const char* text, const char* pattern, size_t tlen, size_t plen,
                                int distance, int metric, int x, int g, const char* cigar, const int* span);
int verification_cpu_score_linear_span(const char* pattern, const char* text, size_t plen, size_t tlen, int metric, int x, int g, const int* span);

#ifdef __cplusplus
}
#endif
#endif
