/* See verification.h.  Used only when check_correctness is set. */
#include "verification.h"

#include <stdlib.h>
#include <string.h>

static const char* next_item(const char* c, long* n, char* op) {
    long v = 0;
    if (*c < '0' || *c > '9') return NULL;
    /* (a run longer than any sequence is not a CIGAR of this pair: refused before the accumulator can overflow --
     * found by the UBSan harness, tests/host_api_asan.c) */
    while (*c >= '0' && *c <= '9') { v = v * 10 + (*c - '0'); ++c; if (v > 0x7FFFFFFFL) return NULL; }
    if (!*c || v <= 0) return NULL;
    *n = v; *op = *c;
    return c + 1;
}

bool check_cigar_edit(const char* text, const char* pattern, size_t tlen, size_t plen,
                      const char* cigar) {
    size_t v = 0, h = 0;
    const char* c = cigar;
    while (*c) {
        long n; char op;
        c = next_item(c, &n, &op);
        if (!c) return false;
        for (long i = 0; i < n; ++i) {
            switch (op) {
                case 'M': if (v >= plen || h >= tlen || pattern[v] != text[h]) return false; ++v; ++h; break;
                case 'X': if (v >= plen || h >= tlen || pattern[v] == text[h]) return false; ++v; ++h; break;
                case 'I': if (h >= tlen) return false; ++h; break;
                case 'D': if (v >= plen) return false; ++v; break;
                default: return false;
            }
        }
    }
    return v == plen && h == tlen;
}

bool check_affine_distance(const char* text, const char* pattern, size_t tlen, size_t plen,
                           int distance, int x, int o, int e, const char* cigar) {
    (void)text; (void)pattern; (void)tlen; (void)plen;
    long cost = 0;
    char prev = 0;
    const char* c = cigar;
    while (*c) {
        long n; char op;
        c = next_item(c, &n, &op);
        if (!c) return false;
        if (op == 'X') cost += n * x;
        else if (op == 'I' || op == 'D') cost += (prev == op ? 0 : o) + n * e;
        else if (op != 'M') return false;
        prev = op;
    }
    return cost == distance;
}

/* Furthest-reaching points per (score, diagonal): the plain textbook formulation (the span grows by one diagonal per
 * side and score, nothing is trimmed, three score-indexed tables) so that it shares nothing with the kernels it
 * checks.  Storage is a ring of depth max(x, o+e)+1 rows per table over columns k + plen + 1, kept in a scratch the
 * caller owns (one per worker) that is grown, never freed per pair, and never bulk-filled: spans only grow, so a ring slot is always
 * reused by a WIDER row, and the only cells a read can reach that the slot's current row has not written are columns
 * that entered the span after the slot's previous (narrower) row was written -- those are set to NONE in every slot
 * of the ring at the moment they enter (two columns per score). */
void verification_scratch_free(verification_scratch_t* sc) {
    if (!sc) return;
    free(sc->buf);
    sc->buf = NULL; sc->cap = 0;
}

int verification_cpu_score(const char* pattern, const char* text, size_t plen, size_t tlen, int x, int o, int e) {
    verification_scratch_t sc = {NULL, 0};
    const int s = verification_cpu_score_scratch(pattern, text, plen, tlen, x, o, e, &sc);
    verification_scratch_free(&sc);
    return s;
}

int verification_cpu_score_scratch(const char* pattern, const char* text, size_t plen_, size_t tlen_,
                                   int x, int o, int e, verification_scratch_t* sc) {
    const int plen = (int)plen_, tlen = (int)tlen_;
    const int W = plen + tlen + 5, K0 = plen + 2;
    const int NONE = -(1 << 28);
    const int oe = o + e;
    const int depth = (x > oe ? x : oe) + 1;
    const size_t need = (size_t)W * 3 * (size_t)depth;
    if (!sc) return -1;
    if (need > sc->cap) {
        free(sc->buf);
        sc->cap = need + need / 4;
        sc->buf = (int*)malloc(sizeof(int) * sc->cap);
        if (!sc->buf) { sc->cap = 0; return -1; }
    }
    int* M = sc->buf; int* I = M + (size_t)W * depth; int* D = I + (size_t)W * depth;
    const int kend = tlen - plen;
    /* columns -1, 0, 1 of every slot: the span of score 0 and its guards */
    for (int r = 0; r < depth; ++r)
        for (int k = -1; k <= 1; ++k) { M[(size_t)r * W + K0 + k] = NONE; I[(size_t)r * W + K0 + k] = NONE; D[(size_t)r * W + K0 + k] = NONE; }
    {
        int h = 0;
        while (h < plen && h < tlen && pattern[h] == text[h]) ++h;
        M[K0] = h;
        if (kend == 0 && h >= tlen) return 0;
    }
    int lo = 0, hi = 0;     /* diagonal span that can be non-empty at the current score */
    int s;
    for (s = 1;; ++s) {
        int* Ms = M + (size_t)(s % depth) * W; int* Is = I + (size_t)(s % depth) * W; int* Ds = D + (size_t)(s % depth) * W;
        const int* Mx = s >= x ? M + (size_t)((s - x) % depth) * W : NULL;
        const int* Mo = s >= oe ? M + (size_t)((s - oe) % depth) * W : NULL;
        const int* Ie = s >= e ? I + (size_t)((s - e) % depth) * W : NULL;
        const int* De = s >= e ? D + (size_t)((s - e) % depth) * W : NULL;
        if (lo > -plen) {
            --lo;
            for (int r = 0; r < depth; ++r) { M[(size_t)r * W + K0 + lo - 1] = NONE; I[(size_t)r * W + K0 + lo - 1] = NONE; D[(size_t)r * W + K0 + lo - 1] = NONE; }
        }
        if (hi < tlen) {
            ++hi;
            for (int r = 0; r < depth; ++r) { M[(size_t)r * W + K0 + hi + 1] = NONE; I[(size_t)r * W + K0 + hi + 1] = NONE; D[(size_t)r * W + K0 + hi + 1] = NONE; }
        }
        for (int k = lo; k <= hi; ++k) {
            int ins = NONE, del = NONE, mis = NONE;
            if (Mo && Mo[K0 + k - 1] > ins) ins = Mo[K0 + k - 1];
            if (Ie && Ie[K0 + k - 1] > ins) ins = Ie[K0 + k - 1];
            if (ins >= 0) ++ins;
            if (Mo && Mo[K0 + k + 1] > del) del = Mo[K0 + k + 1];
            if (De && De[K0 + k + 1] > del) del = De[K0 + k + 1];
            if (Mx && Mx[K0 + k] >= 0) mis = Mx[K0 + k] + 1;
            if (ins >= 0 && (ins > tlen || ins - k > plen)) ins = NONE;
            if (del >= 0 && (del > tlen || del - k > plen)) del = NONE;
            if (mis >= 0 && (mis > tlen || mis - k > plen)) mis = NONE;
            Is[K0 + k] = ins; Ds[K0 + k] = del;
            int m = mis > ins ? mis : ins; if (del > m) m = del;
            if (m >= 0) {
                int h = m, v = m - k;
                while (v < plen && h < tlen && pattern[v] == text[h]) { ++v; ++h; }
                m = h;
            }
            Ms[K0 + k] = m;
        }
        if (kend >= lo && kend <= hi && Ms[K0 + kend] >= tlen) break;
    }
    return s;
}

/* ---- ends-free (see verification.h) ---- */
static void clamp_span(const int* span, int plen, int tlen, int* pb, int* pe, int* tb, int* te) {
    *pb = *pe = *tb = *te = 0;
    if (!span) return;
    *pb = span[0] < plen ? span[0] : plen; *pe = span[1] < plen ? span[1] : plen;
    *tb = span[2] < tlen ? span[2] : tlen; *te = span[3] < tlen ? span[3] : tlen;
    if (*pb < 0) *pb = 0;
    if (*pe < 0) *pe = 0;
    if (*tb < 0) *tb = 0;
    if (*te < 0) *te = 0;
}

bool check_affine_distance_span(const char* text, const char* pattern, size_t tlen, size_t plen,
                                int distance, int x, int o, int e, const char* cigar, const int* span) {
    (void)text; (void)pattern;
    int pb, pe, tb, te;
    clamp_span(span, (int)plen, (int)tlen, &pb, &pe, &tb, &te);
    /* items first: the last one is only known at the end */
    size_t n_items = 0;
    for (const char* c = cigar; *c;) { long n; char op; c = next_item(c, &n, &op); if (!c) return false; ++n_items; }
    long cost = 0;
    char prev = 0;
    size_t idx = 0;
    const char* c = cigar;
    while (*c) {
        long n = 0; char op = 0;
        c = next_item(c, &n, &op);      /* (well-formed: checked above) */
        if (op == 'I' || op == 'D') {
            long paid = n;
            if (idx == 0) { const long f = op == 'I' ? tb : pb; paid -= f < paid ? f : paid; }
            if (idx + 1 == n_items) { const long f = op == 'I' ? te : pe; paid -= f < paid ? f : paid; }
            if (paid > 0) cost += (prev == op ? 0 : o) + paid * e;
        } else if (op == 'X') cost += n * x;
        else if (op != 'M') return false;
        prev = op;
        ++idx;
    }
    return cost == distance;
}

int verification_cpu_score_span(const char* pattern, const char* text, size_t plen, size_t tlen, int x, int o, int e, const int* span) {
    verification_scratch_t sc = {NULL, 0};
    const int s = verification_cpu_score_span_scratch(pattern, text, plen, tlen, x, o, e, span, &sc);
    verification_scratch_free(&sc);
    return s;
}

/* The program of verification_cpu_score_scratch with free borders: score 0 holds every diagonal of [-pbf, tbf] at offset
 * max(k, 0); the alignment ends with the first score one of whose M cells has used up the text with at most pef pattern
 * bases left, or the pattern with at most tef text bases left. */
int verification_cpu_score_span_scratch(const char* pattern, const char* text, size_t plen_, size_t tlen_,
                                        int x, int o, int e, const int* span, verification_scratch_t* sc) {
    const int plen = (int)plen_, tlen = (int)tlen_;
    int pbf, pef, tbf, tef;
    clamp_span(span, plen, tlen, &pbf, &pef, &tbf, &tef);
    const int W = plen + tlen + 5, K0 = plen + 2;
    const int NONE = -(1 << 28);
    const int oe = o + e;
    const int depth = (x > oe ? x : oe) + 1;
    const size_t need = (size_t)W * 3 * (size_t)depth;
    if (!sc) return -1;
    if (need > sc->cap) {
        free(sc->buf);
        sc->cap = need + need / 4;
        sc->buf = (int*)malloc(sizeof(int) * sc->cap);
        if (!sc->buf) { sc->cap = 0; return -1; }
    }
    int* M = sc->buf; int* I = M + (size_t)W * depth; int* D = I + (size_t)W * depth;
    int lo = -pbf, hi = tbf;     /* diagonal span that can be non-empty at the current score */
    /* the span of score 0 and its guards, in every slot */
    for (int r = 0; r < depth; ++r)
        for (int k = lo - 1; k <= hi + 1; ++k) { M[(size_t)r * W + K0 + k] = NONE; I[(size_t)r * W + K0 + k] = NONE; D[(size_t)r * W + K0 + k] = NONE; }
    for (int k = lo; k <= hi; ++k) {
        int h = k > 0 ? k : 0, v = h - k;
        while (v < plen && h < tlen && pattern[v] == text[h]) { ++v; ++h; }
        M[K0 + k] = h;
        if ((h >= tlen && plen - v <= pef) || (v >= plen && tlen - h <= tef)) return 0;
    }
    int s;
    for (s = 1;; ++s) {
        int* Ms = M + (size_t)(s % depth) * W; int* Is = I + (size_t)(s % depth) * W; int* Ds = D + (size_t)(s % depth) * W;
        const int* Mx = s >= x ? M + (size_t)((s - x) % depth) * W : NULL;
        const int* Mo = s >= oe ? M + (size_t)((s - oe) % depth) * W : NULL;
        const int* Ie = s >= e ? I + (size_t)((s - e) % depth) * W : NULL;
        const int* De = s >= e ? D + (size_t)((s - e) % depth) * W : NULL;
        if (lo > -plen) {
            --lo;
            for (int r = 0; r < depth; ++r) { M[(size_t)r * W + K0 + lo - 1] = NONE; I[(size_t)r * W + K0 + lo - 1] = NONE; D[(size_t)r * W + K0 + lo - 1] = NONE; }
        }
        if (hi < tlen) {
            ++hi;
            for (int r = 0; r < depth; ++r) { M[(size_t)r * W + K0 + hi + 1] = NONE; I[(size_t)r * W + K0 + hi + 1] = NONE; D[(size_t)r * W + K0 + hi + 1] = NONE; }
        }
        bool ended = false;
        for (int k = lo; k <= hi; ++k) {
            int ins = NONE, del = NONE, mis = NONE;
            if (Mo && Mo[K0 + k - 1] > ins) ins = Mo[K0 + k - 1];
            if (Ie && Ie[K0 + k - 1] > ins) ins = Ie[K0 + k - 1];
            if (ins >= 0) ++ins;
            if (Mo && Mo[K0 + k + 1] > del) del = Mo[K0 + k + 1];
            if (De && De[K0 + k + 1] > del) del = De[K0 + k + 1];
            if (Mx && Mx[K0 + k] >= 0) mis = Mx[K0 + k] + 1;
            if (ins >= 0 && (ins > tlen || ins - k > plen)) ins = NONE;
            if (del >= 0 && (del > tlen || del - k > plen)) del = NONE;
            if (mis >= 0 && (mis > tlen || mis - k > plen)) mis = NONE;
            Is[K0 + k] = ins; Ds[K0 + k] = del;
            int m = mis > ins ? mis : ins; if (del > m) m = del;
            if (m >= 0) {
                int h = m, v = m - k;
                while (v < plen && h < tlen && pattern[v] == text[h]) { ++v; ++h; }
                m = h;
                if ((h >= tlen && plen - v <= pef) || (v >= plen && tlen - h <= tef)) ended = true;
            }
            Ms[K0 + k] = m;
        }
        if (ended) break;
    }
    return s;
}

/* ---- two-piece gap-affine (see verification.h) ---- */
static long gap2p_cost(long n, int o1, int e1, int o2, int e2) {
    const long a = o1 + n * e1, b = o2 + n * e2;
    return a < b ? a : b;
}

bool check_affine2p_distance(const char* text, const char* pattern, size_t tlen, size_t plen,
                             int distance, int x, int o1, int e1, int o2, int e2, const char* cigar) {
    (void)text; (void)pattern; (void)tlen; (void)plen;
    long cost = 0, gap = 0;     /* gap: bases of the I / D run that is open */
    char prev = 0;
    const char* c = cigar;
    while (*c) {
        long n; char op;
        c = next_item(c, &n, &op);
        if (!c) return false;
        if (op != 'M' && op != 'X' && op != 'I' && op != 'D') return false;
        /* a run ends where the operation changes: priced as a whole, by the cheaper piece */
        if (op != prev && gap) { cost += gap2p_cost(gap, o1, e1, o2, e2); gap = 0; }
        if (op == 'X') cost += n * x;
        else if (op == 'I' || op == 'D') gap += n;
        prev = op;
    }
    if (gap) cost += gap2p_cost(gap, o1, e1, o2, e2);
    return cost == distance;
}

int verification_cpu_score_2p(const char* pattern, const char* text, size_t plen, size_t tlen, int x, int o1, int e1, int o2, int e2) {
    verification_scratch_t sc = {NULL, 0};
    const int s = verification_cpu_score_2p_scratch(pattern, text, plen, tlen, x, o1, e1, o2, e2, &sc);
    verification_scratch_free(&sc);
    return s;
}

/* The program of verification_cpu_score_scratch with five score-indexed tables: M, and I / D once per piece. */
int verification_cpu_score_2p_scratch(const char* pattern, const char* text, size_t plen_, size_t tlen_,
                                      int x, int o1, int e1, int o2, int e2, verification_scratch_t* sc) {
    const int plen = (int)plen_, tlen = (int)tlen_;
    const int W = plen + tlen + 5, K0 = plen + 2;
    const int NONE = -(1 << 28);
    const int oe[2] = {o1 + e1, o2 + e2}, ex[2] = {e1, e2};
    int depth = x;
    if (oe[0] > depth) depth = oe[0];
    if (oe[1] > depth) depth = oe[1];
    ++depth;
    const size_t need = (size_t)W * 5 * (size_t)depth;
    if (!sc) return -1;
    if (need > sc->cap) {
        free(sc->buf);
        sc->cap = need + need / 4;
        sc->buf = (int*)malloc(sizeof(int) * sc->cap);
        if (!sc->buf) { sc->cap = 0; return -1; }
    }
    int* T[5];      /* M, I1, D1, I2, D2 */
    for (int t = 0; t < 5; ++t) T[t] = sc->buf + (size_t)t * W * depth;
    const int kend = tlen - plen;
    for (int t = 0; t < 5; ++t)
        for (int r = 0; r < depth; ++r)
            for (int k = -1; k <= 1; ++k) T[t][(size_t)r * W + K0 + k] = NONE;
    {
        int h = 0;
        while (h < plen && h < tlen && pattern[h] == text[h]) ++h;
        T[0][K0] = h;
        if (kend == 0 && h >= tlen) return 0;
    }
    int lo = 0, hi = 0;
    int s;
    for (s = 1;; ++s) {
        const size_t row = (size_t)(s % depth) * W;
        const int* Mx = s >= x ? T[0] + (size_t)((s - x) % depth) * W : NULL;
        if (lo > -plen) {
            --lo;
            for (int t = 0; t < 5; ++t) for (int r = 0; r < depth; ++r) T[t][(size_t)r * W + K0 + lo - 1] = NONE;
        }
        if (hi < tlen) {
            ++hi;
            for (int t = 0; t < 5; ++t) for (int r = 0; r < depth; ++r) T[t][(size_t)r * W + K0 + hi + 1] = NONE;
        }
        for (int k = lo; k <= hi; ++k) {
            int m = NONE;
            if (Mx && Mx[K0 + k] >= 0) m = Mx[K0 + k] + 1;
            if (m >= 0 && (m > tlen || m - k > plen)) m = NONE;
            for (int pc = 0; pc < 2; ++pc) {
                const int* Mo = s >= oe[pc] ? T[0] + (size_t)((s - oe[pc]) % depth) * W : NULL;
                const int* Ie = s >= ex[pc] ? T[1 + 2 * pc] + (size_t)((s - ex[pc]) % depth) * W : NULL;
                const int* De = s >= ex[pc] ? T[2 + 2 * pc] + (size_t)((s - ex[pc]) % depth) * W : NULL;
                int ins = NONE, del = NONE;
                if (Mo && Mo[K0 + k - 1] > ins) ins = Mo[K0 + k - 1];
                if (Ie && Ie[K0 + k - 1] > ins) ins = Ie[K0 + k - 1];
                if (ins >= 0) ++ins;
                if (Mo && Mo[K0 + k + 1] > del) del = Mo[K0 + k + 1];
                if (De && De[K0 + k + 1] > del) del = De[K0 + k + 1];
                if (ins >= 0 && (ins > tlen || ins - k > plen)) ins = NONE;
                if (del >= 0 && (del > tlen || del - k > plen)) del = NONE;
                T[1 + 2 * pc][row + K0 + k] = ins; T[2 + 2 * pc][row + K0 + k] = del;
                if (ins > m) m = ins;
                if (del > m) m = del;
            }
            if (m >= 0) {
                int h = m, v = m - k;
                while (v < plen && h < tlen && pattern[v] == text[h]) { ++v; ++h; }
                m = h;
            }
            T[0][row + K0 + k] = m;
        }
        if (kend >= lo && kend <= hi && T[0][row + K0 + kend] >= tlen) break;
    }
    return s;
}

int verification_heuristic_verdict(int distance, int optimum) {
    if (distance < optimum) return -1;
    return distance - optimum;
}

/* Edit, indel and gap-linear distances (wfagpu_amd_linear_t): metric 0 indel, 1 edit, 2 gap-linear (x, g). */
static bool linear_pens(int metric, int* x, int* g) {
    if (metric == 1) { *x = 1; *g = 1; return true; }
    if (metric == 0) { *x = 0; *g = 1; return true; }      /* (x = 0: no mismatch move) */
    return metric == 2 && *x > 0 && *g > 0;
}

bool check_linear_distance(const char* text, const char* pattern, size_t tlen, size_t plen,
                           int distance, int metric, int x, int g, const char* cigar) {
    (void)text; (void)pattern; (void)tlen; (void)plen;
    if (!linear_pens(metric, &x, &g)) return false;
    long cost = 0;
    const char* c = cigar;
    while (*c) {
        long n; char op;
        c = next_item(c, &n, &op);
        if (!c) return false;
        if (op == 'X') { if (x == 0) return false; cost += n * x; }      /* (indel: an X is a failure) */
        else if (op == 'I' || op == 'D') cost += n * g;
        else if (op != 'M') return false;
    }
    return cost == distance;
}

/* Furthest-reaching points per (score, diagonal) in ONE table: a ring of max(x, g) + 1 rows over every diagonal of the pair, each
 * row written whole (NONE outside the span of its score).  O(score * (plen + tlen)): a checker, plain on purpose. */
int verification_cpu_score_linear(const char* pattern, const char* text, size_t plen_, size_t tlen_, int metric, int x, int g) {
    if (!linear_pens(metric, &x, &g)) return -1;
    const int plen = (int)plen_, tlen = (int)tlen_, kend = tlen - plen;
    const int W = plen + tlen + 3, K0 = plen + 1, depth = (x > g ? x : g) + 1, NONE = -(1 << 29);
    int* rows = (int*)malloc((size_t)depth * W * sizeof(int));
    if (!rows) return -1;
    for (long i = 0; i < (long)depth * W; ++i) rows[i] = NONE;
    int h0 = 0;
    while (h0 < plen && h0 < tlen && pattern[h0] == text[h0]) ++h0;
    rows[K0] = h0;
    int s = 0;
    const long worst = (long)2 * g * (plen < tlen ? plen : tlen) + (long)g * (kend < 0 ? -kend : kend);
    while (rows[(size_t)(s % depth) * W + K0 + kend] < tlen) {
        ++s;
        if (s > worst) { s = -1; break; }
        int* cur = rows + (size_t)(s % depth) * W;
        const int* rg = s >= g ? rows + (size_t)((s - g) % depth) * W : NULL;
        const int* rx = (x > 0 && s >= x) ? rows + (size_t)((s - x) % depth) * W : NULL;
        for (int k = -plen; k <= tlen; ++k) {
            int best = NONE;
            if (rx && rx[K0 + k] + 1 > best) best = rx[K0 + k] + 1;
            if (rg && rg[K0 + k - 1] + 1 > best) best = rg[K0 + k - 1] + 1;
            if (rg && rg[K0 + k + 1] > best) best = rg[K0 + k + 1];
            int h = best, v = best - k;
            if (h < 0 || v < 0 || h > tlen || v > plen) { cur[K0 + k] = NONE; continue; }
            while (h < tlen && v < plen && pattern[v] == text[h]) { ++h; ++v; }
            cur[K0 + k] = h;
        }
    }
    free(rows);
    return s;
}

/* ---- a one-component metric under an ends-free span (see verification.h) ---- */
bool check_linear_distance_span(const char* text, const char* pattern, size_t tlen, size_t plen,
                                int distance, int metric, int x, int g, const char* cigar, const int* span) {
    (void)text; (void)pattern;
    if (!linear_pens(metric, &x, &g)) return false;
    int pb, pe, tb, te;
    clamp_span(span, (int)plen, (int)tlen, &pb, &pe, &tb, &te);
    /* items first: the last one is only known at the end */
    size_t n_items = 0;
    for (const char* c = cigar; *c;) { long n; char op; c = next_item(c, &n, &op); if (!c) return false; ++n_items; }
    long cost = 0;
    size_t idx = 0;
    const char* c = cigar;
    while (*c) {
        long n = 0; char op = 0;
        c = next_item(c, &n, &op);      /* (well-formed: checked above) */
        if (op == 'I' || op == 'D') {
            long paid = n;
            if (idx == 0) { const long f = op == 'I' ? tb : pb; paid -= f < paid ? f : paid; }
            if (idx + 1 == n_items) { const long f = op == 'I' ? te : pe; paid -= f < paid ? f : paid; }
            cost += paid * g;
        } else if (op == 'X') { if (x == 0) return false; cost += n * x; }      /* (indel: an X is a failure) */
        else if (op != 'M') return false;
        ++idx;
    }
    return cost == distance;
}

/* The program of verification_cpu_score_linear with free borders: score 0 holds every diagonal of [-pbf, tbf] at offset max(k, 0);
 * the alignment ends with the first score one of whose cells has used up the text with at most pef pattern bases left, or the
 * pattern with at most tef text bases left. */
int verification_cpu_score_linear_span(const char* pattern, const char* text, size_t plen_, size_t tlen_, int metric, int x, int g, const int* span) {
    if (!linear_pens(metric, &x, &g)) return -1;
    const int plen = (int)plen_, tlen = (int)tlen_, kend = tlen - plen;
    int pbf, pef, tbf, tef;
    clamp_span(span, plen, tlen, &pbf, &pef, &tbf, &tef);
    const int W = plen + tlen + 3, K0 = plen + 1, depth = (x > g ? x : g) + 1, NONE = -(1 << 29);
    int* rows = (int*)malloc((size_t)depth * W * sizeof(int));
    if (!rows) return -1;
    for (long i = 0; i < (long)depth * W; ++i) rows[i] = NONE;
    bool ended = false;
    for (int k = -pbf; k <= tbf; ++k) {
        int h = k > 0 ? k : 0, v = h - k;
        while (h < tlen && v < plen && pattern[v] == text[h]) { ++h; ++v; }
        rows[K0 + k] = h;
        if ((h >= tlen && plen - v <= pef) || (v >= plen && tlen - h <= tef)) ended = true;
    }
    int s = 0;
    /* (the end-to-end alignment is a candidate: no ends-free one costs more) */
    const long worst = (long)2 * g * (plen < tlen ? plen : tlen) + (long)g * (kend < 0 ? -kend : kend);
    while (!ended) {
        ++s;
        if (s > worst) { s = -1; break; }
        int* cur = rows + (size_t)(s % depth) * W;
        const int* rg = s >= g ? rows + (size_t)((s - g) % depth) * W : NULL;
        const int* rx = (x > 0 && s >= x) ? rows + (size_t)((s - x) % depth) * W : NULL;
        for (int k = -plen; k <= tlen; ++k) {
            int best = NONE;
            if (rx && rx[K0 + k] + 1 > best) best = rx[K0 + k] + 1;
            if (rg && rg[K0 + k - 1] + 1 > best) best = rg[K0 + k - 1] + 1;
            if (rg && rg[K0 + k + 1] > best) best = rg[K0 + k + 1];
            int h = best, v = best - k;
            if (h < 0 || v < 0 || h > tlen || v > plen) { cur[K0 + k] = NONE; continue; }
            while (h < tlen && v < plen && pattern[v] == text[h]) { ++h; ++v; }
            cur[K0 + k] = h;
            if ((h >= tlen && plen - v <= pef) || (v >= plen && tlen - h <= tef)) ended = true;
        }
    }
    free(rows);
    return s;
}
