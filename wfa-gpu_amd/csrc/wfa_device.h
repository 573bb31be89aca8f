// Shared device/host definitions for the gfx950 WFA kernels.
//
// Data layout in HBM (see DESIGN.md "Data layout"):
//   * ASCII input:   the reference's padded buffer + 48-byte sequence_pair_t
//                    records (utils/sequences.h:28-36 of the reference).
//   * Packed input:  2 bits/base, code=(c&6)>>1, 16 bases per 32-bit word,
//                    base i of a sequence in bits [2*(i%16)+1 : 2*(i%16)]
//                    (little-endian inside the word so one v_alignbit_b32
//                    yields the 16 bases starting at any position).
//   * Backtrace arena: one origin byte per wavefront cell, bump-allocated in
//                    16-byte units.  Two layouts, told apart by the first word
//                    of a pair's block (bt_final_row[pair]):
//                    - TILES (the one-wave exact tier, round 6): 64-byte header
//                      {WFA_ROW_NONE, wlo, tile columns, budget}, then 64-byte
//                      tiles of 4 scores x 16 diagonals at a fixed pitch: tile
//                      (s >> 2, (k - wlo) >> 4), byte (s & 3) * 16 + ((k - wlo) & 15);
//                    - ROWS (every other tier): a row table [score] = {unit of
//                      the row, lo} (8 bytes per score) and one row of origin
//                      bytes per score, byte j = diagonal lo + j.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

// Mirror of the reference ABI struct sequence_pair_t (utils/sequences.h:28-36).
struct WfaSeqPair {
  size_t text_offset;
  size_t pattern_offset;
  size_t text_offset_packed;
  size_t pattern_offset_packed;
  unsigned int text_len;
  unsigned int pattern_len;
  bool has_N;
};
static_assert(sizeof(WfaSeqPair) == 48, "sequence_pair_t ABI");

// Per-pair status written by the align kernels.
enum : uint32_t {
  WFA_ST_PENDING = 0,    // not processed yet
  WFA_ST_DONE = 1,       // score (and backtrace rows) valid
  WFA_ST_BAND = 2,       // wavefront left the tier's diagonal capacity -> next tier
  WFA_ST_SCORE = 3,      // score went past the tier's score limit        -> next tier
  WFA_ST_NOMEM = 4,      // backtrace arena exhausted                     -> next sub-batch
  WFA_ST_ALPHABET = 5,   // pair holds bytes outside ACGT                 -> byte-compare tier
};

// Origin byte per wavefront cell (what the backtrace needs, 4 bits used):
//   bits 3:2  source of M : 0 none (cell not valid), 3 mismatch, 2 deletion, 1 insertion  (WFA2's priority on equal
//             offsets, wavefront_backtrace.c:48-59: the lean kernel path gets it from ONE signed max over
//             offset << 16 | these bits)
//   bit  1    D came from D (gap extension) rather than from M (gap open)
//   bit  0    I came from I (gap extension) rather than from M (gap open)
enum : uint32_t { BT_M_NONE = 0, BT_M_X = 12, BT_M_D = 8, BT_M_I = 4, BT_M_MASK = 12, BT_D_EXT = 2, BT_I_EXT = 1 };
// Two-piece gap-affine (the TWOPIECE instantiations, align_kernel_2p.hip), 7 bits used:
//   bits 6:4  source of M : 0 none, then by WFA2's priority on equal offsets (wavefront_backtrace.c:49-59: mismatch, D2, D1, I2, I1)
//   bit  3    D2 came from D2 (extension won, or tied, against opening)      bit 2    I2 came from I2
//   bit  1    D1 came from D1                                                bit 0    I1 came from I1
enum : uint32_t { BT2_M_NONE = 0, BT2_M_X = 5u << 4, BT2_M_D2 = 4u << 4, BT2_M_D1 = 3u << 4, BT2_M_I2 = 2u << 4, BT2_M_I1 = 1u << 4, BT2_M_MASK = 7u << 4,
                  BT2_D2_EXT = 8, BT2_I2_EXT = 4, BT2_D1_EXT = 2, BT2_I1_EXT = 1 };

// Edit, indel and gap-linear distances (the LINEAR instantiations, align_kernel_lin.hip): one component, 2 bits used -- the source of M,
// by WFA2's priority on equal offsets (wavefront_backtrace.c:49-59, 259-264: mismatch, deletion, insertion; never a mismatch under indel)
enum : uint32_t { BTL_NONE = 0, BTL_X = 3, BTL_D = 2, BTL_I = 1, BTL_MASK = 3 };

// Two-piece gap cost and what a budget affords (host and device).  A gap of n bases costs g(n) = min(o1 + n e1, o2 + n e2), g(0) = 0;
// g is increasing, concave and subadditive (g(a) + g(b) >= g(a + b)): several gaps never cost less than one gap of their bases.
// (oe1 = o1 + e1, oe2 = o2 + e2, as the kernels carry them)
__host__ __device__ inline long long wfa_gap2p(const long long n, const int oe1, const int e1, const int oe2, const int e2) {
  if (n <= 0) return 0;
  const long long a = oe1 + (n - 1) * e1, b = oe2 + (n - 1) * e2;
  return a < b ? a : b;
}
// R(S): the longest gap a budget S pays for (0: none)
__host__ __device__ inline long long wfa_reach2p(const long long S, const int oe1, const int e1, const int oe2, const int e2) {
  const long long a = S >= oe1 ? (S - oe1) / e1 + 1 : 0, b = S >= oe2 ? (S - oe2) / e2 + 1 : 0;
  return a > b ? a : b;
}
// The largest t with g(t) + g(t + ak) <= S: how far beyond both its end diagonals (ak apart) a path of cost <= S can stray -- it
// needs a gap of t + ak bases out and one of t back, or more gaps of no fewer bases.  (g(ak) <= S assumed: t = 0 qualifies.)
__host__ __device__ inline int wfa_stray2p(const long long S, const long long ak, const int oe1, const int e1, const int oe2, const int e2) {
  long long lo = 0, hi = wfa_reach2p(S / 2, oe1, e1, oe2, e2);      // (2 g(t) <= S bounds it)
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (wfa_gap2p(mid, oe1, e1, oe2, e2) + wfa_gap2p(mid + ak, oe1, e1, oe2, e2) <= S) lo = mid; else hi = mid - 1;
  }
  return (int)lo;
}

// Operations of a reversed op list (what the backward walk leaves for the replay): the kind, and whether a run of matches
// follows the operation (re-derived by the replay as a longest common prefix).
enum : uint8_t { OP_X = 1, OP_I = 2, OP_D = 3, OP_EXT_AFTER = 0x10 };

// First word of a pair's block in the arena: this value marks the TILES layout; anything else is entry 0 of a ROWS row table.  The
// marker is in band, its one reader (bt_block, trace_kernel.hip) relies on two facts:
//   * every ROWS producer writes word 0 of its table (the arena unit of the row of score 0);
//   * an arena unit can never equal the marker: the arena is capped at WFA_ARENA_MAX_BYTES, its 16-byte units stay below 2^32 - 256.
#define WFA_ROW_NONE 0xFFFFFFFFu
constexpr unsigned long long WFA_ARENA_MAX_BYTES = (1ull << 36) - 4096;
static_assert(WFA_ARENA_MAX_BYTES / 16 < WFA_ROW_NONE, "a row unit must never read as the TILES marker");
// The lean cells of the banded search never switch a lane off: the lanes of a row's last 64-diagonal
// chunk that lie beyond its upper limit store NULL offsets into that many cells behind the row (every ring row carries
// WFA_RING_ROW_PAD extra cells for it) and origin bytes behind the row's bytes in the arena (every arena chunk keeps
// WFA_ARENA_ROW_SLACK 16-byte units unallocated at its end; the arena itself ends with 8 spare units).  The exact lean loops
// store that chunk under its lane mask (align/cells_hot.inc, MASKED_LAST) and write nothing beyond a row; pad and slack stay.
#define WFA_RING_ROW_PAD 64
#define WFA_ARENA_ROW_SLACK 4u

// Backtrace arena, 16-byte units.  Per alignment: a block of tiles, or a row table [score] = {unit of the row, lo} (8 bytes
// per score up to the score budget) followed, wherever the block's bump allocator puts them, by one
// row of origin bytes per score (byte j = diagonal lo + j): the two layouts at the top of this file.
struct WfaAlignParams {
  const uint32_t* packed;        // packed sequences (word base); RAW kernels: the ASCII buffer
  const char* ascii;             // non-null (packed kernels only): the sequences are still ASCII -- pack them while they are staged: the words go
                                 // to LDS and to `packed` (for the backtrace kernels); a pair with a byte outside ACGT leaves with status
                                 // ALPHABET (counted in *n_raw) and is aligned by the byte-compare class afterwards
  unsigned long long* n_raw;
  const WfaSeqPair* meta;
  const uint32_t* work;          // pair indices to process (NULL: identity)
  uint32_t n_work;
  const unsigned long long* n_work_dev;   // optional: the list's real length lives on the device (a list compacted by the launch
                                          // before, not read back by the host yet); n_work is then an upper bound
  int only_pending;              // 1: skip pairs whose status is not PENDING (an unfiltered list: pairs flagged for the byte-compare class)
  unsigned int* work_counter;    // dynamic work distribution: 8 counters, 64 bytes apart (zeroed before launch)
  uint32_t work_shards;          // 1 or 8 of them in use
  int x, oe, e;                  // penalties: mismatch, open+extend, extend
  int dm, de;                    // ring depths: max(x,oe)+1 rows of M, e+1 rows of I and D
  int book_mask;                 // row-book entries - 1 (power of two >= max(dm, 64))
  int rs;                        // row stride (elements), even: widest diagonal window + 3
  int max_score;                 // give up (WFA_ST_SCORE) beyond this score
  const int32_t* budget;         // optional per-pair score budget (auto-tuned), capped by max_score
  int budget_q, budget_slack, budget_margin;   // tier 5 only, budget == NULL, budget_q > 0: the per-pair budget by k_budget's rule (wfa_host.hip), computed in the
                                 // kernel: (q * longer length * margin / 100) / 1024 + slack -- no launch to fill the array in front of the call's only wavefront launch
  int band_width;                // > 0: adaptive band, diagonals kept per wavefront (banded kernels)
  int band_period;               //      re-centre the band every this many scores
  int seq_words_cap;             // LDS words reserved per packed sequence
  int no_lean;                   // diagnostics (WFAGPU_NO_LEAN): keep every score on the careful path
  int32_t* score;                // [pair] out
  uint32_t* status;              // [pair] out
  uint32_t* cells;               // [pair] out, optional: number of wavefront cells computed
  unsigned long long* launch_cells;  // optional: += cells computed by this launch (one atomic per workgroup)
  // tier 5 only.  wave_parts: four u64 per wavefront of the launch {cells, pairs of its share of the list that did not leave DONE, pairs
  // it appended to fail_list, pairs it flagged ALPHABET}, plain stores -- to device memory, or straight to pinned host memory --
  // (instead of the atomic on launch_cells: thousands of wavefronts ending together on one counter line).  fail_list / fail_count: the
  // kernel appends the pairs it leaves with status BAND or SCORE itself (the chain's only launch, score-only: no kernel behind it)
  unsigned long long* wave_parts;
  uint32_t* fail_list;
  unsigned long long* fail_count;
  int arena_top_known;           // tier 5 with CIGARs: 1 = the bump pointer is arena_top0_value when the launch starts (the host knows: a pass's first
  unsigned long long arena_top0_value;   // launch) -- the launch moves it past its slots itself (workgroup 0) instead of a one-thread kernel behind it
  // backtrace (CIGAR mode)
  uint8_t* arena;                // base of the arena
  unsigned long long arena_units;        // capacity in 16-byte units
  unsigned long long* arena_top;         // bump pointer (units)
  uint32_t chunk_units;          // refill granularity
  uint32_t* bt_final_row;        // [pair] out: unit offset of the pair's block of tiles / row table
  // global-memory ring (only the GLOBAL_RING instantiation)
  void* gring;                   // per-block slices of gring_stride bytes
  int ring16;                    //   16-bit offsets in it (sequences <= 32766 bases), else 32-bit
  unsigned long long gring_stride;
  // diagnostics (tuning.timed_barriers): barrier arrival / release clocks of workgroup 0, 3 x u64 per score and wave
  unsigned long long* dbg_times;
  uint32_t dbg_cap;              // records (scores) the buffer holds
  // ends-free alignment (only the ENDSFREE instantiations, align_kernel_ef.hip, read these): the span as the caller gave it -- the
  // kernel clamps each value to the pair's own sequence length -- and where the diagonal the alignment ended on goes
  int span_pbf, span_pef, span_tbf, span_tef;   // pattern begin / pattern end / text begin / text end free
  int32_t* ends;                 // [2 * pair + 1] out: end diagonal k1 ([2 * pair], the start diagonal k0, is the backtrace's; INT_MIN here)
  // two-piece gap-affine (only the TWOPIECE instantiations, align_kernel_2p.hip, read these; e2 == 0: gap-affine): the second piece as
  // open + extend and extend, e2 + 1 rows each of I2 and D2 behind the D ring.  x / oe / e / de are the first piece, dm = max(x, oe, oe2) + 1.
  int oe2, e2, de2;
  // wf-adaptive (only the ADAPTIVE instantiations, align_kernel_ad.hip, read these; ad_steps == 0: exact search): WFA2's
  // min_wavefront_length, max_distance_threshold, steps_between_cutoffs
  int ad_min_len, ad_max_dist, ad_steps;
  // (edit, indel and gap-linear distances -- the LINEAR instantiations, align_kernel_lin.hip -- add no field: mismatch x, every gap base e,
  // oe == e, de == 0 -- no I / D rows, which is how the host tells these calls apart --, dm = max(x, e) + 1 rows of M; indel, which has no
  // mismatch move, is x = WFA_LIN_NO_MISMATCH with dm = e + 1)
};
constexpr int WFA_LIN_NO_MISMATCH = 1 << 30;

struct WfaTraceParams {
  int raw;                       // 1: sequences are the ASCII buffer (byte compare), 0: 2-bit packed
  int seq_lds_stride;            // > 0: stage each lane's pair in LDS, this many (odd) words per lane
  int emit_pairs;                //      ... of the first emit_pairs lanes of a wavefront (the others idle: LDS per wavefront buys occupancy)
  const uint32_t* packed;
  const WfaSeqPair* meta;
  const uint32_t* work;          // pair indices (NULL: identity)
  uint32_t n_work;
  int x, oe, e;
  const int32_t* score;
  int32_t* score_fix;            // banded passes: scores are replaced by the cost of the emitted CIGAR where they differ
  const uint32_t* status;
  const uint8_t* arena;
  unsigned long long arena_bytes;  // size of the arena (the wave-per-alignment kernel range-checks row-table entries of scores without a wavefront)
  int wave_kernel;               // 1: one wavefront per alignment (long alignments), 0: one lane per alignment
  int group;                     // wave kernel: alignments per wavefront (1, 2, 4 or 8: 64/group lanes each, own LDS share)
  int lane_fused;                // lane-per-alignment path: walk + replay in ONE kernel, op lists of ops_lds_bytes per lane in LDS (short alignments)
  int walk_grid_cap;             // workgroups of wfa_walk_kernel (it strides over the list); 0: one per 256 list entries
  int walk_only;                 // wave kernel: only the walk (op list -> slot w of ops_slot bytes in the global scratch); wfa_emit_kernel replays
  uint32_t ops_slot;
  int seq_words_cap;             // wave kernel: LDS words reserved per sequence
  int ops_lds_bytes;             // wave kernel: LDS bytes for the op list (longer lists go through the global scratch)
  int text_lds_bytes;            // wave kernel: LDS bytes for the CIGAR text of one alignment (longer texts: second replay)
  const uint32_t* bt_final_row;
  // scratch for the reversed op list, bump allocated (bytes)
  uint8_t* ops;
  unsigned long long ops_cap;
  unsigned long long* ops_top;
  // output text arena
  char* text;
  unsigned long long text_cap;
  unsigned long long* text_top;
  // lane-per-alignment emit, single replay: texts are first written at upper-bound offsets of this scratch and then
  // compacted into `text` (NULL: two replays, the first one only to size the text)
  char* text_scratch;
  unsigned long long text_scratch_cap;
  unsigned long long* scratch_top;
  int min_op_cost;               // min(x, e) (two pieces: min(x, e1, e2)): an alignment of score s has at most s / min_op_cost operations
  int item_chars;                // widest RLE item (digits of the longest sequence + 1): sizes the upper-bound text slots
  unsigned long long* cigar_off; // [pair] out: byte offset of the CIGAR in `text` (between walk and replay: of the op list in `ops`)
  uint32_t* cigar_len;           // [pair] out: strlen; 0xFFFFFFFF if it did not fit
  // ends-free alignment.  ends == nullptr (and a span of zeros): end to end -- every walk starts on diagonal tlen - plen and ends on 0.
  // Else ends[2 * pair + 1] is the diagonal k1 the walk starts on (written by the wavefront kernel), the walk may end on any diagonal
  // k0 of [-min(span_pbf, plen), min(span_tbf, tlen)] and leaves it in ends[2 * pair]; the replay starts at (max(-k0, 0), max(k0, 0)),
  // prints the free bases in front of and behind the path as D / I runs and prices the text without them.
  int span_pbf, span_tbf;
  int32_t* ends;
  int extra_items;               // RLE items a text may have beyond 2 * operations + 1 (the two free runs): sizes the upper-bound text slots
  int oe2, e2;                   // two-piece gap-affine (wfa_launch_trace_2p only): the second piece; origin bytes are BT2_*
  // (wfa_launch_trace_lin: oe == e is the cost of a gap base, origin bytes are BTL_*)
};

// Host-side launchers (one per translation unit).
// Timed launches.  hipEventRecord puts a barrier packet of its own into the queue, and a kernel behind one starts ~5.5 us after the
// kernel in front of it has finished (back to back: 0.2 us): nine records per call were 35 of the 250 us of a BASELINE configs[1]
// step.  hipExtLaunchKernelGGL lets the kernel's own dispatch packet carry the time stamps: ev0 becomes the start of the kernel,
// ev1 its end (either may be null; hipEventElapsedTime pairs them freely, also with recorded events: scratch/ext_event_probe.hip).
template <typename K, typename... Args>
inline void wfa_launch_timed(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, Args... args) {
  if (ev0 || ev1) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, ev0, ev1, 0, args...);
  else hipLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, args...);
}

// (ev0 / ev1 of every launcher: events that receive the start of the first and the end of the last kernel it launches)
void wfa_launch_pack(const char* d_ascii, const WfaSeqPair* d_meta, uint32_t n_pairs,
                     uint32_t* d_packed, uint8_t* d_flags, hipStream_t stream, uint32_t max_seq_len = 0,
                     hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                     uint32_t* d_status = nullptr, unsigned long long* d_n_raw = nullptr);      // (d_status: flagged pairs get WFA_ST_ALPHABET and are counted in *d_n_raw)
// tier: 0 -> 1 wave/alignment (LDS ring), 1 -> 4 waves (LDS), 2 -> 16 waves (LDS), 4 -> 16 waves, M and I rings in LDS + D ring in HBM,
//       3 -> 16 waves, ring in HBM (int16 or int32 offsets, WfaAlignParams::ring16).  Returns the dynamic LDS bytes used.
size_t wfa_align_lds_bytes(const WfaAlignParams& p, int tier);
// wpe: waves per SIMD the one-wave exact kernels (tier 0, packed class) are compiled for: 8, 7, 6 or 4 (others: 8).
void wfa_launch_align(const WfaAlignParams& p, int tier, bool with_bt, bool raw, int grid, hipStream_t stream, int wpe = 8,
                      hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int wfa_align_max_blocks_per_cu(int tier, bool with_bt, bool raw, bool banded, size_t lds_bytes, int wpe = 8);
// The ends-free instantiations of the wavefront kernel (align_kernel_ef.hip: a translation unit and code object of their own, loaded
// only by calls under a span): tiers 0, 1, 2 and 3, exact search, careful loop; same LDS footprint as the end-to-end ones.
void wfa_launch_align_ef(const WfaAlignParams& p, int tier, bool with_bt, bool raw, int grid, hipStream_t stream,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int wfa_align_ef_max_blocks_per_cu(int tier, bool with_bt, bool raw, size_t lds_bytes);
void wfa_prime_align_ef(hipStream_t stream);
// The span of wfagpu_amd_configure_span (wfa_launch.hip): false when none is configured; out (optional) receives
// {pattern begin, pattern end, text begin, text end} free.  wfa_lane_span: the span the calling thread -- a lane of
// launch_alignments* -- wants its wfagpu_amd_align_device call to run under (nullptr: end to end), as four ints.
bool wfa_configured_span(int* out4);
const int* wfa_lane_span4();
// The two-piece instantiations (align_kernel_2p.hip: a code object of their own, loaded only by two-piece calls): tiers 0, 1, 2 and 3,
// exact search, careful loop, origin bytes in ROWS.  wfa_align_lds_bytes serves them too (WfaAlignParams::e2 > 0).
void wfa_launch_align_2p(const WfaAlignParams& p, int tier, bool with_bt, bool raw, int grid, hipStream_t stream,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int wfa_align_2p_max_blocks_per_cu(int tier, bool with_bt, bool raw, size_t lds_bytes);
void wfa_prime_align_2p(hipStream_t stream);
// The penalties of wfagpu_amd_configure_affine2p (wfa_launch.hip): false when none are configured; out (optional) receives
// {x, o1, e1, o2, e2}.  wfa_lane_affine2p5: what the calling thread -- a lane of launch_alignments* -- wants its
// wfagpu_amd_align_device call to run under (nullptr: gap-affine), as five ints.
bool wfa_configured_affine2p(int* out5);
const int* wfa_lane_affine2p5();
// The wf-adaptive instantiations (align_kernel_ad.hip: a code object of their own, loaded only by calls under the heuristic): tiers 0,
// 1, 2 and 3, careful loop with WFA2's cut-off, origin bytes in ROWS; the gap-affine backtrace kernels serve them as they are.
// wfa_align_lds_bytes serves them too (WfaAlignParams::ad_steps > 0).
void wfa_launch_align_ad(const WfaAlignParams& p, int tier, bool with_bt, bool raw, int grid, hipStream_t stream,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int wfa_align_ad_max_blocks_per_cu(int tier, bool with_bt, bool raw, size_t lds_bytes);
void wfa_prime_align_ad(hipStream_t stream);
// The heuristic of wfagpu_amd_configure_wfadaptive (wfa_launch.hip): false when none is configured; out (optional) receives
// {min_wavefront_length, max_distance_threshold, steps_between_cutoffs}.  wfa_lane_wfadaptive3: what the calling thread -- a lane of
// launch_alignments* -- wants its wfagpu_amd_align_device call to run under (nullptr: exact), as three ints.
bool wfa_configured_wfadaptive(int* out3);
const int* wfa_lane_wfadaptive3();
// The one-component instantiations (align_kernel_lin.hip: a code object of their own, loaded only by calls under an edit, indel or
// gap-linear metric): tiers 0, 1, 2 and 3, exact search, careful loop, origin bytes in ROWS.  wfa_align_lds_bytes serves them too
// (WfaAlignParams::de == 0).
void wfa_launch_align_lin(const WfaAlignParams& p, int tier, bool with_bt, bool raw, int grid, hipStream_t stream,
                          hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int wfa_align_lin_max_blocks_per_cu(int tier, bool with_bt, bool raw, size_t lds_bytes);
void wfa_prime_align_lin(hipStream_t stream);
// The metric of wfagpu_amd_configure_linear (wfa_launch.hip): false when none is configured; out (optional) receives
// {metric, mismatch, indel}.  wfa_lane_linear3: what the calling thread -- a lane of launch_alignments* -- wants its
// wfagpu_amd_align_device call to run under (nullptr: gap-affine), as three ints.
bool wfa_configured_linear(int* out3);
const int* wfa_lane_linear3();
// The instantiations for a one-component metric under an ends-free span (align_kernel_linef.hip: a code object of their own, loaded
// only by such calls): tiers 0, 1, 2 and 3, exact search, careful loop, origin bytes in ROWS; the one-component backtrace kernels
// serve them as they are (the span travels in WfaTraceParams).  wfa_align_lds_bytes serves them too (WfaAlignParams::de == 0).
void wfa_launch_align_linef(const WfaAlignParams& p, int tier, bool with_bt, bool raw, int grid, hipStream_t stream,
                            hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int wfa_align_linef_max_blocks_per_cu(int tier, bool with_bt, bool raw, size_t lds_bytes);
void wfa_prime_align_linef(hipStream_t stream);
// The span that wfagpu_amd_configure_linear_span set with its metric (wfa_launch.hip): false when the configured metric runs end to
// end, or none is configured; out (optional) receives the four members.  wfa_lane_linear_span4: the span the calling thread -- a lane
// of launch_alignments* -- wants its metric to run under (nullptr: end to end).
bool wfa_configured_linear_span(int* out4);
const int* wfa_lane_linear_span4();
bool wfa_launch_trace(const WfaTraceParams& p, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);     // false: nothing to launch
// (the backtrace of two-piece alignments: trace_kernel_2p.hip, the same kernels compiled for five walk states and BT2_* origin bytes)
bool wfa_launch_trace_2p(const WfaTraceParams& p, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
void wfa_prime_trace_2p(hipStream_t stream);
// (the backtrace of edit, indel and gap-linear alignments: trace_kernel_lin.hip, the same kernels compiled for one walk state and BTL_* origin bytes)
bool wfa_launch_trace_lin(const WfaTraceParams& p, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
void wfa_prime_trace_lin(hipStream_t stream);
// Tier 5 (short_kernel.hip): 64 / lanes alignments per wavefront (lanes = 16 or 32 diagonals each), rings in registers; with_bt: one row
// of `lanes` origin bytes per score for the backtrace.
bool wfa_short_supported(int x, int oe, int e);
size_t wfa_short_lds_bytes(const WfaAlignParams& p, int lanes, bool with_bt);
void wfa_launch_short(const WfaAlignParams& p, int lanes, bool with_bt, int grid, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int wfa_short_max_blocks_per_cu(const WfaAlignParams& p, int lanes, bool with_bt);     // (wavefronts a CU holds: registers and LDS)
unsigned long long wfa_short_bt_slot_units(int max_score, int lanes);     // (with_bt: arena units every work item of the launch owns)
// Tier 5's instantiations are picked from tables [x - 1][o + e - 1]; one translation unit (one code object) per gap extension e:
// short_kernel.hip holds e = 1, short_kernel_e2/3/4.hip the others (short_kernel_impl.h is the kernel).
struct WfaShortEntry { void (*launch)(const WfaAlignParams&, int, hipStream_t, hipEvent_t, hipEvent_t); int (*occ)(size_t); };
const WfaShortEntry* wfa_short_entry_e2(int ascii, int bt, int l32, int idx);
const WfaShortEntry* wfa_short_entry_e3(int ascii, int bt, int l32, int idx);
const WfaShortEntry* wfa_short_entry_e4(int ascii, int bt, int l32, int idx);
// Which of the optional code objects -- the ones only some callers load -- this process has entered: every host function that launches,
// queries or primes a kernel of such a unit says so (the runtime loads a code object at the first of these).  Process-wide, never
// cleared; wfagpu_amd_debug_code_objects() (wfa_host.hip) hands the bits out, tests check "never loaded" with them.
enum : unsigned { WFA_UNIT_ALIGN_EF = 1u, WFA_UNIT_ALIGN_2P = 2u, WFA_UNIT_TRACE_2P = 4u, WFA_UNIT_ALIGN_AD = 8u, WFA_UNIT_ALIGN_LIN = 16u, WFA_UNIT_TRACE_LIN = 32u, WFA_UNIT_ALIGN_LINEF = 64u };
void wfa_unit_entered(unsigned unit);
// Code-object priming: one empty launch per kernel translation unit (see the definitions).
void wfa_prime_pack(hipStream_t stream);
void wfa_prime_align(hipStream_t stream);
void wfa_prime_short(hipStream_t stream);
void wfa_prime_trace(hipStream_t stream);
