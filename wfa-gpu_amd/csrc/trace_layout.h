// LDS arithmetic of the backtrace kernels (trace_kernel.hip) and the choice of their mapping: ONE home for every size, used by the
// kernels (to lay their LDS out), by their launchers (to request it) and by the host driver (to decide what fits).  Plain C++17: no
// HIP header needed, compiles with a host compiler alone (tests/trace_plan_check.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WFA_HD __host__ __device__
#else
#define WFA_HD
#endif

constexpr int TILE_LDS_W = 32;          // bytes per row of the origin-byte tile of the wave and group kernels (fetch_bt_rows)
constexpr int LANE_WAVES = 4;           // wavefronts per workgroup of wfa_trace_lane_kernel, a share of LDS each
constexpr int LANE_CACHE_BYTES = 72;    // per lane of the walk: 8 row-table entries (one 64-byte line) + 8 bytes of bank spread
// Policy, not layout: a wavefront of the wave / group kernels stays within 40 KiB (four of them fit a CU), the lane kernels stage the
// pairs of a whole wavefront only where 64 of them fit 48 KiB, a walk-only wavefront keeps op lists of up to 39 KiB in LDS.
constexpr size_t TRACE_LDS_WAVE_CAP = (size_t)40 << 10;
constexpr size_t TRACE_LDS_STAGE_CAP = (size_t)48 << 10;
constexpr size_t TRACE_LDS_WALK_OPS_CAP = (size_t)39 << 10;
constexpr size_t TRACE_WAVE_MIN_ROOM = 64;      // the wave kernel is worth choosing only with this much LDS left beside sequences and tile

// words of one sequence of `len` bases (2-bit packed, or raw bytes) + the word the replay reads ahead
WFA_HD constexpr unsigned trace_seq_words(unsigned len, bool raw) { return raw ? (len + 3) / 4 + 1 : (len + 15) / 16 + 1; }

// wfa_trace_wave_kernel: both sequences, the tile of 64 rows, op list, text; walk only: tile and op list
WFA_HD constexpr size_t wave_kernel_lds_bytes(int seq_words_cap, int ops_lds_bytes, int text_lds_bytes) {
  return (size_t)2 * seq_words_cap * 4 + (size_t)64 * TILE_LDS_W + (size_t)ops_lds_bytes + (size_t)text_lds_bytes;
}
WFA_HD constexpr size_t wave_walk_lds_bytes(int ops_lds_bytes) { return (size_t)64 * TILE_LDS_W + (size_t)ops_lds_bytes; }
// wfa_trace_group_kernel<G>: the same per group of 64 / G lanes (a tile row per lane), every share a multiple of 16 bytes
WFA_HD constexpr size_t group_share_bytes(int g, int seq_words_cap, int ops_lds_bytes, int text_lds_bytes) {
  return ((size_t)2 * seq_words_cap * 4 + (size_t)(64 / g) * TILE_LDS_W + (size_t)ops_lds_bytes + (size_t)text_lds_bytes + 15) / 16 * 16;
}
WFA_HD constexpr size_t group_kernel_lds_bytes(int g, int seq_words_cap, int ops_lds_bytes, int text_lds_bytes) {
  return group_share_bytes(g, seq_words_cap, ops_lds_bytes, text_lds_bytes) * g;
}
// wfa_trace_lane_kernel: per wavefront the staged pairs, their op lists, the walk's cache of every lane
WFA_HD constexpr size_t lane_kernel_wave_bytes(int emit_pairs, int seq_lds_stride, int ops_lds_bytes) {
  return ((size_t)emit_pairs * seq_lds_stride * 4 + (size_t)emit_pairs * ops_lds_bytes + (size_t)64 * LANE_CACHE_BYTES + 15) & ~(size_t)15;
}
WFA_HD constexpr size_t lane_kernel_lds_bytes(int emit_pairs, int seq_lds_stride, int ops_lds_bytes) {
  return (size_t)LANE_WAVES * lane_kernel_wave_bytes(emit_pairs, seq_lds_stride, ops_lds_bytes);
}
// wfa_emit_kernel: the staged pairs; with op lists (walk-only passes): an odd number of words per pair behind them
WFA_HD constexpr uint32_t emit_ops_words(uint32_t ops_slot) { return ((ops_slot >> 2) + 1u) | 1u; }
WFA_HD constexpr size_t emit_kernel_lds_bytes(int emit_pairs, int seq_lds_stride) { return (size_t)emit_pairs * seq_lds_stride * 4; }
WFA_HD constexpr size_t emit_ops_kernel_lds_bytes(int emit_pairs, int seq_lds_stride, uint32_t ops_slot) {
  return (size_t)emit_pairs * ((size_t)seq_lds_stride * 4 + (size_t)emit_ops_words(ops_slot) * 4);
}
// (what the planner budgets per pair of such a pass: emit_ops_words(slot) * 4 <= slot + 8 for every slot)
WFA_HD constexpr size_t emit_ops_pair_bytes_max(unsigned seq_lds_stride, unsigned long long ops_slot) { return (size_t)seq_lds_stride * 4 + (size_t)ops_slot + 8; }

// ---- which kernels walk and replay a chain's finished alignments ---------------------------------------------------------------
// Two steps, because one input -- the largest score of the pass -- is on the device until the caller has read the counters:
// trace_plan_begin needs none of it and says (by_bound) whether the caller can do without the read; trace_plan_finish takes it.
struct TracePlanIn {
  size_t lds_max;            // LDS a workgroup may request on this device
  int trace_mode;            // wfagpu_amd_tuning_t::trace_mode
  int emit_pairs;            // wfagpu_amd_tuning_t::emit_pairs (8..64: forced)
  bool raw;                  // byte-compare class
  unsigned max_len;          // longest sequence of the pass
  uint32_t n_chain;          // alignments of the chain
  long long s_hi;            // no pair of the chain finished above this score
  int min_op_cost;           // min(x, e)
  int item_chars;            // widest RLE item
  int extra_items = 0;       // RLE items beyond 2 * operations + 1 (ends-free: the two free runs)
};
struct TracePlan {
  // the mapping fields of WfaTraceParams
  int seq_lds_stride, emit_pairs, seq_words_cap, wave_kernel, group, lane_fused, walk_only;
  uint32_t ops_slot;
  int ops_lds_bytes, text_lds_bytes;
  // for the caller
  bool by_bound;                               // scratch sizes from the bounds below: no counter read
  unsigned long long ops_bound, text_bound;
  bool text_scratch;                           // single replay into a text scratch + compaction
};

inline TracePlan trace_plan_begin(const TracePlanIn& in) {
  TracePlan tp{};
  // both sequences of a pair, as words, per lane; staged in LDS when 64 lanes fit 48 KiB
  const unsigned per_seq = trace_seq_words(in.max_len, in.raw);
  const unsigned stride = (2 * per_seq) | 1u;
  tp.seq_lds_stride = (emit_kernel_lds_bytes(64, (int)stride) <= TRACE_LDS_STAGE_CAP && in.trace_mode != 1) ? (int)stride : 0;
  // alignments per wavefront of the staged replay: as many as still leave a CU eight wavefronts (two per SIMD).  LDS decides:
  // 1 kbp reads at 64 per wavefront are 4 wavefronts per CU, one per SIMD, every dependent LDS read of the replay exposed;
  // measured on BASELINE configs[2] (trace ms per 1M pairs): 64: 4.14, 56: 3.92, 48: 3.84, 40: 3.84, 32: 3.79, 24: 3.82
  tp.emit_pairs = 64;
  if (tp.seq_lds_stride > 0) {
    while (tp.emit_pairs > 16 && in.lds_max / emit_kernel_lds_bytes(tp.emit_pairs, (int)stride) < 8) tp.emit_pairs -= 8;
    if (in.emit_pairs >= 8 && in.emit_pairs <= 64) tp.emit_pairs = in.emit_pairs & ~7;
  }
  // sequences too long to stage 64 pairs per wavefront: one wavefront per alignment (sequences of ONE pair in LDS)
  tp.seq_words_cap = (int)per_seq + 1;
  // (it needs both sequences of a pair plus the tile and a little room in LDS; sequences at the very edge of what the align tiers
  // stage do not leave that: the lane-per-alignment walk + windowed emit take any length)
  tp.wave_kernel = (tp.seq_lds_stride == 0 && in.trace_mode != 1 &&
                    wave_kernel_lds_bytes(tp.seq_words_cap, 0, 0) + TRACE_WAVE_MIN_ROOM <= in.lds_max) ? 1 : 0;
  // Scratch sizes.  Lane-per-alignment kernels with a bounded score: from the bound (no pair of the chain finished
  // above s_hi), no round trip.  The wave kernels size their LDS from the largest score of the pass and the
  // unbounded tier has no bound: those read the sums k_trace_bounds has formed.
  const unsigned long long s_pos = (unsigned long long)(in.s_hi > 0 ? in.s_hi : 0);
  tp.ops_bound = (unsigned long long)in.n_chain * ((s_pos + 3ull) & ~3ull);
  tp.text_bound = (unsigned long long)in.n_chain * ((unsigned long long)in.item_chars * (2ull * (s_pos / (unsigned long long)in.min_op_cost) + 1ull + (unsigned long long)in.extra_items) + 1ull);
  // (the bound is sized by the chain's largest budget -- the caller's max_error once a re-run link follows -- for EVERY pair:
  // fine for the batches of a pipelined call, whose round trips it saves (62 500 x 1 kbp pairs: 225 MB), too generous for a
  // big resident batch (1M pairs at max_error 300: 3.6 GB of fresh device memory per buffer to save one counter read)
  tp.by_bound = !tp.wave_kernel && in.s_hi >= 0 && in.s_hi <= 30000 && tp.text_bound <= ((unsigned long long)768 << 20);
  return tp;
}

// pass_max_score: the largest score of the pass as the device counted it (not looked at where tp.by_bound)
inline void trace_plan_finish(TracePlan& tp, const TracePlanIn& in, unsigned long long pass_max_score) {
  const unsigned stride = (2 * trace_seq_words(in.max_len, in.raw)) | 1u;
  {
    // op list (one byte per score point of the largest score of the pass) and CIGAR text of one alignment in LDS,
    // within 40 KiB per wavefront so that at least four of them fit a CU
    const size_t seq_b = wave_kernel_lds_bytes(tp.seq_words_cap, 0, 0);      // (sequences + the tile)
    size_t room = seq_b < TRACE_LDS_WAVE_CAP ? TRACE_LDS_WAVE_CAP - seq_b : 0;
    const size_t smax = tp.by_bound ? (size_t)in.s_hi : (size_t)pass_max_score;
    tp.ops_lds_bytes = (int)(((smax + 3) & ~(size_t)3) <= room ? ((smax + 15) & ~(size_t)15) : 0);
    room -= (size_t)tp.ops_lds_bytes;
    const size_t text_want = 2 * smax + 64;
    tp.text_lds_bytes = (int)((room < text_want ? room : text_want) & ~(size_t)15);
    // Several alignments per wavefront (64/G lanes and one LDS share each) for SHORT op lists only (2 kbp reads, G = 8:
    // 262k pairs 13.2 -> 6.6 ms).  With hundreds of operations per alignment the replays of the groups diverge and
    // the wavefront per alignment wins again (16k x 10 kbp: 2.7 ms against 4.0 ms with G = 4).
    // (16 bytes of slack per share on top of what the kernel requests.  The same decision as (unrounded share + 16) * g <= cap, which
    // this test was before the shares had a function: ops_lds_bytes and text_lds_bytes are multiples of 16, the sequences add a
    // multiple of 8, and cap / g is a multiple of 16 -- rounding a share up to 16 can then never cross the limit.  Keep it so.)
    tp.group = 1;
    if (in.trace_mode == 0 && tp.ops_lds_bytes > 0 && smax <= 512)
      for (int g = 8; g >= 2; g >>= 1)
        if (group_kernel_lds_bytes(g, tp.seq_words_cap, tp.ops_lds_bytes, tp.text_lds_bytes) + (size_t)16 * g <= TRACE_LDS_WAVE_CAP && in.n_chain >= (uint32_t)g * 1024u) { tp.group = g; break; }
  }
  // LONG alignments, one wavefront each: the wavefront kernel only walks; the replay is the staged lane-per-alignment kernel's
  // with as many pairs per wavefront (8, 16, ...) as fit LDS next to three more wavefronts (a replay is one serial chain:
  // run by a whole wavefront it is 64 lanes executing the same chain).  Op lists in slots of the largest score of the pass.
  // (big passes only: a replay step takes a lane of the lane kernel -- its neighbours in other branches -- 1.3 us against the 0.4 us
  // of a wavefront with a SIMD to itself; with thousands of alignments the wavefronts share SIMDs five at a time and the lanes
  // win: 16 384 x 10 kbp at 3 %, trace 2.22 -> 2.04 ms.  tuning.trace_mode 4: whatever the size of the pass -- tests)
  tp.walk_only = 0;
  if (tp.wave_kernel && tp.group == 1 && in.trace_mode != 2 && (in.n_chain >= 8192u || in.trace_mode == 4)) {
    const unsigned long long slot = (pass_max_score + 3ull) & ~3ull;
    const size_t per_pair = emit_ops_pair_bytes_max(stride, slot);      // LDS of one alignment of the replay: sequences + op list
    if (8 * per_pair <= in.lds_max && (unsigned long long)in.n_chain * slot <= (1ull << 30)) {
      tp.walk_only = 1; tp.ops_slot = (uint32_t)slot;
      tp.seq_lds_stride = (int)stride;
      tp.emit_pairs = 8;
      while (tp.emit_pairs < 64 && (size_t)(tp.emit_pairs + 8) * per_pair * 4 <= in.lds_max) tp.emit_pairs += 8;
      const int forced = in.emit_pairs;
      if (forced >= 8 && forced <= 64 && (size_t)(forced & ~7) * per_pair <= in.lds_max) tp.emit_pairs = forced & ~7;
      // (the walk keeps its op list in LDS when it fits: ops_lds_bytes from above, without the sequences)
      const size_t smax = (size_t)pass_max_score;
      tp.ops_lds_bytes = (int)(smax + 16 <= TRACE_LDS_WALK_OPS_CAP ? ((smax + 15) & ~(size_t)15) : 0);
      tp.text_lds_bytes = 0;
    }
  }
  // SHORT alignments (no pair of the chain finished above a score of 124): walk and replay in one kernel, op lists in LDS
  tp.lane_fused = 0;
  if (!tp.wave_kernel && tp.seq_lds_stride > 0 && in.s_hi >= 0 && in.s_hi <= 124 && in.trace_mode != 3) {
    tp.lane_fused = 1;
    tp.ops_lds_bytes = (int)((in.s_hi + 3) & ~3ll);
    if (!(in.emit_pairs >= 8 && in.emit_pairs <= 64)) {
      tp.emit_pairs = 64;
      while (tp.emit_pairs > 16 && in.lds_max / lane_kernel_wave_bytes(tp.emit_pairs, (int)stride, tp.ops_lds_bytes) < 8) tp.emit_pairs -= 8;
    }
    // (the kernel's workgroups are LANE_WAVES wavefronts with a share of LDS each; 16 bytes of slack per share)
    while (tp.emit_pairs > 8 && LANE_WAVES * (lane_kernel_wave_bytes(tp.emit_pairs, (int)stride, tp.ops_lds_bytes) + 16) > in.lds_max) tp.emit_pairs -= 8;
  }
  // lane-per-alignment emit with whole sequences staged: one replay into a scratch + compaction (big passes only: the
  // scratch holds the upper bounds, ~3x the text)
  // (long alignments replayed by the lane kernel -- walk_only -- always: a second replay of hundreds of operations costs more than
  // the compaction launch)
  tp.text_scratch = ((!tp.wave_kernel && in.n_chain >= 8192u) || tp.walk_only) && !tp.lane_fused && tp.seq_lds_stride > 0;
}

#undef WFA_HD
