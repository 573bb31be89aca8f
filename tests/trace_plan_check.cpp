// Stand-alone check of the backtrace planner (wfa-gpu_amd/csrc/trace_layout.h), host compiler only: tests/test_trace_plan_cpu.py
// compiles and runs it.  Every plan of a sweep over lengths, scores, chain sizes and tuning.trace_mode must request no more LDS than
// the device limit it was given and stage a multiple of 8 pairs in 8..64; five named shapes are pinned to the mapping the host
// driver chose for them before the choice was lifted out of its chain loop (values taken from that code, not from this header).
#include <cstdio>
#include <cstring>

#include "trace_layout.h"

// which kernels wfa_launch_trace starts for a plan (the order of its tests)
static const char* mapping(const TracePlan& p) {
  if (p.wave_kernel && p.group > 1) return p.group == 8 ? "group8" : p.group == 4 ? "group4" : "group2";
  if (p.wave_kernel && !p.walk_only) return "wave";
  if (p.wave_kernel) return "walk-only";
  if (p.lane_fused) return "lane-fused";
  if (p.seq_lds_stride == 0) return "window";
  return "walk+emit";
}
// the dynamic LDS the largest request of that launch asks for
static size_t lds_request(const TracePlan& p) {
  if (p.wave_kernel && p.group > 1) return group_kernel_lds_bytes(p.group, p.seq_words_cap, p.ops_lds_bytes, p.text_lds_bytes);
  if (p.wave_kernel && !p.walk_only) return wave_kernel_lds_bytes(p.seq_words_cap, p.ops_lds_bytes, p.text_lds_bytes);
  if (p.wave_kernel) {
    const size_t walk = wave_walk_lds_bytes(p.ops_lds_bytes), emit = emit_ops_kernel_lds_bytes(p.emit_pairs, p.seq_lds_stride, p.ops_slot);
    return walk > emit ? walk : emit;
  }
  if (p.lane_fused) return lane_kernel_lds_bytes(p.emit_pairs, p.seq_lds_stride, p.ops_lds_bytes);
  if (p.seq_lds_stride == 0) return 0;
  return emit_kernel_lds_bytes(p.emit_pairs, p.seq_lds_stride);
}
static int item_chars_of(unsigned max_len) {
  int c = 2;
  for (unsigned v = max_len; v >= 10; v /= 10) ++c;
  return c < 6 ? 6 : c;
}
static TracePlan plan(size_t lds_max, int mode, bool raw, unsigned len, uint32_t n, long long s_hi, unsigned long long smax) {
  const TracePlanIn in{lds_max, mode, 0, raw, len, n, s_hi, 1, item_chars_of(len)};
  TracePlan p = trace_plan_begin(in);
  trace_plan_finish(p, in, smax);
  return p;
}

int main() {
  int bad = 0;
  long plans = 0;
  const unsigned lens[] = {150, 1000, 1700, 10000, 30000, 60000};
  const long long scores[] = {0, 124, 125, 512, 513, 3000, 40000};
  const uint32_t chains[] = {1, 1024, 8191, 8192, 1000000};
  const size_t limits[] = {(size_t)64 << 10, (size_t)160 << 10};
  for (size_t lds_max : limits) for (int raw = 0; raw < 2; ++raw) for (int mode = 0; mode <= 4; ++mode)
  for (unsigned len : lens) for (long long s : scores) for (uint32_t n : chains) {
    const TracePlan p = plan(lds_max, mode, raw != 0, len, n, s, (unsigned long long)s);
    ++plans;
    if (lds_request(p) > lds_max) { printf("LDS %zu > %zu: %s, mode %d raw %d len %u score %lld n %u\n", lds_request(p), lds_max, mapping(p), mode, raw, len, s, n); ++bad; }
    if (p.emit_pairs < 8 || p.emit_pairs > 64 || p.emit_pairs % 8) { printf("emit_pairs %d: mode %d raw %d len %u score %lld n %u\n", p.emit_pairs, mode, raw, len, s, n); ++bad; }
  }
  // {shape, tuning.trace_mode, length, pairs, largest budget of the chain, largest score of the pass} -> mapping, pairs per wavefront of the staged
  // kernels, op-list and text bytes in LDS, sizes by bound, text scratch
  struct Pin { const char* name; int mode; unsigned len; uint32_t n; long long s_hi; unsigned long long smax;
               const char* map; int emit_pairs, ops_lds, text_lds; bool by_bound, text_scratch; };
  const Pin pins[] = {
    {"cfg2", 0, 150, 100000, 45, 45, "lane-fused", 64, 48, 144, true, false},
    {"cfg3", 0, 1000, 1000000, 300, 160, "walk+emit", 32, 160, 384, false, true},
    {"cfg4", 0, 10000, 16384, 3000, 1100, "walk-only", 8, 1104, 0, false, true},
    {"cfg5", 0, 30000, 1024, 9000, 8200, "wave", 64, 8208, 15680, false, false},
    {"trace_mode=1", 1, 10000, 16384, 3000, 1100, "window", 64, 3008, 6064, true, false},
  };
  for (const Pin& k : pins) {
    const TracePlan p = plan((size_t)160 << 10, k.mode, false, k.len, k.n, k.s_hi, k.smax);
    if (strcmp(mapping(p), k.map) || p.emit_pairs != k.emit_pairs || p.ops_lds_bytes != k.ops_lds || p.text_lds_bytes != k.text_lds ||
        p.by_bound != k.by_bound || p.text_scratch != k.text_scratch) {
      printf("%s: %s emit_pairs %d ops_lds %d text_lds %d by_bound %d text_scratch %d, expected %s %d %d %d %d %d\n", k.name, mapping(p), p.emit_pairs,
             p.ops_lds_bytes, p.text_lds_bytes, (int)p.by_bound, (int)p.text_scratch, k.map, k.emit_pairs, k.ops_lds, k.text_lds, (int)k.by_bound, (int)k.text_scratch);
      ++bad;
    }
  }
  // the group kernel's window: G by the size of the CHAIN (tests/test_gpu_parity.py reaches these on the device: batches of 2100 and
  // 4200 pairs, and one of 8800 whose chain is the 8250 pairs left by the sample that tunes the score budgets)
  const struct { uint32_t n; const char* map; } groups[] = {{2047, "wave"}, {2100, "group2"}, {4200, "group4"}, {8191, "group4"}, {8250, "group8"}};
  for (const auto& g : groups) {
    const TracePlan p = plan((size_t)160 << 10, 0, false, 1700, g.n, 450, 120);
    if (strcmp(mapping(p), g.map)) { printf("1700 bp x %u: %s, expected %s\n", g.n, mapping(p), g.map); ++bad; }
  }
  if (bad) return 1;
  printf("trace_plan_check ok: %ld plans\n", plans);
  return 0;
}
