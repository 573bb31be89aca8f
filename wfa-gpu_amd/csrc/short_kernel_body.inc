// short_kernel_body.inc -- the body of the tier-5 kernels: wfa_short_kernel (short_kernel_impl.h, gap-affine: LIN == false) and
// wfa_short_lin_kernel (short_kernel_lin.hip, the one-component metrics: LIN == true).  Textually included in both, where L, X, OE, E,
// BT, ASCII, LIN, EF and the kernel argument p are declared; the notes in front of wfa_short_kernel describe it.
// EF (wfa_short_linef_kernel, short_kernel_linef.hip: the metrics; wfa_short_ef_kernel, short_kernel_ef_impl.h: gap-affine): under an
// ends-free span -- a start row, an interval of end diagonals, the diagonal the alignment ended on to WfaAlignParams::ends.
// TP2 (wfa_short_2p_kernel, short_kernel_2p.hip): two-piece penalties, end to end -- OE / E are the first piece, OE2 / E2 the second; five
// values per cell, their rings in registers (the notes in front of that kernel).  Every kernel declares TP2, OE2 and E2.
  static_assert(TP2 ? (!LIN && !EF && X >= 1 && E >= 1 && OE >= E && E2 >= 1 && OE2 >= E2 && (L == 16 || L == 32)) : LIN ? (X >= 0 && X <= 8 && OE >= 1 && OE <= 4 && E == OE && (X > 0 || OE == 1)) : (X >= 1 && X <= 8 && OE >= 1 && OE <= 8 && E >= 1 && E <= OE && L >= 16), "history of eight scores");
  // (TP2: max(X, OE, OE2) rounded up to a multiple of E and of E2 -- short2p_ring_depth --, so that the unrolled score loop finds every ring at a constant index)
  constexpr int D = TP2 ? short2p_ring_depth(X, OE, E, OE2, E2) : (X > OE ? X : OE);
  constexpr int RL = L < 16 ? 16 : L;     // bytes of a row of origin bytes: whole 16-byte units
  constexpr int DG = TP2 ? E : (E == 1 ? 1 : D);      // depth of the I / D history (TP2: of I1 / D1, exactly E scores back)
  extern __shared__ __attribute__((aligned(16))) uint32_t slds[];
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63, grp = lane / L, j = lane % L;
  const int cap = p.seq_words_cap;
  // Two sets of staged sequences: the pairs of this iteration and the pairs of the next one (below).
  const size_t set_words = (((size_t)G * 2 * cap) + 3) & ~(size_t)3;
  uint32_t* Pw = slds + (size_t)grp * 2 * cap;
  uint32_t* Pn = Pw + set_words;
  // BT: the group's rows of origin bytes collect in LDS ([score][lane of the group], behind the staged sequences) and go out in
  // 16-byte pieces when the alignment is done.  (A global byte store per score -- four 16-byte pieces of four different cache
  // lines per wave instruction -- cost 0.035 of the 0.26 ms per 100k configs[1] pairs.)
  const int rows_cap = p.max_score + 1;
  uint8_t* const lrows = BT ? reinterpret_cast<uint8_t*>(slds + 2 * set_words) + (size_t)grp * rows_cap * RL + j : nullptr;
  uint32_t n_work = p.n_work;
  if (p.n_work_dev) n_work = min(n_work, (uint32_t)*p.n_work_dev);
  const unsigned long long grp_mask = (L == 64) ? ~0ull : (((1ull << L) - 1ull) << (grp * L));
  uint32_t lane_rows = 0;                                   // (group leaders: rows -- score + 1 -- of the alignments they finished; x L = cells)
  // pairs of this wavefront's share that did not leave DONE / went to fail_list / were flagged ALPHABET: wave-uniform counts (scalar
  // registers: the kernel's vector registers decide how many wavefronts a SIMD holds)
  uint32_t not_done = 0, n_fail = 0, n_flag = 0;
  auto count_of = [](const bool pred) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(pred)); };
  unsigned long long arena_top0 = 0;                        // (the bump pointer as the launch found it: nobody moves it while the launch runs)
  if constexpr (BT) {
    if (p.arena_top_known) {
      // (nobody reads the bump pointer while the launch runs: workgroup 0 moves it past the launch's slots, never beyond the arena)
      arena_top0 = p.arena_top0_value;
      if (blockIdx.x == 0 && lane == 0) {
        const uint32_t tab_units = (uint32_t)(((long long)p.max_score + 2) >> 1), slot = tab_units + (uint32_t)(p.max_score + 1) * (RL / 16);
        const unsigned long long t = arena_top0 + (unsigned long long)n_work * slot;
        *p.arena_top = t < p.arena_units ? t : p.arena_units;
      }
    } else arena_top0 = *p.arena_top;
  }

  // Software pipeline over the iterations of a wavefront.  All wavefronts of a launch start together, do the same amount of work
  // and so stay in step: with the loads of an iteration issued when it starts -- work item -> record and status -> sequences,
  // three dependent round trips, every wavefront of the chip asking at once -- the vector pipe sat idle for half of the launch
  // (0.133 ms per 100k configs[1] pairs at 47 % VALU busy; with CIGARs, whose stores the next loads also queued behind, 0.22).
  // Now the work item of iteration i+3, the record of i+2 and the sequences of i+1 are requested at the top of iteration i and
  // looked at one iteration later; the sequences wait in registers (NPF words per lane and sequence; longer ones fetch the
  // rest when they are staged) and go into the other LDS set when iteration i is done.
  constexpr int NPF = ASCII ? 1 : 2;
  struct Meta { uint32_t pair, st, poff, toff; int plen, tlen, budget; uint32_t pasc, tasc; };      // (pasc / tasc: ASCII, dword index of the sequence in the batch)
  struct SeqRegs { uint32_t a[ASCII ? 4 : NPF], b[ASCII ? 4 : NPF]; };
  const uint32_t* const asc = reinterpret_cast<const uint32_t*>(p.ascii);
  uint32_t* const packed_out = const_cast<uint32_t*>(p.packed);
  const uint32_t stride = gridDim.x * G;
  auto fetch_pair = [&](const uint32_t b) -> uint32_t {     // (groups beyond the list look at its last item and stay inactive)
    const uint32_t w = min(b + (uint32_t)grp, n_work - 1u);
    return p.work ? p.work[w] : w;
  };
  auto fetch_meta = [&](const uint32_t pair) -> Meta {
    Meta m;
    m.pair = pair;
    m.st = p.only_pending ? p.status[pair] : (uint32_t)WFA_ST_PENDING;
    const WfaSeqPair mp = p.meta[pair];
    m.plen = (int)mp.pattern_len; m.tlen = (int)mp.text_len;
    // (the packed words: read, or -- ASCII, CIGAR launches -- written)
    m.poff = (ASCII && !BT) ? 0u : (uint32_t)(mp.pattern_offset_packed >> 2); m.toff = (ASCII && !BT) ? 0u : (uint32_t)(mp.text_offset_packed >> 2);
    m.pasc = ASCII ? (uint32_t)(mp.pattern_offset >> 2) : 0u; m.tasc = ASCII ? (uint32_t)(mp.text_offset >> 2) : 0u;
    if (p.budget) m.budget = p.budget[pair];
    else if (p.budget_q > 0) {
      // (k_budget's rule, wfa_host.hip)
      const unsigned long long ql = (unsigned long long)p.budget_q * (unsigned)max(m.plen, m.tlen);
      const long long v = (long long)((p.budget_margin == 100 ? ql : ql * (unsigned)p.budget_margin / 100ull) >> 10) + p.budget_slack;
      m.budget = (int)min(0x3FFFFFFFll, v);
    } else m.budget = p.max_score;
    return m;
  };
  auto words_of = [](const int len) { return ((len + 15) >> 4) + 1; };
  auto seq_ok = [&](const Meta& m, const uint32_t b) {      // will this group stage sequences for the iteration at list position b?
    return b + (uint32_t)grp < n_work && m.st == (uint32_t)WFA_ST_PENDING && words_of(m.plen) <= cap && words_of(m.tlen) <= cap;
  };
  auto fetch_seq = [&](const Meta& m, const bool ok) -> SeqRegs {
    SeqRegs r;
    const int pw = ok ? words_of(m.plen) : 0, tw = ok ? words_of(m.tlen) : 0;
    if constexpr (ASCII) {
      // the sixteen bytes of word j of either sequence (indices clamped to the sequence's last dword: pack_device.h; an empty
      // sequence may sit at the very end of the buffer: its fully masked loads go to the record array)
      const uint32_t* const ps = m.plen ? asc + m.pasc : reinterpret_cast<const uint32_t*>(p.meta);
      const uint32_t* const ts = m.tlen ? asc + m.tasc : reinterpret_cast<const uint32_t*>(p.meta);
      wfa_pack::PackWord a{0u, 0u, 0u, 0u}, b{0u, 0u, 0u, 0u};
      if (j < pw) a = wfa_pack::load_word(ps, (uint32_t)m.plen, (uint32_t)j);
      if (j < tw) b = wfa_pack::load_word(ts, (uint32_t)m.tlen, (uint32_t)j);
      r.a[0] = a.a0; r.a[1] = a.a1; r.a[2] = a.a2; r.a[3] = a.a3;
      r.b[0] = b.a0; r.b[1] = b.a1; r.b[2] = b.a2; r.b[3] = b.a3;
    } else {
#pragma unroll
    for (int u = 0; u < NPF; ++u) {
      const int i = j + u * L;
      r.a[u] = i < pw ? p.packed[(size_t)m.poff + i] : 0u;
      r.b[u] = i < tw ? p.packed[(size_t)m.toff + i] : 0u;
    }
    }
    return r;
  };
  // (ASCII: marks a group whose pair has a byte outside ACGT -- status ALPHABET, counted, out of this kernel's hands)
  auto stage_seq = [&](uint32_t* const Pb, Meta& m, const SeqRegs& r, const bool ok) {
    uint32_t* const Tb = Pb + cap;
    const int pw = ok ? words_of(m.plen) : 0, tw = ok ? words_of(m.tlen) : 0;
    if constexpr (ASCII) {
      uint32_t bad = 0;
      const uint32_t* const ps = m.plen ? asc + m.pasc : reinterpret_cast<const uint32_t*>(p.meta);
      const uint32_t* const ts = m.tlen ? asc + m.tasc : reinterpret_cast<const uint32_t*>(p.meta);
      // (the words go to the packed buffer as well where a backtrace kernel will look for them: CIGAR launches.  A pair that leaves a
      // score-only launch unfinished is packed again by the kernel that takes it over.)
      if (j < pw) { const uint32_t w = wfa_pack::pack_word(wfa_pack::PackWord{r.a[0], r.a[1], r.a[2], r.a[3]}, (uint32_t)m.plen, (uint32_t)j, bad); Pb[j] = w; if constexpr (BT) packed_out[(size_t)m.poff + j] = w; }
      if (j < tw) { const uint32_t w = wfa_pack::pack_word(wfa_pack::PackWord{r.b[0], r.b[1], r.b[2], r.b[3]}, (uint32_t)m.tlen, (uint32_t)j, bad); Tb[j] = w; if constexpr (BT) packed_out[(size_t)m.toff + j] = w; }
#pragma nounroll
      for (int i = j + L; i < pw; i += L) { const uint32_t w = wfa_pack::pack_word(wfa_pack::load_word(ps, (uint32_t)m.plen, (uint32_t)i), (uint32_t)m.plen, (uint32_t)i, bad); Pb[i] = w; if constexpr (BT) packed_out[(size_t)m.poff + i] = w; }
#pragma nounroll
      for (int i = j + L; i < tw; i += L) { const uint32_t w = wfa_pack::pack_word(wfa_pack::load_word(ts, (uint32_t)m.tlen, (uint32_t)i), (uint32_t)m.tlen, (uint32_t)i, bad); Tb[i] = w; if constexpr (BT) packed_out[(size_t)m.toff + i] = w; }
      const bool flagged = (__builtin_amdgcn_ballot_w64(bad != 0u) & grp_mask) != 0ull;
      if (flagged) {
        // WFA2 compares raw bytes: this pair belongs to the byte-compare class, which runs after the packed one
        if (j == 0) {
          atomicAdd(p.n_raw, 1ull);
          p.score[m.pair] = -1;
          p.status[m.pair] = WFA_ST_ALPHABET;
          if (p.cells) p.cells[m.pair] = 0;
        }
        m.st = WFA_ST_ALPHABET;
      }
      n_flag += count_of(flagged && j == 0);
      return;
    }
#pragma unroll
    for (int u = 0; u < NPF; ++u) {
      const int i = j + u * L;
      if (i < pw) Pb[i] = r.a[u];
      if (i < tw) Tb[i] = r.b[u];
    }
#pragma nounroll
    for (int i = j + NPF * L; i < pw; i += L) Pb[i] = p.packed[(size_t)m.poff + i];
#pragma nounroll
    for (int i = j + NPF * L; i < tw; i += L) Tb[i] = p.packed[(size_t)m.toff + i];
  };

  uint32_t base = blockIdx.x * G;
  Meta m0 = {}, m1 = {};
  uint32_t pair2 = 0;
  if (base < n_work) {
    // fill the pipeline
    m0 = fetch_meta(fetch_pair(base));
    m1 = fetch_meta(fetch_pair(base + stride));
    pair2 = fetch_pair(base + 2u * stride);
    const bool ok0 = seq_ok(m0, base);
    const SeqRegs r0 = fetch_seq(m0, ok0);
    stage_seq(Pw, m0, r0, ok0);
  }
  for (; base < n_work; base += stride) {
    // ---- requests for the iterations to come
    const Meta m2 = fetch_meta(pair2);
    const bool ok1 = seq_ok(m1, base + stride);
    const SeqRegs r1 = fetch_seq(m1, ok1);
    const uint32_t pair3 = fetch_pair(base + 3u * stride);
    // ---- this iteration
    const uint32_t w = base + grp;
    const bool active = w < n_work && m0.st == (uint32_t)WFA_ST_PENDING;
    const uint32_t pair = m0.pair;
    const int plen = active ? m0.plen : 0, tlen = active ? m0.tlen : 0;
    uint32_t* const Tw = Pw + cap;
    const int kend = tlen - plen;
    // (EF) the span of this pair: each value clamped to its sequence's length (an inactive group: zeros)
    int pbf = 0, pef = 0, tbf = 0, tef = 0;
    if constexpr (EF) { pbf = min(p.span_pbf, plen); pef = min(p.span_pef, plen); tbf = min(p.span_tbf, tlen); tef = min(p.span_tef, tlen); }
    const int pwords = ((plen + 15) >> 4) + 1, twords = ((tlen + 15) >> 4) + 1;
    // the pair's score budget and the diagonal window that can hold an alignment within it (align_kernel.hip: a path that
    // visits diagonal k beyond both 0 and kend pays one gap out and one gap back)
    int budget = p.max_score;
    if (active) budget = min(budget, m0.budget);
    {
      long long worst = (long long)X * min(plen, tlen) + (kend ? OE + (long long)E * (abs(kend) - 1) : 0);
      if constexpr (LIN) worst = (long long)((X && X < 2 * OE) ? X : 2 * OE) * min(plen, tlen) + (long long)OE * abs(kend);
      if constexpr (TP2) worst = (long long)X * min(plen, tlen) + wfa_gap2p(abs(kend), OE, E, OE2, E2);
      budget = (int)min((long long)budget, worst);
    }
    uint32_t status = WFA_ST_DONE;
    int wlo = 0;
    if constexpr (TP2) {
      // (align_kernel.hip, TWOPIECE: a path that visits a diagonal t beyond both 0 and kend holds gaps of t + |kend| bases one way and t
      // the other, g(t + |kend|) + g(t) <= S -- g the cheaper piece, subadditive; the largest such t by bisection, wfa_stray2p, once per
      // alignment; feasible: g(|kend|) <= S)
      if (active) {
        const int ak = kend < 0 ? -kend : kend;
        const bool feasible = wfa_gap2p(ak, OE, E, OE2, E2) <= (long long)budget;
        const int t = feasible ? wfa_stray2p(budget, ak, OE, E, OE2, E2) : 0;
        const int whi = min(max(0, kend) + t, tlen);
        wlo = max(min(0, kend) - t, -plen);
        if (!feasible) status = WFA_ST_SCORE;
        else if (whi - wlo + 1 > L || pwords > cap || twords > cap) status = WFA_ST_BAND;
      }
    } else if constexpr (EF && LIN) {
      // (align_kernel.hip, LINEAR && ENDSFREE: the hull of the start diagonals [-pbf, tbf] and the end diagonals [kend - tef, kend + pef],
      // beyond it (gb - what the two intervals leave between them) / 2 -- quotients of non-negative numerators only)
      if (active) {
        const int s_lo = -pbf, s_hi = tbf, e_lo = kend - tef, e_hi = kend + pef;
        const int hull_hi = max(s_hi, e_hi), hull_lo = min(s_lo, e_lo);
        const long long gb = budget / OE;
        const bool feasible = (long long)max(0, max(e_lo - s_hi, s_lo - e_hi)) <= gb;
        const long long a_hi = gb + s_hi + e_hi, a_lo = gb - s_lo - e_lo;
        int whi = a_hi >= 0 ? max(hull_hi, (int)min((long long)tlen, a_hi / 2)) : hull_hi;
        wlo = a_lo >= 0 ? min(hull_lo, -(int)min((long long)plen, a_lo / 2)) : hull_lo;
        whi = min(whi, tlen); wlo = max(wlo, -plen);
        if (!feasible) status = WFA_ST_SCORE;
        else if (whi - wlo + 1 > L || pwords > cap || twords > cap) status = WFA_ST_BAND;
      }
    } else if constexpr (EF) {
      // (align_kernel.hip, ENDSFREE: a path that visits a diagonal k above both intervals holds k - a bases of insertion and k - b of
      // deletion, a in [-pbf, tbf], b in [kend - tef, kend + pef], in at least one gap each: 2o + (2k - a - b) e <= S, widest at a = tbf,
      // b = kend + pef; below both, symmetric; between the hulls' ends every diagonal stays -- quotients of non-negative numerators only.
      // feasible: the gap between the two intervals is affordable.  A span of zeros: the end-to-end formulas below.)
      if (active) {
        const int s_lo = -pbf, s_hi = tbf, e_lo = kend - tef, e_hi = kend + pef;
        const int hull_hi = max(s_hi, e_hi), hull_lo = min(s_lo, e_lo);
        const long long S = budget, o = OE - E;
        const int gap = max(0, max(e_lo - s_hi, s_lo - e_hi));
        const bool feasible = (gap ? o + (long long)gap * E : 0) <= S;
        const long long a_hi = S - 2 * o + ((long long)s_hi + e_hi) * E, a_lo = S - 2 * o - ((long long)s_lo + e_lo) * E;
        int whi = a_hi >= 0 ? max(hull_hi, (int)min((long long)tlen, a_hi / (2 * E))) : hull_hi;
        wlo = a_lo >= 0 ? min(hull_lo, -(int)min((long long)plen, a_lo / (2 * E))) : hull_lo;
        whi = min(whi, tlen); wlo = max(wlo, -plen);
        if (!feasible) status = WFA_ST_SCORE;
        else if (whi - wlo + 1 > L || pwords > cap || twords > cap) status = WFA_ST_BAND;
      }
    } else if constexpr (LIN) {
      // (g (2 t + |kend|) <= S: t diagonals on either side of the end diagonals)
      if (active) {
        const int ak = kend < 0 ? -kend : kend, gb = budget / OE;
        const bool feasible = ak <= gb;
        const int t = feasible ? (gb - ak) / 2 : 0;
        const int whi = min(max(0, kend) + t, tlen);
        wlo = max(min(0, kend) - t, -plen);
        if (!feasible) status = WFA_ST_SCORE;
        else if (whi - wlo + 1 > L || pwords > cap || twords > cap) status = WFA_ST_BAND;
      }
    } else if (active) {
      const long long S = budget, o = OE - E;
      const int ak = kend < 0 ? -kend : kend;
      const bool feasible = (ak ? o + (long long)ak * E : 0) <= S;
      const long long a_hi = S - 2 * o + (long long)kend * E, a_lo = S - 2 * o - (long long)kend * E;
      const int kmax0 = max(0, kend), kmin0 = min(0, kend);
      int whi = a_hi >= 0 ? max(kmax0, (int)min((long long)tlen, a_hi / (2 * E))) : kmax0;
      wlo = a_lo >= 0 ? min(kmin0, -(int)min((long long)plen, a_lo / (2 * E))) : kmin0;
      whi = min(whi, tlen); wlo = max(wlo, -plen);
      if (!feasible) status = WFA_ST_SCORE;
      else if (whi - wlo + 1 > L || pwords > cap || twords > cap) status = WFA_ST_BAND;
    }
    // CIGARs: the row table (8 bytes per score up to the budget, in 16-byte units) and one row of L origin bytes per score
    // Arena space WITHOUT atomics: work item w owns the units [top + w * slot, top + (w + 1) * slot) above the arena's bump pointer
    // as the launch found it, slot = what the launch's largest budget needs (wfa_short_bt_slot_units); the host moves the bump
    // pointer past the whole region with a one-thread kernel behind this launch.  (One returning atomic per alignment on the
    // one bump word -- ~88 per microsecond on this chip -- was 0.3 of the 0.43 ms of a 100k-pair launch.)
    uint32_t tab_unit = WFA_ROW_NONE, rows_unit = 0;
    if constexpr (BT) {
      const uint32_t tab_units = (uint32_t)(((long long)p.max_score + 2) >> 1), slot = tab_units + (uint32_t)(p.max_score + 1) * (RL / 16);
      const unsigned long long b = arena_top0 + (unsigned long long)w * slot;
      if (active && status == WFA_ST_DONE) {
        if (b + slot <= p.arena_units) { tab_unit = (uint32_t)b; rows_unit = tab_unit + tab_units; }
        else status = WFA_ST_NOMEM;
      }
    }
    const bool run = active && status == WFA_ST_DONE;
    const int k = wlo + j;                                  // this lane's diagonal, for the whole alignment
    // An offset on diagonal k is inside the matrix -- !(h > tlen || v > plen), h >= 0, v = h - k >= 0: wavefront_compute_affine.c:45-87
    // -- iff max(0, k) <= h <= min(tlen, plen + k): ONE unsigned compare against per-lane constants.  (Two compares and an
    // s_and_b64 left the select behind them with a mask no vector instruction in flight had written: a v_cndmask_b32 that
    // issues once per 23 cycles on this chip instead of 4 -- profiles/r04/valu_classes.txt.)
    const int h_hi = min(tlen, plen + k);
    const int h_lo = h_hi >= max(0, k) ? max(0, k) : INT_MAX / 2;      // (a diagonal that misses the matrix: nothing is inside)
    const uint32_t h_span = (uint32_t)max(h_hi - h_lo, 0);
    // (EF) an end diagonal: a cell at the end of it -- h >= h_hi -- has used up the text with at most pef pattern bases left
    // (kend <= k <= kend + pef, h_hi == tlen) or the pattern with at most tef text bases left (kend - tef <= k <= kend, h_hi == plen + k)
    bool end_lane = false;
    int end_k = 0;                                          // (EF) the diagonal the alignment ended on
    if constexpr (EF) end_lane = k >= kend - tef && k <= kend + pef;
    __builtin_amdgcn_wave_barrier();                        // (one wavefront: LDS operations execute in order)

    // run length from (v, h) on this lane's diagonal, 16 bases per step, wave-uniform continuation
    auto extend = [&](int h, bool ok) -> int {
      const int hmax = min(plen + k, tlen);
      const int v = h - k;
      int rem = ok ? hmax - h : 0;
      const uint32_t* pw = Pw + (ok ? (v >> 4) : 0);
      const uint32_t* tw = Tw + (ok ? (h >> 4) : 0);
      const uint32_t sa = (uint32_t)v << 1, sb = (uint32_t)h << 1;
      // (32 bases per LDS round trip: the loop goes on while ANY lane of the wavefront still matches -- the longest run of four
      // alignments' main diagonals, five or six 16-base steps per score on 150 bp reads at 2 % -- and every step is a dependent
      // LDS read; the waves of this kernel wait, they do not compete for the vector pipe)
      while (__builtin_amdgcn_ballot_w64(rem > 0) != 0ull) {
        const uint32_t p0 = pw[0], p1 = pw[1], p2 = pw[2], t0 = tw[0], t1 = tw[1], t2 = tw[2];
        const uint32_t d0 = __builtin_amdgcn_alignbit(p1, p0, sa) ^ __builtin_amdgcn_alignbit(t1, t0, sb);
        const uint32_t d1 = __builtin_amdgcn_alignbit(p2, p1, sa) ^ __builtin_amdgcn_alignbit(t2, t1, sb);
        const int run32 = d0 ? (__builtin_ctz(d0) >> 1) : 16 + (d1 ? (__builtin_ctz(d1) >> 1) : 16);
        const int n = min(run32, max(rem, 0));
        h += n;
        rem = (n == 32) ? rem - 32 : 0;
        pw += 2; tw += 2;
      }
      return h;
    };

    // score 0
    int m[D];                                               // M of the scores with (s % D) == index
#pragma unroll
    for (int i = 0; i < D; ++i) m[i] = S_NULL;
    int ig[DG], dg[DG];                                     // E == 1: I and D of the last score; else of the scores with (s % D) == index (LIN: unused)
#pragma unroll
    for (int i = 0; i < DG; ++i) { ig[i] = S_NULL; dg[i] = S_NULL; }
    int ig2[TP2 ? E2 : 1], dg2[TP2 ? E2 : 1];               // (TP2) I2 and D2 of the scores with (s % E2) == index
    if constexpr (TP2) {
#pragma unroll
      for (int i = 0; i < E2; ++i) { ig2[i] = S_NULL; dg2[i] = S_NULL; }
    }
    {
      bool mine = run && k == 0;
      int h_start = 0;
      // (EF) the start row: every diagonal of [-pbf, tbf], from the border cell (wavefront_unialign.c:137-178)
      if constexpr (EF) { mine = run && k >= -pbf && k <= tbf; h_start = max(k, 0); }
      const int h = extend(h_start, mine);
      m[0] = mine ? h : S_NULL;
      if constexpr (BT) { if (run) lrows[0] = 0; }
    }
    bool fin = !run;                                        // this lane's group has its result (or never ran)
    int score = -1;
    {
      bool hit = run && k == kend && m[0] >= tlen;
      if constexpr (EF) hit = run && end_lane && m[0] >= h_hi;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
      if (run && (bal & grp_mask) != 0ull) {
        fin = true; score = 0;
        if constexpr (EF) end_k = (int)__builtin_ctzll(bal & grp_mask) - grp * L + wlo;
      }
    }
    int s = 0;
    // one score: reads M[s - X], M[s - OE], I[s - E], D[s - E] from their registers (by value: one of them may be the register written)
    auto step = [&](int& m_out, int& i1, int& d1, const int m_x, const int m_o, const int i_src, const int d_src) {
      ++s;
      const int m_ol = from_below<L>(m_o, j), i_e = from_below<L>(i_src, j), m_or = from_above<L>(m_o, j), d_e = from_above<L>(d_src, j);
      const int ins = max(m_ol, i_e) + 1;
      const int del = max(m_or, d_e);
      const int mis = m_x + 1;
      // !(h > tlen || v > plen), unsigned so that NULLs fail too (wavefront_compute_affine.c:45-87)
      const bool i_ok = (uint32_t)(ins - h_lo) <= h_span;
      const bool d_ok = (uint32_t)(del - h_lo) <= h_span;
      i1 = i_ok ? ins : S_NULL;
      d1 = d_ok ? del : S_NULL;
      const int mv = max(max(d1, i1), mis);
      if constexpr (BT) {
        // tie-breaks: gap extension over gap open (wavefront_compute_affine.c:135-143,153-161); M: mismatch, then deletion, then
        // insertion (wavefront_backtrace.c:48-59).  A group that has its result stores nothing more (its rows end at its budget).
        if (!fin) {
          const uint32_t code = (i_e >= m_ol ? BT_I_EXT : 0u) | (d_e >= m_or ? BT_D_EXT : 0u) |
                                ((mis == mv) ? BT_M_X : ((d1 == mv) ? BT_M_D : BT_M_I));
          lrows[s * RL] = (uint8_t)code;
        }
      }
      const bool ok = !fin & ((uint32_t)(mv - h_lo) <= h_span);
      const int h = extend(mv, ok);
      m_out = ok ? h : S_NULL;
      bool hit = ok && k == kend && h >= tlen;
      // (EF) an M cell at the end of an end diagonal; the LOWEST such diagonal of the group wins, as in step_lin.  I and D values never
      // end an alignment: WFA2 scans the M wavefront (wavefront_extend.c:124-170), and a gap that reaches an end is in M at the same score.
      // The note in front of wfa_short_kernel under a span -- an I (D) value nulled at once because it ran past the end of diagonal k came
      // from a cell at the very end of the text (pattern) on diagonal k - 1 (k + 1) at a lower score, where M is at least as far.  If that
      // neighbour is an end diagonal, the alignment ended there before this score.  If it is not, it lies beyond the interval of end
      // diagonals and so does k: every path from cell (s, k) to ANY end diagonal crosses the neighbour behind an M offset that had
      // reached its end at a lower score, and is dominated.  So the cells where nulling at once and WFA2's trimming differ are on no
      // optimal path to any end diagonal, not only on none to the corner: scores, tie-breaks, end diagonal and CIGAR are WFA2's.
      if constexpr (EF) hit = ok && end_lane && h >= h_hi;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
      if (!fin) {
        if ((bal & grp_mask) != 0ull) {
          fin = true; score = s;
          if constexpr (EF) end_k = (int)__builtin_ctzll(bal & grp_mask) - grp * L + wlo;
        }
        else if (s >= budget) { fin = true; status = WFA_ST_SCORE; }     // (the next score would be past the budget)
      }
    };
    // LIN, one score: reads M[s - X] (not under indel) and M[s - g]
    auto step_lin = [&](int& m_out, const int m_x, const int m_g) {
      ++s;
      const int ins = from_below<L>(m_g, j) + 1;
      const int del = from_above<L>(m_g, j);
      const int mis = X ? m_x + 1 : S_NULL;
      const int mv = max(del, max(mis, ins));
      if constexpr (BT) {
        // mismatch, then deletion, then insertion (loop_careful_lin.inc); never a mismatch under indel
        if (!fin) lrows[s * RL] = (uint8_t)((X && mis == mv) ? BTL_X : ((del == mv) ? BTL_D : BTL_I));
      }
      const bool ok = !fin & ((uint32_t)(mv - h_lo) <= h_span);
      const int h = extend(mv, ok);
      m_out = ok ? h : S_NULL;
      bool hit = ok && k == kend && h >= tlen;
      // (EF) the LOWEST diagonal of the group that ends the alignment wins (wavefront_extend.c:124-170)
      if constexpr (EF) hit = ok && end_lane && h >= h_hi;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
      if (!fin) {
        if ((bal & grp_mask) != 0ull) {
          fin = true; score = s;
          if constexpr (EF) end_k = (int)__builtin_ctzll(bal & grp_mask) - grp * L + wlo;
        }
        else if (s >= budget) { fin = true; status = WFA_ST_SCORE; }
      }
    };
    // TP2, one score (the cells of align/loop_careful_2p.inc: seven sources, five values): reads M[s - X], M[s - OE], M[s - OE2] by value
    // and I1 / D1[s - E], I2 / D2[s - E2] from the ring slots it then writes.  The SOURCE lane takes the max of opening and extension,
    // so each component crosses to its neighbour once: four lane shifts per score instead of eight; with CIGARs the four "extension won
    // or tied" flags (wavefront_compute_affine2p.c:173,191,214,232) cross as two more -- the I flags upwards, the D flags downwards.
    // Lanes without a neighbour get NULL (flags: none -- their gap values are NULL, nobody asks where they came from).
    auto step_2p = [&](int& m_out, int& i1, int& d1, int& i2, int& d2, const int m_x, const int m_o1, const int m_o2) {
      if constexpr (TP2) {
        ++s;
        const int ins1 = short2p_from_below<L>(max(m_o1, i1), j) + 1, ins2 = short2p_from_below<L>(max(m_o2, i2), j) + 1;
        const int del1 = short2p_from_above<L>(max(m_o1, d1), j), del2 = short2p_from_above<L>(max(m_o2, d2), j);
        uint32_t ext = 0;
        if constexpr (BT) {
          const int f_i = (i1 >= m_o1 ? (int)BT2_I1_EXT : 0) | (i2 >= m_o2 ? (int)BT2_I2_EXT : 0);
          const int f_d = (d1 >= m_o1 ? (int)BT2_D1_EXT : 0) | (d2 >= m_o2 ? (int)BT2_D2_EXT : 0);
          ext = (uint32_t)(short2p_from_below<L, 0>(f_i, j) | short2p_from_above<L, 0>(f_d, j));
        }
        const int mis = m_x + 1;
        // !(h > tlen || v > plen), unsigned so that NULLs fail too (wavefront_compute_affine2p.c:46-106); a value past an end is NULL at
        // once (DESIGN.md section 4.16: no cell of an optimal path reads one)
        i1 = ((uint32_t)(ins1 - h_lo) <= h_span) ? ins1 : S_NULL;
        i2 = ((uint32_t)(ins2 - h_lo) <= h_span) ? ins2 : S_NULL;
        d1 = ((uint32_t)(del1 - h_lo) <= h_span) ? del1 : S_NULL;
        d2 = ((uint32_t)(del2 - h_lo) <= h_span) ? del2 : S_NULL;
        const int mv = max(max(max(d2, d1), max(i2, i1)), mis);
        if constexpr (BT) {
          // M on equal offsets: mismatch, D2, D1, I2, I1 (wavefront_compute_affine2p.c:251-270, wavefront_backtrace.c:49-59)
          if (!fin) lrows[s * RL] = (uint8_t)(ext | ((mis == mv) ? BT2_M_X : (d2 == mv) ? BT2_M_D2 : (d1 == mv) ? BT2_M_D1 : (i2 == mv) ? BT2_M_I2 : BT2_M_I1));
        }
        const bool ok = !fin & ((uint32_t)(mv - h_lo) <= h_span);
        const int h = extend(mv, ok);
        m_out = ok ? h : S_NULL;
        const bool hit = ok && k == kend && h >= tlen;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
        if (!fin) {
          if ((bal & grp_mask) != 0ull) { fin = true; score = s; }
          else if (s >= budget) { fin = true; status = WFA_ST_SCORE; }
        }
      }
    };
    // s % D runs 1, 2, .., D - 1, 0, 1, ..: M[s - X] sits in register (s - X) % D, M[s - OE] in (s - OE) % D
    bool more = __builtin_amdgcn_ballot_w64(!fin) != 0ull;
    while (more) {
#pragma unroll
      for (int r = 1; r <= D; ++r) {
        if (more) {
          if constexpr (TP2) step_2p(m[r % D], ig[r % E], dg[r % E], ig2[r % E2], dg2[r % E2], m[(r - X + D) % D], m[(r - OE + D) % D], m[(r - OE2 + D) % D]);
          else if constexpr (LIN) step_lin(m[r % D], m[(r - X + D) % D], m[(r - OE + D) % D]);
          else if constexpr (E == 1) step(m[r % D], ig[0], dg[0], m[(r - X + D) % D], m[(r - OE + D) % D], ig[0], dg[0]);
          else step(m[r % D], ig[r % D], dg[r % D], m[(r - X + D) % D], m[(r - OE + D) % D], ig[(r - E + D) % D], dg[(r - E + D) % D]);
          more = __builtin_amdgcn_ballot_w64(!fin) != 0ull;
        }
      }
    }
    // ---- the sequences of the next iteration: registers -> the other LDS set.  (Before this iteration's results go out: the wait
    // for the loads would otherwise wait for those stores as well -- one counter, in order.)
    stage_seq(Pn, m1, r1, ok1);
    if constexpr (BT) {
      if (run && status == WFA_ST_DONE) {
        // the rows, LDS -> arena: (score + 1) * L bytes in 16-byte pieces (LDS operations of one wavefront execute in order)
        asm volatile("" ::: "memory");
        {
          const uint4* src = reinterpret_cast<const uint4*>(lrows - j);
          uint4* dst = reinterpret_cast<uint4*>(p.arena + (size_t)rows_unit * 16);
          const int n16 = (score + 1) * (RL / 16);
          for (int q = j; q < n16; q += L) dst[q] = src[q];
        }
        // the row table: [score] = {unit of the row, its lower diagonal} (what every tier leaves for the backtrace)
        uint2* tab = reinterpret_cast<uint2*>(p.arena + (size_t)tab_unit * 16);
        for (int t = j; t <= score; t += L) tab[t] = make_uint2(rows_unit + (uint32_t)t * (RL / 16), (uint32_t)wlo);
        if (j == 0) p.bt_final_row[pair] = tab_unit;
      }
    }
    if (active && j == 0) {
      p.score[pair] = (status == WFA_ST_DONE) ? score : -1;
      p.status[pair] = status;
      const uint32_t cells = (status == WFA_ST_DONE) ? (uint32_t)(max(score, 0) + 1) * (uint32_t)L : 0u;
      if (p.cells) p.cells[pair] = cells;
      lane_rows += (status == WFA_ST_DONE) ? (uint32_t)(max(score, 0) + 1) : 0u;
      // (EF) the diagonal the alignment ended on; the one it started on is the backtrace's to find
      if constexpr (EF) { if (status == WFA_ST_DONE) { int32_t* const en = p.ends + 2 * (size_t)pair; en[0] = INT_MIN; en[1] = end_k; } }
    }
    {
      const bool failed = active && j == 0 && p.fail_list && (status == WFA_ST_BAND || status == WFA_ST_SCORE);
      if (failed) p.fail_list[atomicAdd(p.fail_count, 1ull)] = pair;      // (rare)
      n_fail += count_of(failed);
      not_done += count_of(j == 0 && w < n_work && !(active && status == WFA_ST_DONE));      // (skipped pairs -- another class's -- included)
    }
    // ---- everything moves up one stage
    m0 = m1; m1 = m2; pair2 = pair3;
    { uint32_t* const t = Pw; Pw = Pn; Pn = t; }
    __builtin_amdgcn_wave_barrier();
  }
  // cells of this wavefront (the group leaders counted theirs)
  unsigned long long blk_cells = lane_rows;
  for (int d = 32; d > 0; d >>= 1) blk_cells += __shfl_down(blk_cells, d);
  blk_cells *= (unsigned)L;
  if (lane == 0) {
    if (p.wave_parts) {
      ulonglong4* const out = reinterpret_cast<ulonglong4*>(p.wave_parts) + blockIdx.x;
      *out = make_ulonglong4(blk_cells, not_done, n_fail, n_flag);
    }
    else if (blk_cells && p.launch_cells) atomicAdd(p.launch_cells, blk_cells);
  }
