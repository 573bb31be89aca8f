// loop_careful_2pad.inc -- the careful score step of the wf-adaptive instantiations under two-piece penalties (ADAPTIVE && TWOPIECE):
// WFA2's gap_affine_2p to the letter, its heuristic cut-off included.
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// One iteration of the score loop.  The cells and the seven-row limit rule are loop_careful_2p.inc's, the semantics loop_careful_ad.inc's:
//   * no pruning: a row is clipped by the sequences ([-plen, tlen]) and must fit the ring ([wlo, whi], else the pair leaves with status
//     BAND); no window clip, no reach interval;
//   * no regular regime: limits always come from the five words the two row books keep per score;
//   * every component carries WFA2's trimmed limits (wavefront_compute.c:570-625), M too.  One pass over the cells just written finds
//     the ten limits and the smallest distance to the end; every cell outside a component's limits is stored as NULL;
//   * the cut-off (wavefront_heuristic.c:508-561) behind the termination test of a score that goes on; under gap_affine_2p it equates
//     I1, D1, I2 and D2 to M's limits (:549-560).
// Reductions over the waves (NW > 1): the score's slot of `red` is RED_W = 12 words here -- words 0..9 the limits of M, I1, D1, I2, D2
// (first, last), word 10 the negated distance --, rotated over three scores and reset one score ahead like the 8-word slot; red2 as
// in loop_careful_ad.inc.  NW == 1: ballots and the wave reduction in registers, no LDS traffic beyond the rows.
        ++s;
        if (s > budget) { status = WFA_ST_SCORE; break; }
        if constexpr (NW > 1) {
          // reduction slots of the NEXT score (nobody reads them any more: their readers passed barrier s-1)
          if (tid < RED_W) red[RED_W * ((s + 1) % 3) + tid] = (tid == RED_W - 1) ? 0 : ((tid & 1) || tid == 10) ? INT_MIN : INT_MAX;
          else if (tid < RED_W + 2) red2[2 * ((s + 1) % 3) + (tid & 1)] = (tid & 1) ? INT_MIN : INT_MAX;
        }
        p_m += rs;   if (p_m == m_end) p_m = m_first;
        p_x += rs;   if (p_x == m_end) p_x = m_first;
        p_oe += rs;  if (p_oe == m_end) p_oe = m_first;
        p_oe2 += rs; if (p_oe2 == m_end) p_oe2 = m_first;
        p_ic += rs;  if (p_ic == i_end) p_ic = i_first;
        p_ip += rs;  if (p_ip == i_end) p_ip = i_first;
        p_ic2 += rs; if (p_ic2 == i2_end) p_ic2 = i2_first;
        p_ip2 += rs; if (p_ip2 == i2_end) p_ip2 = i2_first;
        const int bk_s = s & bkm, bk_x = (s - x) & bkm, bk_oe = (s - oe) & bkm, bk_e = (s - e) & bkm, bk_oe2 = (s - oe2) & bkm, bk_e2 = (s - e2) & bkm;
        // predecessor rows: s-x, s-(o1+e1) and s-(o2+e2) of M, s-e1 of I1 and D1, s-e2 of I2 and D2, each with its own limits (trimmed, cut off)
        const int a_x = book.get_a(bk_x), a_oe = book.get_a(bk_oe), a_oe2 = book.get_a(bk_oe2);
        const int bi1 = book.get_i(bk_e), bd1 = book.get_d(bk_e), bi2 = book2.get_i(bk_e2), bd2 = book2.get_d(bk_e2);
        const int mxlo = range_lo(a_x), mxhi = range_hi(a_x), molo = range_lo(a_oe), mohi = range_hi(a_oe), m2lo = range_lo(a_oe2), m2hi = range_hi(a_oe2);
        const bool mx_null = mxlo > mxhi, mo_null = molo > mohi, m2_null = m2lo > m2hi;
        const bool i1_null = range_lo(bi1) > range_hi(bi1), d1_null = range_lo(bd1) > range_hi(bd1);
        const bool i2_null = range_lo(bi2) > range_hi(bi2), d2_null = range_lo(bd2) > range_hi(bd2);
        const bool all_null = mx_null && mo_null && m2_null && i1_null && d1_null && i2_null && d2_null;
        const bool have_i1 = !(mo_null && i1_null), have_d1 = !(mo_null && d1_null), have_i2 = !(m2_null && i2_null), have_d2 = !(m2_null && d2_null);
        // limits (wavefront_compute.c:41-90; rows that do not exist drop out of the min / max by themselves), then the sequences
        // (the empty asm keeps the chains on the scalar unit: min(min(a,b),c) would be matched to v_min3)
        int lo = min(mxlo, molo - 1), hi = max(mxhi, mohi + 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = min(lo, m2lo - 1); hi = max(hi, m2hi + 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = min(lo, range_lo(bi1) + 1); hi = max(hi, range_hi(bi1) + 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = min(lo, range_lo(bd1) - 1); hi = max(hi, range_hi(bd1) - 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = min(lo, range_lo(bi2) + 1); hi = max(hi, range_hi(bi2) + 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = min(lo, range_lo(bd2) - 1); hi = max(hi, range_hi(bd2) - 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = max(lo, -plen); hi = min(hi, tlen);
        OffT* const out_m = p_m;             // [q] = diagonal q
        OffT* const out_i = p_ic;
        OffT* const out_d = d_of(p_ic);
        OffT* const out_i2 = p_ic2;
        OffT* const out_d2 = d2_of(p_ic2);
        // what the previous occupants of the five slots (score s-dm of M, s-de of I1 and D1, s-de2 of I2 and D2) hold: nothing outside
        // their recorded limits
        int f0, f1;
        {
          const int o_m = book.get_a((s - dm) & bkm), o_i = book.get_i((s - de) & bkm), o_d = book.get_d((s - de) & bkm);
          const int o_i2 = book2.get_i((s - de2) & bkm), o_d2 = book2.get_d((s - de2) & bkm);
          f0 = min(range_lo(o_m), min(range_lo(o_i), range_lo(o_d))); f1 = max(range_hi(o_m), max(range_hi(o_i), range_hi(o_d)));
          f0 = min(f0, min(range_lo(o_i2), range_lo(o_d2))); f1 = max(f1, max(range_hi(o_i2), range_hi(o_d2)));
        }
        auto null_cell = [&](const int q) {
          out_m[q] = (OffT)OffNull<OffT>::value; out_i[q] = (OffT)OffNull<OffT>::value; out_d[q] = (OffT)OffNull<OffT>::value;
          out_i2[q] = (OffT)OffNull<OffT>::value; out_d2[q] = (OffT)OffNull<OffT>::value;
        };
        if (all_null || lo > hi) {
          // no wavefront at this score (wavefront_compute_affine2p.c:340-350); more of them in a row than the ring is deep: nothing is
          // left to go on from -- WFA2's "unfeasible" (wavefront_extend.c:368-376), reported like a budget overrun
          if (all_null) { if (++null_steps > dm) { status = WFA_ST_SCORE; break; } } else null_steps = 0;
          book.set(bk_s, ROW_NONE_A, ROW_NONE_A, ROW_NONE_A);
          book2.set(bk_s, ROW_NONE_A, ROW_NONE_A);
          for (int q = f0 + tid; q <= f1; q += NT) null_cell(q);
          block_sync<NW>();
          continue;
        }
        null_steps = 0;
        // the ring holds [wlo, whi] (every row up to the budget fits: align_kernel.hip) and the row books 16-bit limits: a row beyond
        // either is never clipped, the pair leaves and is escalated
        if (lo < wlo || hi > whi || lo < -ROW_NONE_LO + 2 || hi > ROW_NONE_LO - 2) { status = WFA_ST_BAND; break; }
        const int width = hi - lo + 1;
        ncells += (uint32_t)width;

        uint8_t* codes = nullptr;
        if constexpr (BT) {
          if (!alloc_row(width)) { status = WFA_ST_NOMEM; break; }
          tab_set(s, row_s, lo);      // (rows keep their computed lower limit for addressing, whatever is cut off later)
          codes = p.arena + (size_t)row_s * 16;
        }
        {
          // ring invariant: whatever the previous occupants had beyond [lo, hi] becomes NULL again
          const int nlo = max(lo - f0, 0), ntot = nlo + max(f1 - hi, 0);
          for (int j = tid; j < ntot; j += NT) null_cell((j < nlo) ? f0 + j : hi + 1 + (j - nlo));
        }
        // ---- the cells of this score (cells_generic.inc): [k] of a read base is the diagonal the recurrence wants for cell k
        rb2_mo = p_oe2 - 1;             // [k] = k-1, [k+2] = k+1
        rb2_ie = p_ip2 - 1;             // [k] = k-1
        rb2_de = d2_of(p_ip2) + 1;      // [k] = k+1
        wb2_i = out_i2; wb2_d = out_d2;
        bool my_over = false;
        unsigned long long touch_mask = 0;
        cells_of_score(std::false_type{}, lo, hi, codes, p_x, p_oe - 1, p_ip - 1, d_of(p_ip) + 1, out_m, out_i, out_d, my_over, touch_mask);

        // ---- one pass over the cells this wave has just written (same striping as cells_of_score): first / last valid cell of M, I1,
        // D1, I2 and D2, and the smallest distance to the end over the M cells, max(plen - v, tlen - h) (wavefront_heuristic.c:125-133;
        // a cell that is not valid -- M holds NULL there -- counts as 2^30, WFA2's -WAVEFRONT_OFFSET_NULL).
        constexpr int DIST_NULL = 1 << 30;
        const int wave = (NW == 1) ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6);
        int r[10] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN};
        int min_d = DIST_NULL;
        for (int k0 = lo; k0 <= hi; k0 += NT) {
          const int kraw = k0 + tid;
          const bool active = kraw <= hi;
          const int k = active ? kraw : hi;
          const int mv = (int)out_m[k];
          const int cv[4] = {have_i1 ? (int)out_i[k] : OffNull<OffT>::value, have_d1 ? (int)out_d[k] : OffNull<OffT>::value,
                             have_i2 ? (int)out_i2[k] : OffNull<OffT>::value, have_d2 ? (int)out_d2[k] : OffNull<OffT>::value};
          const bool m_ok = mv >= 0;      // (cells_of_score stores NULL for an M cell outside the sequences)
          min_d = min(min_d, m_ok ? max(plen - (mv - k), tlen - mv) : DIST_NULL);
          const int b = k0 + wave * 64;
          const unsigned long long bm = __ballot(active && m_ok);
          if (bm) { r[0] = min(r[0], b + (int)__builtin_ctzll(bm)); r[1] = max(r[1], b + 63 - (int)__builtin_clzll(bm)); }
          #pragma unroll
          for (int c = 0; c < 4; ++c) {
            const bool c_ok = ((unsigned)cv[c] <= (unsigned)tlen) && ((unsigned)(cv[c] - k) <= (unsigned)plen);
            const unsigned long long bc = __ballot(active && c_ok);
            if (bc) { r[2 + 2 * c] = min(r[2 + 2 * c], b + (int)__builtin_ctzll(bc)); r[3 + 2 * c] = max(r[3 + 2 * c], b + 63 - (int)__builtin_clzll(bc)); }
          }
        }
        for (int off = 32; off; off >>= 1) min_d = min(min_d, __shfl_xor(min_d, off, 64));
        min_d = __builtin_amdgcn_readfirstlane(min_d);
        if constexpr (NW == 1) {
          block_sync<NW>();
        } else {
          int* acc = red + RED_W * (s % 3);
          if (lane == 0) {
            #pragma unroll
            for (int c = 0; c < 5; ++c) if (r[2 * c] <= r[2 * c + 1]) { atomicMin(&acc[2 * c], r[2 * c]); atomicMax(&acc[2 * c + 1], r[2 * c + 1]); }
            atomicMax(&acc[10], -min_d);
          }
          __syncthreads();
          #pragma unroll
          for (int j = 0; j < 10; ++j) r[j] = acc[j];
          min_d = -acc[10];      // (every wave has contributed: never INT_MIN)
        }
        min_d = min(min_d, max(plen, tlen));      // (wavefront_heuristic.c:183)
        // termination (wavefront_extend.c:47-67): every lane reads the same cell
        done = ((unsigned)(kend - lo) <= (unsigned)(hi - lo)) && __builtin_amdgcn_readfirstlane((int)out_m[kend]) >= tlen;
        int mlo = r[0], mhi = r[1];
        // ---- the cut-off (wavefront_heuristic_cufoff).  A score without M cells returns at once, the counter untouched.
        if (!done && mlo <= mhi) {
          --steps_wait;
          if (steps_wait <= 0 && mhi - mlo + 1 >= p.ad_min_len) {
            // first and last diagonal of the row that lags at most the threshold behind the closest one: two ballot scans in one pass
            // (NW > 1: minimum and maximum over the waves through this score's words of red2, one barrier more)
            const int thr = p.ad_max_dist;
            int f = INT_MAX, l = INT_MIN;
            for (int k0 = mlo; k0 <= mhi; k0 += NT) {
              const int kraw = k0 + tid;
              const bool active = kraw <= mhi;
              const int k = active ? kraw : mhi;
              const int mv = (int)out_m[k];
              const int dist = mv >= 0 ? max(plen - (mv - k), tlen - mv) : DIST_NULL;
              const unsigned long long bw = __ballot(active && dist - min_d <= thr);
              const int b = k0 + wave * 64;
              if (bw) { f = min(f, b + (int)__builtin_ctzll(bw)); l = max(l, b + 63 - (int)__builtin_clzll(bw)); }
            }
            if constexpr (NW > 1) {
              int* acc2 = red2 + 2 * (s % 3);
              if (lane == 0 && f <= l) { atomicMin(&acc2[0], f); atomicMax(&acc2[1], l); }
              __syncthreads();
              f = acc2[0]; l = acc2[1];
            }
            // lo moves up past every diagonal that lags more, but not past min(kend, hi); hi moves down likewise, not past
            // max(kend, lo): the target diagonal is preserved (wavefront_heuristic.c:232-256)
            const int nlo = min(f, max(mlo, min(kend, mhi)));
            const int nhi = max(l, min(mhi, max(kend, nlo)));
            mlo = nlo; mhi = nhi;
            steps_wait = p.ad_steps;
          }
          // I1, D1, I2 and D2 of the score are narrowed to M's limits (wf_heuristic_equate, :161-172, :549-560: behind every cut-off
          // call that found an M row, due or not); a component that becomes empty no longer exists
          #pragma unroll
          for (int c = 1; c < 5; ++c) { r[2 * c] = max(r[2 * c], mlo); r[2 * c + 1] = min(r[2 * c + 1], mhi); }
        }
        // cells outside a component's limits read as NULL from now on, for the scores to come and for the backtrace
        for (int q = lo + tid; q <= hi; q += NT) {
          if (q < mlo || q > mhi) out_m[q] = (OffT)OffNull<OffT>::value;
          if (q < r[2] || q > r[3]) out_i[q] = (OffT)OffNull<OffT>::value;
          if (q < r[4] || q > r[5]) out_d[q] = (OffT)OffNull<OffT>::value;
          if (q < r[6] || q > r[7]) out_i2[q] = (OffT)OffNull<OffT>::value;
          if (q < r[8] || q > r[9]) out_d2[q] = (OffT)OffNull<OffT>::value;
        }
        block_sync<NW>();
        book.set(bk_s, mlo <= mhi ? pack_range(mlo, mhi) : ROW_NONE_A, r[2] <= r[3] ? pack_range(r[2], r[3]) : ROW_NONE_A, r[4] <= r[5] ? pack_range(r[4], r[5]) : ROW_NONE_A);
        book2.set(bk_s, r[6] <= r[7] ? pack_range(r[6], r[7]) : ROW_NONE_A, r[8] <= r[9] ? pack_range(r[8], r[9]) : ROW_NONE_A);
        if (done) break;
