// loop_careful_ad.inc -- the careful score step of the wf-adaptive instantiations: WFA2 to the letter, its heuristic cut-off included.
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// One iteration of the score loop.  Against loop_careful.inc:
//   * no pruning: a row is clipped by the sequences ([-plen, tlen]: cells beyond are never valid) and must fit the ring ([wlo, whi], else
//     the pair leaves with status BAND); no window clip, no reach interval -- pruned cells would be missing from min_distance and the scan;
//   * every component carries WFA2's trimmed limits (wavefront_compute.c:570-603: first / last cell inside both sequences), M too: the
//     length test and the scan of the cut-off run over them.  One pass over the cells just written finds the six limits and the
//     smallest distance to the end; every cell outside a component's limits is stored as NULL (wf_elements_init_min/max:
//     wavefront_compute.c:489-560), which is also what keeps the ring invariant;
//   * no regular regime: limits always come from the row book's three words;
//   * the cut-off (wavefront_heuristic.c:508-561) behind the termination test of a score that goes on: see below.
        ++s;
        if (s > budget) { status = WFA_ST_SCORE; break; }
        if constexpr (NW > 1) {
          // reduction slots of the NEXT score (nobody reads them any more: their readers passed barrier s-1)
          if (tid < 8) red[8 * ((s + 1) % 3) + tid] = (tid == 6) ? 0 : ((tid & 1) ? INT_MIN : INT_MAX);
          else if (tid < 10) red2[2 * ((s + 1) % 3) + (tid & 1)] = (tid & 1) ? INT_MIN : INT_MAX;
        }
        p_m += rs;  if (p_m == m_end) p_m = m_first;
        p_x += rs;  if (p_x == m_end) p_x = m_first;
        p_oe += rs; if (p_oe == m_end) p_oe = m_first;
        p_ic += rs; if (p_ic == i_end) p_ic = i_first;
        p_ip += rs; if (p_ip == i_end) p_ip = i_first;
        const int bk_s = s & bkm, bk_x = (s - x) & bkm, bk_oe = (s - oe) & bkm, bk_e = (s - e) & bkm;
        // predecessor rows: s-x and s-(o+e) of M, s-e of I and D, each with its own limits (trimmed, cut off)
        const int a_x = book.get_a(bk_x), a_oe = book.get_a(bk_oe), bi_e = book.get_i(bk_e), bd_e = book.get_d(bk_e);
        const int mxlo = range_lo(a_x), mxhi = range_hi(a_x), molo = range_lo(a_oe), mohi = range_hi(a_oe);
        const int ielo = range_lo(bi_e), iehi = range_hi(bi_e), delo = range_lo(bd_e), dehi = range_hi(bd_e);
        const bool mx_null = mxlo > mxhi, mo_null = molo > mohi, ie_null = ielo > iehi, de_null = delo > dehi;
        const bool all_null = mx_null && mo_null && ie_null && de_null;
        const bool have_i = !(mo_null && ie_null), have_d = !(mo_null && de_null);
        // limits (wavefront_compute.c:41-71; rows that do not exist drop out of the min / max by themselves), then the sequences
        int lo = min(min(mxlo, molo - 1), min(ielo + 1, delo - 1)), hi = max(max(mxhi, mohi + 1), max(iehi + 1, dehi - 1));
        lo = max(lo, -plen); hi = min(hi, tlen);
        OffT* const out_m = p_m;             // [q] = diagonal q
        OffT* const out_i = p_ic;
        OffT* const out_d = d_of(p_ic);
        // what the previous occupants of the three slots (score s-dm of M, s-de of I and D) hold: nothing outside their recorded limits
        const int o_m = book.get_a((s - dm) & bkm), o_i = book.get_i((s - de) & bkm), o_d = book.get_d((s - de) & bkm);
        const int f0 = min(range_lo(o_m), min(range_lo(o_i), range_lo(o_d))), f1 = max(range_hi(o_m), max(range_hi(o_i), range_hi(o_d)));
        if (all_null || lo > hi) {
          // no wavefront at this score (wavefront_compute_affine.c:235-242); more of them in a row than the ring is deep: nothing is
          // left to go on from -- WFA2's "unfeasible" (wavefront_extend.c:368-376), reported like a budget overrun
          if (all_null) { if (++null_steps > dm) { status = WFA_ST_SCORE; break; } } else null_steps = 0;
          book.set(bk_s, ROW_NONE_A, ROW_NONE_A, ROW_NONE_A);
          for (int q = f0 + tid; q <= f1; q += NT) {
            out_m[q] = (OffT)OffNull<OffT>::value; out_i[q] = (OffT)OffNull<OffT>::value; out_d[q] = (OffT)OffNull<OffT>::value;
          }
          block_sync<NW>();
          continue;
        }
        null_steps = 0;
        // the ring holds [wlo, whi] (every row up to the budget fits: align_kernel.hip) and the row book 16-bit limits: a row beyond
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
          for (int j = tid; j < ntot; j += NT) {
            const int q = (j < nlo) ? f0 + j : hi + 1 + (j - nlo);
            out_m[q] = (OffT)OffNull<OffT>::value; out_i[q] = (OffT)OffNull<OffT>::value; out_d[q] = (OffT)OffNull<OffT>::value;
          }
        }
        bool my_over = false;
        unsigned long long touch_mask = 0;
        cells_of_score(std::false_type{}, lo, hi, codes, p_x, p_oe - 1, p_ip - 1, d_of(p_ip) + 1, out_m, out_i, out_d, my_over, touch_mask);

        // ---- one pass over the cells this wave has just written (same striping as cells_of_score): first / last valid cell of M, I
        // and D, and the smallest distance to the end over the M cells, max(plen - v, tlen - h) (wavefront_heuristic.c:125-133; a
        // cell that is not valid -- M holds NULL there -- counts as 2^30, WFA2's -WAVEFRONT_OFFSET_NULL).  NW > 1: through the
        // score's reduction slot (words 0..5 the limits, word 7 the negated distance), under the barrier the score has anyway.
        constexpr int DIST_NULL = 1 << 30;
        const int wave = (NW == 1) ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6);
        int r[6] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN};
        int min_d = DIST_NULL;
        for (int k0 = lo; k0 <= hi; k0 += NT) {
          const int kraw = k0 + tid;
          const bool active = kraw <= hi;
          const int k = active ? kraw : hi;
          const int mv = (int)out_m[k];
          const int iv = have_i ? (int)out_i[k] : OffNull<OffT>::value;
          const int dv = have_d ? (int)out_d[k] : OffNull<OffT>::value;
          const bool m_ok = mv >= 0;      // (cells_of_score stores NULL for an M cell outside the sequences)
          const bool i_ok = ((unsigned)iv <= (unsigned)tlen) && ((unsigned)(iv - k) <= (unsigned)plen);
          const bool d_ok = ((unsigned)dv <= (unsigned)tlen) && ((unsigned)(dv - k) <= (unsigned)plen);
          min_d = min(min_d, m_ok ? max(plen - (mv - k), tlen - mv) : DIST_NULL);
          const int b = k0 + wave * 64;
          const unsigned long long bm = __ballot(active && m_ok), bi = __ballot(active && i_ok), bd = __ballot(active && d_ok);
          if (bm) { r[0] = min(r[0], b + (int)__builtin_ctzll(bm)); r[1] = max(r[1], b + 63 - (int)__builtin_clzll(bm)); }
          if (bi) { r[2] = min(r[2], b + (int)__builtin_ctzll(bi)); r[3] = max(r[3], b + 63 - (int)__builtin_clzll(bi)); }
          if (bd) { r[4] = min(r[4], b + (int)__builtin_ctzll(bd)); r[5] = max(r[5], b + 63 - (int)__builtin_clzll(bd)); }
        }
        for (int off = 32; off; off >>= 1) min_d = min(min_d, __shfl_xor(min_d, off, 64));
        min_d = __builtin_amdgcn_readfirstlane(min_d);
        if constexpr (NW == 1) {
          block_sync<NW>();
        } else {
          int* acc = red + 8 * (s % 3);
          if (lane == 0) {
            if (r[0] <= r[1]) { atomicMin(&acc[0], r[0]); atomicMax(&acc[1], r[1]); }
            if (r[2] <= r[3]) { atomicMin(&acc[2], r[2]); atomicMax(&acc[3], r[3]); }
            if (r[4] <= r[5]) { atomicMin(&acc[4], r[4]); atomicMax(&acc[5], r[5]); }
            atomicMax(&acc[7], -min_d);
          }
          __syncthreads();
          for (int j = 0; j < 6; ++j) r[j] = acc[j];
          min_d = -acc[7];      // (every wave has contributed: never INT_MIN)
        }
        min_d = min(min_d, max(plen, tlen));      // (wavefront_heuristic.c:183)
        // termination (wavefront_extend.c:47-67): every lane reads the same cell
        done = ((unsigned)(kend - lo) <= (unsigned)(hi - lo)) && __builtin_amdgcn_readfirstlane((int)out_m[kend]) >= tlen;
        int mlo = r[0], mhi = r[1], ilo = r[2], ihi = r[3], dlo = r[4], dhi = r[5];
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
          // I and D of the score are narrowed to M's limits (wf_heuristic_equate, :161-172, :549-555: behind every cut-off call that
          // found an M row, due or not); a component that becomes empty no longer exists
          ilo = max(ilo, mlo); ihi = min(ihi, mhi); dlo = max(dlo, mlo); dhi = min(dhi, mhi);
        }
        // cells outside a component's limits read as NULL from now on, for the scores to come and for the backtrace.  (The whole row
        // is looked at.  Visiting only its two ends -- [lo, highest lower limit) and (lowest upper limit, hi], a cell or two each
        // between cut-offs, and no barrier where there is nothing to write -- was measured: 3-4 % SLOWER, EXPERIMENTS.md R9.)
        for (int q = lo + tid; q <= hi; q += NT) {
          if (q < mlo || q > mhi) out_m[q] = (OffT)OffNull<OffT>::value;
          if (q < ilo || q > ihi) out_i[q] = (OffT)OffNull<OffT>::value;
          if (q < dlo || q > dhi) out_d[q] = (OffT)OffNull<OffT>::value;
        }
        block_sync<NW>();
        book.set(bk_s, mlo <= mhi ? pack_range(mlo, mhi) : ROW_NONE_A, ilo <= ihi ? pack_range(ilo, ihi) : ROW_NONE_A, dlo <= dhi ? pack_range(dlo, dhi) : ROW_NONE_A);
        if (done) break;
