// loop_careful_2p.inc -- the careful score step of the two-piece instantiations (TWOPIECE): WFA2's gap_affine_2p to the letter.
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// One iteration of the score loop: every score of a two-piece alignment.  It is loop_careful.inc with five components: limits from
// the trimmed limits of SEVEN input rows (wavefront_compute.c:41-90), a component exists when one of its two inputs does
// (:440-485), the wavefront is missing when all seven are (wavefront_compute_affine2p.c:340-350), end trimming for I1, D1, I2 and D2
// (wavefront_compute.c:570-625), termination as for gap-affine (wavefront_extend.c:47-67).  The limits of I2 and D2 live in book2.
        ++s;
        // (past the budget the reach interval is empty, so that test sits on the "no wavefront" path; e_reach: align_kernel.hip)
        if (reach_r == 0) { ++rlo; --rhi; reach_r = e_reach - 1; } else --reach_r;
        if constexpr (NW > 1) {
          // reduction slot of the NEXT score (nobody reads it any more: its readers passed barrier s-1)
          if (tid < 8) red[8 * ((s + 1) % 3) + tid] = (tid == 6) ? 0 : ((tid & 1) ? INT_MIN : INT_MAX);
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
        // predecessor rows: s-x, s-(o1+e1) and s-(o2+e2) of M, s-e1 of I1 and D1, s-e2 of I2 and D2
        const int a_x = book.get_a(bk_x), a_oe = book.get_a(bk_oe), a_oe2 = book.get_a(bk_oe2);
        const int mxlo = range_lo(a_x), mxhi = range_hi(a_x), molo = range_lo(a_oe), mohi = range_hi(a_oe), m2lo = range_lo(a_oe2), m2hi = range_hi(a_oe2);
        // (the empty asm keeps the chains on the scalar unit: min(min(a,b),c) would be matched to v_min3)
        int lo = min(mxlo, molo - 1), hi = max(mxhi, mohi + 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = min(lo, m2lo - 1); hi = max(hi, m2hi + 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        bool all_null = false, have_i1 = true, have_d1 = true, have_i2 = true, have_d2 = true;
        // the "regular" regime: the last dm - 1 scores had all five components with untrimmed limits
        const bool fast = regular >= dm - 1;
        if (fast) {
          const int a_e = book.get_a(bk_e), a_e2 = book.get_a(bk_e2);
          lo = min(lo, range_lo(a_e) - 1); hi = max(hi, range_hi(a_e) + 1);
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = min(lo, range_lo(a_e2) - 1); hi = max(hi, range_hi(a_e2) + 1);
        } else {
          const int bi1 = book.get_i(bk_e), bd1 = book.get_d(bk_e), bi2 = book2.get_i(bk_e2), bd2 = book2.get_d(bk_e2);
          const bool mx_null = mxlo > mxhi, mo_null = molo > mohi, m2_null = m2lo > m2hi;
          const bool i1_null = range_lo(bi1) > range_hi(bi1), d1_null = range_lo(bd1) > range_hi(bd1);
          const bool i2_null = range_lo(bi2) > range_hi(bi2), d2_null = range_lo(bd2) > range_hi(bd2);
          all_null = mx_null && mo_null && m2_null && i1_null && d1_null && i2_null && d2_null;
          have_i1 = !(mo_null && i1_null); have_d1 = !(mo_null && d1_null); have_i2 = !(m2_null && i2_null); have_d2 = !(m2_null && d2_null);
          lo = min(lo, range_lo(bi1) + 1); hi = max(hi, range_hi(bi1) + 1);
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = min(lo, range_lo(bd1) - 1); hi = max(hi, range_hi(bd1) - 1);
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = min(lo, range_lo(bi2) + 1); hi = max(hi, range_hi(bi2) + 1);
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = min(lo, range_lo(bd2) - 1); hi = max(hi, range_hi(bd2) - 1);
        }
        {
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = max(lo, wlo); hi = min(hi, whi);
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = max(lo, rlo); hi = min(hi, rhi);
        }
        OffT* const out_m = p_m;             // [q] = diagonal q
        OffT* const out_i = p_ic;
        OffT* const out_d = d_of(p_ic);
        OffT* const out_i2 = p_ic2;
        OffT* const out_d2 = d2_of(p_ic2);
        // what the previous occupants of the five slots (the rows of s-dm, s-de and s-de2) had: their computed limits
        const int o_m = book.get_a((s - dm) & bkm), o_e = book.get_a((s - de) & bkm), o_e2 = book.get_a((s - de2) & bkm);
        const int f0 = min(range_lo(o_m), min(range_lo(o_e), range_lo(o_e2))), f1 = max(range_hi(o_m), max(range_hi(o_e), range_hi(o_e2)));
        auto null_cell = [&](const int q) {
          out_m[q] = (OffT)OffNull<OffT>::value; out_i[q] = (OffT)OffNull<OffT>::value; out_d[q] = (OffT)OffNull<OffT>::value;
          out_i2[q] = (OffT)OffNull<OffT>::value; out_d2[q] = (OffT)OffNull<OffT>::value;
        };
        if (all_null || lo > hi) {
          // no wavefront at this score (wavefront_compute_affine2p.c:340-350)
          if (s > budget) { status = WFA_ST_SCORE; break; }
          regular = 0;
          book.set(bk_s, ROW_NONE_A, ROW_NONE_A, ROW_NONE_A);
          book2.set(bk_s, ROW_NONE_A, ROW_NONE_A);
          // the slots this score would have written: clear what their previous occupants left
          for (int q = f0 + tid; q <= f1; q += NT) null_cell(q);
          block_sync<NW>();
          continue;
        }
        const int width = hi - lo + 1;
        ncells += (uint32_t)width;

        uint8_t* codes = nullptr;
        if constexpr (BT) {
          if (!alloc_row(width)) { status = WFA_ST_NOMEM; break; }
          tab_set(s, row_s, lo);
          codes = p.arena + (size_t)row_s * 16;
        }
        {
          // Keep the ring invariant: whatever the previous occupants had beyond [lo, hi] becomes NULL again
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
        bool any_over = false;
        {
          const bool wave_over = __builtin_amdgcn_ballot_w64(my_over) != 0ull;
          if constexpr (NW == 1) {
            block_sync<NW>();
            any_over = wave_over;
          } else {
            int* acc = red + 8 * (s % 3);
            if (lane == 0 && wave_over) atomicOr(&acc[6], 2);
            __syncthreads();
            any_over = (acc[6] & 2) != 0;
          }
          // termination (wavefront_extend.c:47-67): every lane reads the same cell
          done = ((unsigned)(kend - lo) <= (unsigned)(hi - lo)) && __builtin_amdgcn_readfirstlane((int)out_m[kend]) >= tlen;
        }
        // Limits recorded for the row: the computed ones.  Cells that are not valid hold NULL or a negative value, which is all a
        // reader needs; only values past a sequence end need the exact per-component trimming: first / last in-range cell.
        const int lim = pack_range(lo, hi);
        if (fast && !any_over) {
          // the regular regime goes on: the five components exist and span the computed limits
          ++regular;
          book.set(bk_s, lim, lim, lim);
          book2.set(bk_s, lim, lim);
          if constexpr (NW == 1) block_sync<NW>();
          if (done) break;
          continue;
        }
        int lim_c[4] = {have_i1 ? lim : ROW_NONE_A, have_d1 ? lim : ROW_NONE_A, have_i2 ? lim : ROW_NONE_A, have_d2 ? lim : ROW_NONE_A};
        if (any_over) {
          // first and last cell of each gap component that lies inside both sequences; two components per round (NW > 1: words 2..5 of
          // the score's reduction slot carry one round, re-initialised in between -- this path is the last few scores of an alignment)
          const int wave = (NW == 1) ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6);
          for (int round = 0; round < 2; ++round) {
            OffT* const row_i = round ? out_i2 : out_i;
            OffT* const row_d = round ? out_d2 : out_d;
            const bool hv_i = round ? have_i2 : have_i1, hv_d = round ? have_d2 : have_d1;
            int r[4] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN};
            for (int k0 = lo; k0 <= hi; k0 += NT) {
              const int kraw = k0 + tid;
              const bool active = kraw <= hi;
              const int k = active ? kraw : hi;
              const int iv = hv_i ? (int)row_i[k] : OffNull<OffT>::value;
              const int dv = hv_d ? (int)row_d[k] : OffNull<OffT>::value;
              const bool i_ok = ((unsigned)iv <= (unsigned)tlen) && ((unsigned)(iv - k) <= (unsigned)plen);
              const bool d_ok = ((unsigned)dv <= (unsigned)tlen) && ((unsigned)(dv - k) <= (unsigned)plen);
              const int b = k0 + wave * 64;
              const unsigned long long bi = __ballot(active && i_ok), bd = __ballot(active && d_ok);
              if (bi) { r[0] = min(r[0], b + (int)__builtin_ctzll(bi)); r[1] = max(r[1], b + 63 - (int)__builtin_clzll(bi)); }
              if (bd) { r[2] = min(r[2], b + (int)__builtin_ctzll(bd)); r[3] = max(r[3], b + 63 - (int)__builtin_clzll(bd)); }
            }
            if constexpr (NW > 1) {
              int* acc = red + 8 * (s % 3) + 2;
              if (lane == 0) {
                if (r[0] <= r[1]) { atomicMin(&acc[0], r[0]); atomicMax(&acc[1], r[1]); }
                if (r[2] <= r[3]) { atomicMin(&acc[2], r[2]); atomicMax(&acc[3], r[3]); }
              }
              __syncthreads();
              r[0] = acc[0]; r[1] = acc[1]; r[2] = acc[2]; r[3] = acc[3];
              __syncthreads();      // (everybody has read the round's result: the words can be set up for the next round)
              if (round == 0 && tid < 4) acc[tid] = (tid & 1) ? INT_MIN : INT_MAX;
              __syncthreads();
            }
            if (r[0] > r[1]) { r[0] = ROW_NONE_LO; r[1] = ROW_NONE_HI; }
            if (r[2] > r[3]) { r[2] = ROW_NONE_LO; r[3] = ROW_NONE_HI; }
            lim_c[2 * round] = pack_range(r[0], r[1]); lim_c[2 * round + 1] = pack_range(r[2], r[3]);
            // trimmed-away cells read as NULL from now on (wavefront_compute.c:480-520)
            for (int q = lo + tid; q <= hi; q += NT) {
              if (q < r[0] || q > r[1]) row_i[q] = (OffT)OffNull<OffT>::value;
              if (q < r[2] || q > r[3]) row_d[q] = (OffT)OffNull<OffT>::value;
            }
          }
          if constexpr (NW > 1) __syncthreads();
        }
        regular = (have_i1 && have_d1 && have_i2 && have_d2 && !any_over) ? regular + 1 : 0;
        book.set(bk_s, lim, lim_c[0], lim_c[1]);
        book2.set(bk_s, lim_c[2], lim_c[3]);
        if constexpr (NW == 1) block_sync<NW>();
        if (done) break;
