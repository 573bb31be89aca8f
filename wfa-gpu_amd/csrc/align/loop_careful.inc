// loop_careful.inc -- the careful score step: WFA2 to the letter (limits from the trimmed limits of the input rows, missing wavefronts, trimming, termination).
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// One iteration of the score loop: every score of the byte-compare and 32-bit tiers after the first touch, the last few scores of every alignment.
        ++s;
        // (ENDSFREE: the reach interval surrounds an interval of end diagonals and outlives the budget by some scores: said here, the row
        // table holds the scores up to the budget)
        if constexpr (ENDSFREE) { if (s > budget) { status = WFA_ST_SCORE; break; } }
        // (past the budget the reach interval is empty, so that test sits on the "no wavefront" path)
        if (reach_r == 0) { ++rlo; --rhi; reach_r = e - 1; } else --reach_r;
        if constexpr (NW > 1) {
          // reduction slot of the NEXT score (nobody reads it any more: its readers passed barrier s-1)
          if (tid < 8) red[8 * ((s + 1) % 3) + tid] = (tid == 6) ? 0 : ((tid & 1) ? INT_MIN : INT_MAX);
        }
        p_m += rs;  if (p_m == m_end) p_m = m_first;
        p_x += rs;  if (p_x == m_end) p_x = m_first;
        p_oe += rs; if (p_oe == m_end) p_oe = m_first;
        p_ic += rs; if (p_ic == i_end) p_ic = i_first;
        p_ip += rs; if (p_ip == i_end) p_ip = i_first;
        const int bk_s = s & bkm, bk_x = (s - x) & bkm, bk_oe = (s - oe) & bkm, bk_e = (s - e) & bkm;
        // predecessor rows: s-x and s-(o+e) of M, s-e of I and D
        const int a_x = book.get_a(bk_x);
        const int a_oe = book.get_a(bk_oe);
        const int mxlo = range_lo(a_x), mxhi = range_hi(a_x), molo = range_lo(a_oe), mohi = range_hi(a_oe);
        // limits (wavefront_compute.c:41-71; null rows carry lo=1, hi=-1)
        // (the empty asm keeps the chains on the scalar unit: min(min(a,b),c) would be matched to v_min3)
        int lo = min(mxlo, molo - 1), hi = max(mxhi, mohi + 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        bool mx_null = false, mo_null = false, ie_null = false, de_null = false;
        bool all_null = false, have_i = true, have_d = true;
        int ielo, iehi, delo, dehi;
        const bool fast = regular >= dm - 1;
        if (fast) {
          // I and D of s-e span the M limits of s-e: min(lo+1, lo-1), max(hi+1, hi-1)
          const int a_e = book.get_a(bk_e);
          ielo = delo = range_lo(a_e); iehi = dehi = range_hi(a_e);
          lo = min(lo, ielo - 1); hi = max(hi, iehi + 1);
        } else {
          const int bi_e = book.get_i(bk_e);
          const int bd_e = book.get_d(bk_e);
          ielo = range_lo(bi_e); iehi = range_hi(bi_e); delo = range_lo(bd_e); dehi = range_hi(bd_e);
          mx_null = mxlo > mxhi; mo_null = molo > mohi; ie_null = ielo > iehi; de_null = delo > dehi;
          all_null = mx_null && mo_null && ie_null && de_null;
          have_i = !(mo_null && ie_null); have_d = !(mo_null && de_null);
          lo = min(lo, ielo + 1); hi = max(hi, iehi + 1);
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = min(lo, delo - 1); hi = max(hi, dehi - 1);
        }
        {
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = max(lo, wlo); hi = min(hi, whi);
          if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
          lo = max(lo, rlo); hi = min(hi, rhi);
        }
        OffT* out_m = p_m;             // exact mode: [q] = diagonal q
        OffT* out_i = p_ic;
        OffT* out_d = d_of(p_ic);
        if (all_null || lo > hi) {
          // no wavefront at this score (wavefront_compute_affine.c:236-243)
          if (s > budget) { status = WFA_ST_SCORE; break; }
          regular = 0;
          book.set(bk_s, ROW_NONE_A, ROW_NONE_A, ROW_NONE_A);
          if constexpr (BANDED) {
            // (relative rows: the whole slot)
            for (int q = tid; q < p.band_width + 2 * GZ; q += NT) {
              out_m[q] = (OffT)OffNull<OffT>::value; out_i[q] = (OffT)OffNull<OffT>::value; out_d[q] = (OffT)OffNull<OffT>::value;
            }
          } else {
            // the slots this score would have written: clear what their previous occupants left
            const int o_m = book.get_a((s - dm) & bkm), o_e = book.get_a((s - de) & bkm);
            const int f0 = min(range_lo(o_m), range_lo(o_e)), f1 = max(range_hi(o_m), range_hi(o_e));
            for (int q = f0 + tid; q <= f1; q += NT) {
              out_m[q] = (OffT)OffNull<OffT>::value; out_i[q] = (OffT)OffNull<OffT>::value; out_d[q] = (OffT)OffNull<OffT>::value;
            }
          }
          block_sync<NW>();
          continue;
        }
        // (the banded search has a loop of its own above and never gets here)
        const int width = hi - lo + 1;
        ncells += (uint32_t)width;

        uint8_t* codes = nullptr;
        if constexpr (TILED) {
          codes = (uint8_t*)tile_row(s);      // (the alignment owns its block of tiles: nothing to claim, nothing to record)
        } else if constexpr (BT) {
          if (!alloc_row(width)) { status = WFA_ST_NOMEM; break; }
          tab_set(s, row_s, lo);
          codes = p.arena + (size_t)row_s * 16;
        }

        const OffT* row_mx = p_x;
        const OffT* row_mo = p_oe;
        const OffT* row_ie = p_ip;
        const OffT* row_de = d_of(p_ip);

        if constexpr (BANDED) {
          // ring invariant of relative rows: NULL guard zones on both sides of the row, whatever the slot held before
          for (int j = tid; j < 2 * GZ; j += NT) {
            const int q = j < GZ ? j : width + j;
            out_m[q] = (OffT)OffNull<OffT>::value; out_i[q] = (OffT)OffNull<OffT>::value; out_d[q] = (OffT)OffNull<OffT>::value;
          }
        } else {
          // Keep the ring invariant: the M slot last held score s-dm, the I/D slots score s-e-1; whatever
          // those rows had beyond [lo, hi] becomes NULL again (nothing while the wavefront grows).
          const int o_m = book.get_a((s - dm) & bkm), o_e = book.get_a((s - de) & bkm);
          const int f0 = min(range_lo(o_m), range_lo(o_e)), f1 = max(range_hi(o_m), range_hi(o_e));
          const int nlo = max(lo - f0, 0), ntot = nlo + max(f1 - hi, 0);
          if (ntot > 0) {
            for (int j = tid; j < ntot; j += NT) {
              const int q = (j < nlo) ? f0 + j : hi + 1 + (j - nlo);
              out_m[q] = (OffT)OffNull<OffT>::value; out_i[q] = (OffT)OffNull<OffT>::value; out_d[q] = (OffT)OffNull<OffT>::value;
            }
          }
        }

        // ---- the cells of this score.  Lanes past the end recompute cell `hi` (same values, same
        // addresses), so no store needs an exec mask; the only inner loop (extend) is wave-uniform.
        // The vector ALU is the unit this kernel saturates (one integer wave64 instruction holds its
        // SIMD for 4 cycles), so everything uniform is folded into scalar row bases: each LDS address
        // is one v_lshl_add of the diagonal.
        // (banded: a row is stored relative to its own lower limit -- diagonal 0 of a row with limits [lo_r, ..] is column
        // GZ - lo_r of its slot; M, I and D of a score share the mapping; a row that does not exist is read through the
        // mapping of the current one: its slot is NULL all over)
        const int rel_cur = BANDED ? GZ - lo : 0;
        const int rel_x = BANDED ? (mxlo <= mxhi ? GZ - mxlo : rel_cur) : 0;
        const int rel_oe = BANDED ? (molo <= mohi ? GZ - molo : rel_cur) : 0;
        int rel_e = 0;
        if constexpr (BANDED) { const int a_e2 = book.get_a(bk_e); rel_e = range_lo(a_e2) <= range_hi(a_e2) ? GZ - range_lo(a_e2) : rel_cur; }
        const OffT* rb_mx = row_mx + rel_x;          // [k]
        const OffT* rb_mo = row_mo + rel_oe - 1;      // [k] = k-1, [k+2] = k+1
        const OffT* rb_ie = row_ie + rel_e - 1;      // [k] = k-1
        const OffT* rb_de = row_de + rel_e + 1;      // [k] = k+1
        OffT* wb_m = out_m + rel_cur;
        OffT* wb_i = out_i + rel_cur;
        OffT* wb_d = out_d + rel_cur;
        bool my_over = false;
        unsigned long long touch_mask = 0;
        cells_of_score(std::false_type{}, lo, hi, codes, rb_mx, rb_mo, rb_ie, rb_de, wb_m, wb_i, wb_d, my_over, touch_mask);
        // (ENDSFREE) termination (wavefront_extend.c:124-170, 240-262): the LOWEST diagonal of the extended M row whose cell has used up
        // the text with at most pef pattern bases left, or the pattern with at most tef text bases left.  Every wave scans the cells it
        // has just written (same striping as cells_of_score, ascending: its first hit is its lowest); NW > 1: the minimum over the waves
        // through word 0 of the score's reduction slot, under the barrier the score has anyway.
        int my_end = INT_MAX;
        if constexpr (ENDSFREE) {
          const int wave = (NW == 1) ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6);
          for (int k0 = lo; k0 <= hi; k0 += NT) {
            const int kraw = k0 + tid;
            const bool act = kraw <= hi;
            const int k = act ? kraw : hi;
            const int h = (int)wb_m[k], v = h - k;
            const bool hit = act && h >= 0 && ((h >= tlen && plen - v <= pef) || (v >= plen && tlen - h <= tef));
            const unsigned long long bh = __builtin_amdgcn_ballot_w64(hit);
            if (bh) { my_end = k0 + wave * 64 + (int)__builtin_ctzll(bh); break; }
          }
        }
        bool any_over = false;
        {
          const bool wave_over = __builtin_amdgcn_ballot_w64(my_over) != 0ull;
          const bool wave_touch = touch_mask != 0ull;
          if constexpr (NW == 1) {
            block_sync<NW>();
            any_over = wave_over;
            touched_ever |= wave_touch;
            if constexpr (ENDSFREE) end_k = my_end;
          } else {
            int* acc = red + 8 * (s % 3);
            if (lane == 0 && (wave_over || wave_touch)) atomicOr(&acc[6], (wave_over ? 2 : 0) | (wave_touch ? 4 : 0));
            if constexpr (ENDSFREE) { if (lane == 0 && my_end != INT_MAX) atomicMin(&acc[0], my_end); }
            __syncthreads();
            any_over = (acc[6] & 2) != 0;
            touched_ever |= (acc[6] & 4) != 0;
            if constexpr (ENDSFREE) end_k = acc[0];
          }
          // termination (wavefront_extend.c:47-67): every lane reads the same cell
          if constexpr (ENDSFREE) done = end_k != INT_MAX;
          else done = ((unsigned)(kend - lo) <= (unsigned)(hi - lo)) && __builtin_amdgcn_readfirstlane((int)wb_m[kend]) >= tlen;
        }
        // Limits recorded for the row: the computed ones.  Cells that are not valid hold NULL or a
        // negative value, which is all a reader needs; only values past a sequence end need the
        // exact per-component trimming (wavefront_compute.c:570-603): first/last in-range cell.
        if (fast && !any_over) {
          // regular regime goes on: the three components exist and span the computed limits
          const int lim = pack_range(lo, hi);
          ++regular;
          book.set(bk_s, lim, lim, lim);
          last_lo = lo; last_hi = hi;
          if constexpr (NW == 1) block_sync<NW>();
          if (done) break;
          continue;
        }
        int lim_i = have_i ? pack_range(lo, hi) : ROW_NONE_A, lim_d = have_d ? pack_range(lo, hi) : ROW_NONE_A;
        if (any_over) {
          const int wave = (NW == 1) ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6);
          int r[4] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN};
          for (int k0 = lo; k0 <= hi; k0 += NT) {
            const int kraw = k0 + tid;
            const bool active = kraw <= hi;
            const int k = active ? kraw : hi;
            const int iv = have_i ? (int)wb_i[k] : OffNull<OffT>::value;
            const int dv = have_d ? (int)wb_d[k] : OffNull<OffT>::value;
            const bool i_ok = ((unsigned)iv <= (unsigned)tlen) && ((unsigned)(iv - k) <= (unsigned)plen);
            const bool d_ok = ((unsigned)dv <= (unsigned)tlen) && ((unsigned)(dv - k) <= (unsigned)plen);
            const int b = k0 + wave * 64;
            const unsigned long long bi = __ballot(active && i_ok), bd = __ballot(active && d_ok);
            if (bi) { r[0] = min(r[0], b + (int)__builtin_ctzll(bi)); r[1] = max(r[1], b + 63 - (int)__builtin_clzll(bi)); }
            if (bd) { r[2] = min(r[2], b + (int)__builtin_ctzll(bd)); r[3] = max(r[3], b + 63 - (int)__builtin_clzll(bd)); }
          }
          if constexpr (NW > 1) {
            int* acc = red + 8 * (s % 3) + 2;            // words 2..5 of this score's slot are unused so far
            if (lane == 0) {
              if (r[0] <= r[1]) { atomicMin(&acc[0], r[0]); atomicMax(&acc[1], r[1]); }
              if (r[2] <= r[3]) { atomicMin(&acc[2], r[2]); atomicMax(&acc[3], r[3]); }
            }
            __syncthreads();
            r[0] = acc[0]; r[1] = acc[1]; r[2] = acc[2]; r[3] = acc[3];
          }
          if (r[0] > r[1]) { r[0] = ROW_NONE_LO; r[1] = ROW_NONE_HI; }
          if (r[2] > r[3]) { r[2] = ROW_NONE_LO; r[3] = ROW_NONE_HI; }
          lim_i = pack_range(r[0], r[1]); lim_d = pack_range(r[2], r[3]);
          {
            // trimmed-away cells read as NULL from now on (wavefront_compute.c:480-520)
            for (int q = lo + tid; q <= hi; q += NT) {
              if (q < r[0] || q > r[1]) wb_i[q] = (OffT)OffNull<OffT>::value;
              if (q < r[2] || q > r[3]) wb_d[q] = (OffT)OffNull<OffT>::value;
            }
            if constexpr (NW > 1) __syncthreads();
          }
        }
        regular = (have_i && have_d && !any_over) ? regular + 1 : 0;
        book.set(bk_s, pack_range(lo, hi), lim_i, lim_d);
        last_lo = lo; last_hi = hi;
        if constexpr (NW == 1) block_sync<NW>();
        if (done) break;
