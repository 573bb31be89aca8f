// loop_careful_lin.inc -- the careful score step of the LINEAR instantiations (edit, indel, gap-linear): WFA2 to the letter, one component.
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
//   M[s][k] = max(M[s-x][k] + 1, M[s-g][k-1] + 1, M[s-g][k+1])      (wavefront_compute_linear.c:45-74; g = e = oe here)
//   indel (x == WFA_LIN_NO_MISMATCH): no first term                               (wavefront_compute_edit.c:45-71)
// nulled where h > tlen or v > plen, then extended.  Limits: min / max over the two input rows (wavefront_compute.c:41-60; edit and
// indel: [lo(s-1) - 1, hi(s-1) + 1], wavefront_compute_edit.c:340-343, which is the same rule with x == g or without the mismatch row),
// clipped by window and reach.  The row book records the limits as computed: a cell WFA2 trims from an end of a row
// (wavefront_compute.c:570-603) is not valid, holds NULL here, and so does every cell that only such cells lead to -- the rows here
// are supersets of WFA2's with NULL in the surplus, which is all a reader needs.  (WFA2's exact pruning of wide edit rows,
// wavefront_compute_edit.c:216-271, drops diagonals that lie on no optimal path: not restated, DESIGN.md section 4.9.)
// Origin byte (ROWS in every tier): BTL_X / BTL_D / BTL_I by WFA2's priority on equal offsets (wavefront_backtrace.c:259-264).
// Three reads and one store per cell; under indel two reads.
        ++s;
        // (ENDSFREE: the reach interval surrounds an interval of end diagonals and outlives the budget by some scores: said here, the row
        // table holds the scores up to the budget)
        if constexpr (ENDSFREE) { if (s > budget) { status = WFA_ST_SCORE; break; } }
        if constexpr (ENDSFREE && NW > 1) {
          // word 0 of the reduction slot of the NEXT score (nobody reads it any more: its readers -- of score s-2 -- passed barrier s-1)
          if (tid == 0) red[8 * ((s + 1) % 3)] = INT_MAX;
        }
        if (reach_r == 0) { ++rlo; --rhi; reach_r = e - 1; } else --reach_r;
        const bool indel = x >= WFA_LIN_NO_MISMATCH;      // (wave-uniform: a kernel argument)
        p_m += rs;  if (p_m == m_end) p_m = m_first;
        p_x += rs;  if (p_x == m_end) p_x = m_first;
        p_oe += rs; if (p_oe == m_end) p_oe = m_first;
        const int bk_s = s & bkm;
        // predecessor rows: s-x (not under indel) and s-g
        const int a_x = indel ? ROW_NONE_A : book.get_a((s - x) & bkm);
        const int a_g = book.get_a((s - e) & bkm);
        const int mxlo = range_lo(a_x), mxhi = range_hi(a_x), mglo = range_lo(a_g), mghi = range_hi(a_g);
        int lo = min(mxlo, mglo - 1), hi = max(mxhi, mghi + 1);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = max(lo, wlo); hi = min(hi, whi);
        if constexpr (NW == 1) asm volatile("" : "+s"(lo), "+s"(hi));
        lo = max(lo, rlo); hi = min(hi, rhi);
        OffT* const out_m = p_m;             // [q] = diagonal q
        // the slot last held score s-dm: whatever that row had beyond [lo, hi] becomes NULL again (ring invariant)
        const int o_m = book.get_a((s - dm) & bkm);
        const int f0 = range_lo(o_m), f1 = range_hi(o_m);
        if (lo > hi) {
          // no wavefront at this score (both input rows missing, wavefront_compute_linear.c:172-177; or nothing left inside window and
          // reach -- past the budget the reach interval is empty)
          if (s > budget) { status = WFA_ST_SCORE; break; }
          book.set(bk_s, ROW_NONE_A, ROW_NONE_A, ROW_NONE_A);
          for (int q = f0 + tid; q <= f1; q += NT) out_m[q] = (OffT)OffNull<OffT>::value;
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
          const int nlo = max(lo - f0, 0), ntot = nlo + max(f1 - hi, 0);
          for (int j = tid; j < ntot; j += NT) {
            const int q = (j < nlo) ? f0 + j : hi + 1 + (j - nlo);
            out_m[q] = (OffT)OffNull<OffT>::value;
          }
        }
        // (ENDSFREE) termination (wavefront_extend.c:124-170, 240-262): the LOWEST diagonal of the extended row whose cell has used up the
        // text with at most pef pattern bases left, or the pattern with at most tef text bases left.  Every wave tests the cells it
        // writes, as it writes them (the chunks ascend: its first hit is its lowest); NW > 1: the minimum over the waves below.
        int my_end = INT_MAX;
        // ---- the cells of this score.  Lanes past the end recompute cell `hi` (same values, same addresses), so no store needs an exec
        // mask.  (x == g, and so edit: p_x and p_oe are the same row.)
        {
          const OffT* const rb_mx = indel ? p_oe : p_x;       // [k]      (indel: read, never used)
          const OffT* const rb_mg = p_oe;                      // [k-1], [k+1]
          constexpr int SH = RAW ? 2 : 4, PER = 1 << SH, BITS = RAW ? 3 : 1;
          for (int k0 = lo; k0 <= hi; k0 += NT) {
            const int k = min(k0 + tid, hi);
            const int m_l = (int)rb_mg[k - 1], m_r = (int)rb_mg[k + 1];
            const int m_x = indel ? (int)OffNull<OffT>::value : (int)rb_mx[k];
            const int ins = m_l + 1, del = m_r, mis = m_x + 1;
            const int mv0 = max(del, max(mis, ins));
            uint32_t code = 0;
            if constexpr (BT) code = (!indel && mis == mv0) ? BTL_X : ((del == mv0) ? BTL_D : BTL_I);
            // !(h > tlen || v > plen), unsigned so that negatives fail too
            const bool ok = ((unsigned)mv0 <= (unsigned)tlen) & ((unsigned)(mv0 - k) <= (unsigned)plen);
            // extend (wavefront_extend.c:174-199): the cells that are not valid idle along with nothing left to match
            int h = mv0;
            const int hmax = min(plen + k, tlen);
            int left = ok ? hmax - h : 0;
            {
              // (a cell that is not valid reads the first words of the sequences: its offset is no address)
              const int v = ok ? mv0 - k : 0, h_at = ok ? h : 0;
              const char* pp = reinterpret_cast<const char*>(Pw + (v >> SH));
              const char* tp = reinterpret_cast<const char*>(Tw + (h_at >> SH));
              const uint32_t sa = (uint32_t)v << BITS, sb = (uint32_t)h_at << BITS;
              while (__builtin_amdgcn_ballot_w64(left > 0) != 0ull) {
                const uint32_t* pw = reinterpret_cast<const uint32_t*>(pp);
                const uint32_t* tw = reinterpret_cast<const uint32_t*>(tp);
                const uint32_t d = left > 0 ? (__builtin_amdgcn_alignbit(pw[1], pw[0], sa) ^ __builtin_amdgcn_alignbit(tw[1], tw[0], sb)) : 1u;
                const int nn = min(min(d ? (int)((uint32_t)__builtin_ctz(d) >> BITS) : PER, PER), max(left, 0));
                h += nn;
                left = (nn == PER) ? left - PER : 0;
                if (left > 0) { pp += 4; tp += 4; }
              }
            }
            const int mv = ok ? h : OffNull<OffT>::value;
            out_m[k] = (OffT)mv;
            if constexpr (BT) codes[(uint32_t)(k - lo)] = (uint8_t)code;
            if constexpr (ENDSFREE) {
              // (a cell that WFA2 trims holds NULL here: `ok` keeps it out)
              const int vv = mv - k;
              const bool hit = (k0 + tid <= hi) && ok && ((mv >= tlen && plen - vv <= pef) || (vv >= plen && tlen - mv <= tef));
              const unsigned long long bh = __builtin_amdgcn_ballot_w64(hit);
              if (bh && my_end == INT_MAX) my_end = k0 + (tid & ~63) + (int)__builtin_ctzll(bh);
            }
          }
        }
        if constexpr (ENDSFREE) {
          // the one barrier of the score carries the minimum over the waves: word 0 of the score's reduction slot (three slots in
          // rotation, reset two scores ahead: above)
          if constexpr (NW == 1) {
            block_sync<NW>();
            end_k = my_end;
          } else {
            int* acc = red + 8 * (s % 3);
            if (lane == 0 && my_end != INT_MAX) atomicMin(&acc[0], my_end);
            __syncthreads();
            end_k = acc[0];
          }
          done = end_k != INT_MAX;
        } else {
        // termination (wavefront_extend.c:47-67): every lane reads the same cell, behind the one barrier of the score
        block_sync<NW>();
        done = ((unsigned)(kend - lo) <= (unsigned)(hi - lo)) && __builtin_amdgcn_readfirstlane((int)out_m[kend]) >= tlen;
        }
        book.set(bk_s, pack_range(lo, hi), ROW_NONE_A, ROW_NONE_A);
        last_lo = lo; last_hi = hi;
        // (NW > 1: the book entry is a same-value store of every thread, each reads back its own)
        if (done) break;
