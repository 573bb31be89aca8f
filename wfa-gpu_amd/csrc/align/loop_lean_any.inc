// loop_lean_any.inc -- lean score loop, any gap extension e > 1 (exact 16-bit LDS tiers: 0, 1, 2 and the hybrid ring): limits carried along, no row book.
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// Same contract as loop_lean_e1.inc: runs from the current score until a cell touches a sequence end, the reach interval empties or the
// arena is exhausted; then hands the general state (s, limits, row pointers, row book, reach) back to the careful loop.
        // ---- lean path, any gap extension.  Through round 5 this loop took its limits from the row book (three reads, unpacked,
        // min / max over them: wavefront_compute.c:41-71 to the letter), handled scores without a wavefront, re-NULLed the guard
        // cells and advanced five ring pointers at every score: ~80 cycles of a CU per score against the ~35 of the e == 1 loop --
        // 1M x 1 kbp pairs under (5,3,2) at 292 G cells/s, under (3,1,4) at 148, against 575 under (2,3,1)
        // (profiles/r06/penalty_sets_before.txt).  The reference's kernels are penalty-agnostic (one next_MDI for any x, o, e:
        // lib/kernels/sequence_distance_kernel.cu:57-160); now this loop is the e == 1 loop with two counters more.
        //
        // Limits.  No wavefront of score s reaches beyond diagonal +-floor((s - o) / e) (s >= o + e; 0 before): by induction over
        // hi(s) = max(hi(s-x), hi(s-o-e) + 1, hi(s-e) + 1).  The loop computes the rows over THAT interval -- clipped by the window and
        // by the budget's reach like every row -- instead of WFA2's own limits, which are narrower by a parity fringe of up to x / e + 1
        // diagonals a side and miss whole scores (no combination of the penalties adds up to them).  The extra cells are not valid
        // cells: every predecessor of a cell outside WFA2's limits lies outside ITS row's WFA2 limits (WFA2's limits are the union of
        // what the predecessor rows can reach), hence is NULL by induction, or lies beyond what its row was computed with, hence is
        // NULL by the ring invariant; a NULL plus one per score stays negative.  Valid cells get WFA2's values and origin bytes, the
        // backtrace only ever visits valid cells, and a NULL never equals a run limit (no false "touched").  Same argument as the
        // e == 1 loop's, which computes [-s, s]; SURVEY.md A.1.  A score WFA2 has no wavefront for is a row of NULL cells here.
        // The interval grows by one diagonal a side every e scores (one counter), the reach interval shrinks alike (reach_r).
        if constexpr (HOT && !BANDED && !ENDSFREE) {
          if (e != 1 && !touched_ever) {
            const int s_in = s;
            const int o_pen = oe - e;
            // half-width of the superset interval at s_in and the scores left until it grows next (it grows at s = oe, oe + e, ...)
            int u_w = s_in >= oe ? (s_in - o_pen) / e : 0;
            int g_cnt = s_in >= oe ? e - (s_in - o_pen) % e : oe - s_in;
            // first score at which a limit may move inwards (the reach bound catches up with the window or with the growing front:
            // computed on the safe side, a few scores early); from then on the slots written hold cells beyond the new limits
            int s_clear = INT_MAX;
            if (bounded) {
              const int lo_a = budget - e * (kend - wlo) + 1, lo_b = (budget + o_pen - e * (kend + 1)) / 2 + 1;
              const int hi_a = budget - e * (whi - kend) + 1, hi_b = (budget + o_pen + e * (kend - 1)) / 2 + 1;
              s_clear = min(min(lo_a, lo_b), min(hi_a, hi_b)) - 2 * e - 2;
            }
            s_clear = __builtin_amdgcn_readfirstlane(s_clear);
            const uint32_t rsb = (uint32_t)rs * 2u;
            const uint32_t a_first = lds_addr(m_first), a_end = lds_addr(m_end), ai_first = lds_addr(i_first), ai_end = lds_addr(i_end);
            uint32_t a_m = lds_addr(p_m), a_x = lds_addr(p_x), a_oe = lds_addr(p_oe), a_ic = lds_addr(p_ic), a_ip = lds_addr(p_ip);
            // the D row of an I row: further up in LDS, or (hybrid ring) the same offset into the global D ring
            uint32_t d_delta = HYBRID ? 0u - ai_first : (uint32_t)(de * rs) * 2u;
            uint32_t pw_addr = lds_addr(Pw), tw_addr = lds_addr(Tw), a_hm = lds_addr(hm_row0);
            asm volatile("" : "+s"(pw_addr), "+s"(tw_addr), "+s"(a_hm), "+s"(d_delta));
            int lo = last_lo, hi = last_hi;
            int f_lo = max(wlo, rlo), f_hi = min(whi, rhi);      // (window and reach together: both only ever move inwards)
            unsigned long long touch = 0;
            uint32_t a_last = a_m;
            GlobalBytes code_addr = nullptr;
            uint32_t need_prev = 0;
            if constexpr (TILED) code_addr = tile_row(s);      // (the tile row of the current score: a scalar)
            else if constexpr (BT) code_addr = (GlobalBytes)(uintptr_t)p.arena + ((size_t)chunk_cur * 16u + (uint32_t)stid);
            const uint32_t tile_pitch = tile_cols * 64u - 48u;      // (TILED: from in-tile row 3 of a group to row 0 of the next)
            if constexpr (NW > 1) {
              if (tid == 0) { *touch_flag(0) = 0u; *touch_flag(1) = 0u; }
              __syncthreads();
            }
            const bool far_is_oe = oe >= x;
            // why the loop ends: 1 = the reach interval is empty, 2 = arena exhausted, 3 = a cell touched a sequence end
            int why = 0;
            do {
              ++s;
              if (reach_r == 0) { ++rlo; --rhi; reach_r = e - 1; f_lo = max(f_lo, rlo); f_hi = min(f_hi, rhi); } else --reach_r;
              if (--g_cnt == 0) { g_cnt = e; ++u_w; }
              asm volatile("" : "+s"(f_lo), "+s"(f_hi), "+s"(u_w));
              lo = max(-u_w, f_lo); hi = min(u_w, f_hi);
              if (__builtin_expect(lo > hi, 0)) { why = 1; continue; }
              const int wm1 = hi - lo;            // width - 1
              uint32_t need = 0;
              if constexpr (TILED) {
                // the tile row of this score: 16 bytes on, or on to the next group of four scores
                code_addr += (s & 3) ? 16u : tile_pitch;
              } else if constexpr (BT) {
                // the row of origin bytes (before anything of this score is committed: a failure leaves the loop right here)
                need = ((uint32_t)wm1 + 16u) >> 4;
                code_addr += need_prev << 4;
                if (__builtin_expect(need + WFA_ARENA_ROW_SLACK > chunk_left, 0)) {
                  const bool got = refill_arena(need + WFA_ARENA_ROW_SLACK);
                  code_addr = (GlobalBytes)(uintptr_t)cold_params()->arena + ((size_t)chunk_cur * 16u + (uint32_t)stid);
                  need_prev = 0;
                  if (!got) { why = 2; continue; }
                }
              }
              // (the M ring holds max(x, o + e) + 1 rows: the row of s - max(x, o + e) is the slot the NEXT score writes -- the new M row is
              // the slot the farther of the two read pointers has just left: one wrap test fewer on the pipe this loop saturates)
              a_m = far_is_oe ? a_oe : a_x;
              a_x += rsb;  if (a_x == a_end) a_x = a_first;
              a_oe += rsb; if (a_oe == a_end) a_oe = a_first;
              // (the I / D rings hold e + 1 rows: the row of s - e is the slot the NEXT score writes)
              a_ic = a_ip;
              a_ip += rsb; if (a_ip == ai_end) a_ip = ai_first;
              ncells += (uint32_t)wm1;            // (+ 1 per score when the loop is left)
              if constexpr (BT && !TILED) {
                row_s = chunk_cur; chunk_cur += need; chunk_left -= need; need_prev = need;
                if constexpr (NW == 1) {
                  // row table, buffered by lane: a new group of 64 scores starts at every multiple of 64
                  const int sl = s & 63;
                  if (sl == 0) tab[s - 64 + lane] = make_uint2((uint32_t)tabv_row, (uint32_t)tabv_lo);
                  asm("s_mov_b32 m0, %4\n\tv_writelane_b32 %0, %2, m0\n\tv_writelane_b32 %1, %3, m0"
                      : "+v"(tabv_row), "+v"(tabv_lo) : "s"((int)row_s), "s"(lo), "s"(sl));
                } else {
                  if (tid == 0) tab[s] = make_uint2(row_s, (uint32_t)lo);
                }
              }
              if (__builtin_expect(s >= s_clear, 0)) {
                // the slots written now last held scores s-dm (M) and s-e-1 (I, D), whose limits lay up to dm diagonals
                // further out: NULL the dm cells beyond each end (rows carry dm guard cells per side)
                // (lanes beyond 2 dm repeat the last of those cells: same value, same address, no exec mask)
                auto clear_guards = [&](const int j0) {
                  const int j = min(j0, 2 * dm - 1);
                  const int q = (j < dm) ? lo - 1 - j : hi + 1 - dm + j;
                  const uint32_t qa = (uint32_t)q << 1;
                  *(LdsRow)(qa + a_m) = (OffT)OffNull<OffT>::value;
                  *(LdsRow)(qa + a_ic) = (OffT)OffNull<OffT>::value;
                  if constexpr (HYBRID) *(GlobalRow)((GlobalBytes)(uintptr_t)d_first + (ptrdiff_t)(int32_t)(qa + a_ic + d_delta)) = (OffT)OffNull<OffT>::value;
                  else *(LdsRow)(qa + a_ic + d_delta) = (OffT)OffNull<OffT>::value;
                };
                clear_guards(tid);
                if constexpr (NW == 1) { if (__builtin_expect(2 * dm > 64, 0)) clear_guards(tid + 64); }      // (dm <= 64 in this tier)
              }
              hot_cells(lo, wm1, code_addr, a_oe, a_x, a_m, a_ip, a_ic, d_delta, pw_addr, tw_addr, a_hm, touch);
              a_last = a_m;
              // a cell sits on a sequence end: it may be the last one (wavefront_extend.c:47-67), and from the next
              // score on values may run past the ends -- the careful path takes over
              if constexpr (NW == 1) {
                block_sync<NW>();
                if (touch != 0ull) why = 3;
              } else {
                if (touch != 0ull && lane == 0) atomicOr(touch_flag(s), 1u);
                __syncthreads();
                if (*touch_flag(s) != 0u) why = 3;
              }
            } while (why == 0);
            if constexpr (NW > 1) {
              // the reduction slots of the careful loop (it resets the one of the next score as it goes)
              if (tid < 24) red[tid] = (tid & 7) == 6 ? 0 : (((tid & 7) & 1) ? INT_MIN : INT_MAX);
              __syncthreads();
            }
            const bool nomem = why == 2;
            if (why == 3) touched_ever = true;
            // the limits of score j of this run, again (the state above is the last score's only)
            auto limits_of = [&](const int j, int& jl, int& jh) {
              const int uj = j >= oe ? (j - o_pen) / e : 0;
              jl = max(-uj, wlo); jh = min(uj, whi);
              if (bounded) { const int rj = (budget - j) / e; jl = max(jl, kend - rj); jh = min(jh, kend + rj); }
            };
            if (why != 3) {
              // the score at which the loop gave up was not computed: back to the state of the one before
              --s;
              if (reach_r == e - 1) { --rlo; ++rhi; reach_r = 0; } else ++reach_r;
              if (s > s_in) limits_of(s, lo, hi); else { lo = last_lo; hi = last_hi; }
            }
            const int n_lean = s - s_in;
            ncells += (uint32_t)n_lean;
            if (touched_ever && n_lean > 0)
              done = ((unsigned)(kend - lo) <= (unsigned)(hi - lo)) &&
                     __builtin_amdgcn_readfirstlane((int)*(LdsRow)(a_last + ((uint32_t)kend << 1))) >= tlen;
            // row book: the last dm scores (older entries are never read again)
            for (int j = max(s_in + 1, s - dm + 1); j <= s; ++j) {
              int jl, jh;
              limits_of(j, jl, jh);
              book.set_a(j & bkm, pack_range(jl, jh));
            }
            if (n_lean > 0) book.copy_a_to_id(tid, NT, bkm);
            regular += n_lean;
            last_lo = lo; last_hi = hi;
            p_m = m_first + (a_m - a_first) / 2; p_x = m_first + (a_x - a_first) / 2; p_oe = m_first + (a_oe - a_first) / 2;
            p_ic = m_first + (a_ic - a_first) / 2; p_ip = m_first + (a_ip - a_first) / 2;
            tab_group = s >> 6;
            if (nomem) { status = WFA_ST_NOMEM; break; }
            if (done) break;
          }
        }
