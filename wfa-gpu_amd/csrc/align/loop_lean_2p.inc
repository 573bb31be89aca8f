// loop_lean_2p.inc -- lean score loop of the exact, end-to-end two-piece instantiations (16-bit LDS tiers 0, 1 and 2): limits carried along, no row book.
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// Same contract as loop_lean_any.inc: runs from the current score until an M cell touches a sequence end, the reach interval empties or the
// arena is exhausted; then hands the general state (s, limits, the eight row pointers, BOTH row books, reach, regular) back to
// loop_careful_2p.inc, which finishes the alignment.
        // ---- lean path under two pieces.  The careful step (loop_careful_2p.inc) takes its limits from seven entries of two row books,
        // applies the existence rule per component, tests four gap values for overrun, trims and reads the termination cell at every
        // score; before any M cell has touched a sequence end none of that can find anything (align_kernel.hip, touched_ever).
        //
        // Limits.  All five components of score s are computed over ONE interval [-U(s), U(s)], U(s) = max(floor((s - o1) / e1),
        // floor((s - o2) / e2), 0): the longest gap s pays for under either piece (wfa_reach2p) -- clipped by the window and by the
        // budget's reach like every row.  It is a superset of WFA2's limits of every component: a cell of M, I1, D1, I2 or D2 on diagonal
        // k ends a path from (0, 0) that holds gaps of at least |k| net bases, in one gap or in several, and g(n) = min(o1 + n e1, o2 + n e2)
        // is increasing and subadditive (wfa_device.h), so the path costs at least g(|k|): g(|k|) <= s, i.e. |k| <= U(s).  (A cell of I or D
        // sits inside an open gap whose opening and bases so far are paid for: the same bound.)  The extra cells are not valid cells, by
        // loop_lean_any.inc's argument made for five components and three ring depths: WFA2's limits of a component are the union of
        // what its predecessor rows can reach (M: the rows s-x, s-o1-e1, s-o2-e2 of M -- ring depth max(x, o1+e1, o2+e2) + 1 --, s-e1 of
        // I1 / D1 -- depth e1 + 1 --, s-e2 of I2 / D2 -- depth e2 + 1; I1, D1: M of s-o1-e1 and their own row of s-e1; I2, D2: M of
        // s-o2-e2 and their own row of s-e2), so every predecessor of a cell outside WFA2's limits lies outside ITS row's WFA2 limits,
        // hence is NULL by induction, or lies beyond what its row was computed with, hence is NULL by the ring invariant; a NULL plus one
        // per score stays negative.  Valid cells get WFA2's values and origin bytes, the backtrace only visits valid cells, a NULL never
        // equals a run limit.  A score WFA2 has no wavefront for (every odd score below 25 under (4,6,2,24,1)) is a row of NULL cells.
        // U(s) is carried by one counter per piece; the reach interval shrinks every min(e1, e2) scores (reach_r, e_reach).
        if constexpr (HOT && !ENDSFREE && !ADAPTIVE) {
          if (!touched_ever) {
            const int s_in = s;
            const int o1_pen = oe - e, o2_pen = oe2 - e2;
            // per piece: the gap length score s_in pays for and the scores left until it grows next (at s = oe, oe + e, ...)
            int u1 = s_in >= oe ? (s_in - o1_pen) / e : 0, g1_cnt = s_in >= oe ? e - (s_in - o1_pen) % e : oe - s_in;
            int u2 = s_in >= oe2 ? (s_in - o2_pen) / e2 : 0, g2_cnt = s_in >= oe2 ? e2 - (s_in - o2_pen) % e2 : oe2 - s_in;
            // First score at which a limit may move inwards, on the safe side (early).  Only the reach interval moves inwards:
            // lo(s) = max(-U(s), wlo, kend - R(s)) with R(s) = floor((budget - s) / er), er = min(e1, e2).  Its term passes the window at
            // s > budget - er (kend - wlo), and the front where R(s) < U(s) + kend: with R(s) > (budget - s) / er - 1 and
            // U(s) <= (s - min(o1, o2)) / er that needs 2 s > budget + min(o1, o2) - er (kend + 1); the upper side alike with -kend.
            int s_clear = INT_MAX;
            if (bounded) {
              const int er = e_reach, o_min = min(o1_pen, o2_pen);
              const int lo_a = budget - er * (kend - wlo) + 1, lo_b = (budget + o_min - er * (kend + 1)) / 2 + 1;
              const int hi_a = budget - er * (whi - kend) + 1, hi_b = (budget + o_min + er * (kend - 1)) / 2 + 1;
              s_clear = min(min(lo_a, lo_b), min(hi_a, hi_b)) - 2 * er - 2;
            }
            s_clear = __builtin_amdgcn_readfirstlane(s_clear);
            const uint32_t rsb = (uint32_t)rs * 2u;
            const uint32_t a_first = lds_addr(m_first), a_end = lds_addr(m_end), ai_first = lds_addr(i_first), ai_end = lds_addr(i_end);
            const uint32_t ai2_first = lds_addr(i2_first), ai2_end = lds_addr(i2_end);
            uint32_t a_m = lds_addr(p_m), a_x = lds_addr(p_x), a_oe = lds_addr(p_oe), a_oe2 = lds_addr(p_oe2);
            uint32_t a_ic = lds_addr(p_ic), a_ip = lds_addr(p_ip), a_ic2 = lds_addr(p_ic2), a_ip2 = lds_addr(p_ip2);
            // the D1 row of an I1 row and the D2 row of an I2 row: further up in LDS; the run-limit row (one-wave tier) behind all five rings
            uint32_t d_delta = (uint32_t)(de * rs) * 2u, d2_delta = (uint32_t)(de2 * rs) * 2u;
            uint32_t pw_addr = lds_addr(Pw), tw_addr = lds_addr(Tw), a_hm = lds_addr(Mr + (dm + 2 * de + 2 * de2) * rs + kidx0);
            asm volatile("" : "+s"(pw_addr), "+s"(tw_addr), "+s"(a_hm), "+s"(d_delta), "+s"(d2_delta));
            int lo = last_lo, hi = last_hi;
            int f_lo = max(wlo, rlo), f_hi = min(whi, rhi);      // (window and reach together: both only ever move inwards)
            unsigned long long touch = 0;
            uint32_t a_last = a_m;
            GlobalBytes code_addr = nullptr;
            uint32_t need_prev = 0;
            if constexpr (BT) code_addr = (GlobalBytes)(uintptr_t)p.arena + ((size_t)chunk_cur * 16u + (uint32_t)stid);
            if constexpr (NW > 1) {
              if (tid == 0) { *touch_flag(0) = 0u; *touch_flag(1) = 0u; }
              __syncthreads();
            }
            // which M read pointer is the farthest back: 0 = s-x, 1 = s-o1-e1, 2 = s-o2-e2
            const int far = (oe2 >= x && oe2 >= oe) ? 2 : (oe >= x ? 1 : 0);
            // why the loop ends: 1 = the reach interval is empty, 2 = arena exhausted, 3 = a cell touched a sequence end
            int why = 0;
            do {
              ++s;
              if (reach_r == 0) { ++rlo; --rhi; reach_r = e_reach - 1; f_lo = max(f_lo, rlo); f_hi = min(f_hi, rhi); } else --reach_r;
              if (--g1_cnt == 0) { g1_cnt = e; ++u1; }
              if (--g2_cnt == 0) { g2_cnt = e2; ++u2; }
              int u_w = max(u1, u2);
              asm volatile("" : "+s"(f_lo), "+s"(f_hi), "+s"(u_w));
              lo = max(-u_w, f_lo); hi = min(u_w, f_hi);
              if (__builtin_expect(lo > hi, 0)) { why = 1; continue; }
              const int wm1 = hi - lo;            // width - 1
              uint32_t need = 0;
              if constexpr (BT) {
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
              // (the M ring holds max(x, o1+e1, o2+e2) + 1 rows: the new M row is the slot the farthest read pointer has just left)
              a_m = far == 2 ? a_oe2 : (far == 1 ? a_oe : a_x);
              a_x += rsb;   if (a_x == a_end) a_x = a_first;
              a_oe += rsb;  if (a_oe == a_end) a_oe = a_first;
              a_oe2 += rsb; if (a_oe2 == a_end) a_oe2 = a_first;
              // (the I1 / D1 rings hold e1 + 1 rows, the I2 / D2 rings e2 + 1: the row of s - e is the slot the NEXT score writes)
              a_ic = a_ip;   a_ip += rsb;  if (a_ip == ai_end) a_ip = ai_first;
              a_ic2 = a_ip2; a_ip2 += rsb; if (a_ip2 == ai2_end) a_ip2 = ai2_first;
              ncells += (uint32_t)wm1;            // (+ 1 per score when the loop is left)
              if constexpr (BT) {
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
                // the five slots written now last held scores s-dm (M), s-e1-1 (I1, D1) and s-e2-1 (I2, D2), whose limits lay up to dm
                // diagonals further out: NULL the dm cells beyond each end (rows carry dm guard cells per side)
                for (int j = tid; j < 2 * dm; j += NT) {
                  const int q = (j < dm) ? lo - 1 - j : hi + 1 - dm + j;
                  const uint32_t qa = (uint32_t)q << 1;
                  *(LdsRow)(qa + a_m) = (OffT)OffNull<OffT>::value;
                  *(LdsRow)(qa + a_ic) = (OffT)OffNull<OffT>::value;
                  *(LdsRow)(qa + a_ic + d_delta) = (OffT)OffNull<OffT>::value;
                  *(LdsRow)(qa + a_ic2) = (OffT)OffNull<OffT>::value;
                  *(LdsRow)(qa + a_ic2 + d2_delta) = (OffT)OffNull<OffT>::value;
                }
              }
              hot_cells_2p(lo, wm1, code_addr, a_oe, a_oe2, a_x, a_m, a_ip, a_ic, d_delta, a_ip2, a_ic2, d2_delta, pw_addr, tw_addr, a_hm, touch);
              a_last = a_m;
              // a cell sits on a sequence end: it may be the last one (wavefront_extend.c:47-67), and from the next
              // score on values may run past the ends -- the careful path takes over
              if constexpr (NW == 1) {
                block_sync<NW>();
                if (touch != 0ull) why = 3;
              } else {
                // (one barrier per score; the touch word per score parity: align_kernel.hip, touch_flag)
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
            // the limits of score j of this run, again, in closed form (the state above is the last score's only)
            auto limits_of = [&](const int j, int& jl, int& jh) {
              const int uj = max(j >= oe ? (j - o1_pen) / e : 0, j >= oe2 ? (j - o2_pen) / e2 : 0);
              jl = max(-uj, wlo); jh = min(uj, whi);
              if (bounded) { const int rj = (budget - j) / e_reach; jl = max(jl, kend - rj); jh = min(jh, kend + rj); }
            };
            if (why != 3) {
              // the score at which the loop gave up was not computed: back to the state of the one before
              --s;
              if (reach_r == e_reach - 1) { --rlo; ++rhi; reach_r = 0; } else ++reach_r;
              if (s > s_in) limits_of(s, lo, hi); else { lo = last_lo; hi = last_hi; }
            }
            const int n_lean = s - s_in;
            ncells += (uint32_t)n_lean;
            if (touched_ever && n_lean > 0)
              done = ((unsigned)(kend - lo) <= (unsigned)(hi - lo)) &&
                     __builtin_amdgcn_readfirstlane((int)*(LdsRow)(a_last + ((uint32_t)kend << 1))) >= tlen;
            // both row books: the last dm scores (older entries are never read again); every lean score has all five components over
            // the limits of its M row, so the I1 / D1 entries and the I2 / D2 entries are the A entries
            for (int j = max(s_in + 1, s - dm + 1); j <= s; ++j) {
              int jl, jh;
              limits_of(j, jl, jh);
              book.set_a(j & bkm, pack_range(jl, jh));
            }
            if (n_lean > 0) {
              book.copy_a_to_id(tid, NT, bkm);
              if constexpr (BOOK_NW == 1) { book2.i = book.a; book2.d = book.a; }
              else { for (int j = tid; j <= bkm; j += NT) { book2.I[j] = book.A[j]; book2.D[j] = book.A[j]; } __syncthreads(); }
            }
            regular += n_lean;
            last_lo = lo; last_hi = hi;
            p_m = m_first + (a_m - a_first) / 2; p_x = m_first + (a_x - a_first) / 2; p_oe = m_first + (a_oe - a_first) / 2; p_oe2 = m_first + (a_oe2 - a_first) / 2;
            p_ic = m_first + (a_ic - a_first) / 2; p_ip = m_first + (a_ip - a_first) / 2;
            p_ic2 = m_first + (a_ic2 - a_first) / 2; p_ip2 = m_first + (a_ip2 - a_first) / 2;
            tab_group = s >> 6;
            if (nomem) { status = WFA_ST_NOMEM; break; }
            if (done) break;
          }
        }
