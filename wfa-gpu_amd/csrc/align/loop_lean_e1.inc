// loop_lean_e1.inc -- lean score loop, gap extension 1, closed-form limits (exact 16-bit LDS tiers: 0, 1, 2 and the hybrid ring).
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// Runs from the current score until a cell touches a sequence end, the reach interval empties or the arena is exhausted; then hands the
// general state (s, limits, row pointers, row book, reach) back to the careful loop.
        // ---- lean path: gap extension 1 and no cell has touched a sequence end yet.  Then no value can run past an end,
        // nothing is ever trimmed, and with e == 1 the limits of wavefront_compute.c:41-71 collapse to [lo - 1, hi + 1] of
        // the last score (the I and D rows of s-1 span its M limits), clipped by the window and the budget's reach.  It starts
        // at score 1: wavefronts and components that WFA2 does not create yet (no predecessor row exists) are computed here
        // as rows of NULL cells from the NULL rows of the ring -- a superset of WFA2's cells whose extra members are not
        // valid and only feed cells that are not valid either (SURVEY.md A.1), at most one 64-lane chunk per early score.
        // An inner loop with its own small state: the instruction-issue pipes are what this kernel saturates, and
        // the scalar registers are what the compiler runs out of (every spilled one comes back through the vector unit).
        // ---- the same lean path written out for the one-wavefront 16-bit LDS tier (BASELINE's short-read configs live
        // here).  Vector and scalar instructions of a wavefront share its issue slots (one instruction per wave every
        // four cycles), so the per-score bookkeeping -- as many instructions as a 64-diagonal chunk of cells -- is cut
        // to the bone: limits in closed form, row addresses as one lane base (lo + lane - 1) plus a scalar slot base each
        // (every neighbour is a non-negative immediate away), row book written when the loop is left (its entries are
        // a function of the score), row-table entries by v_writelane, guard cells re-NULLed only once the budget's
        // reach makes the wavefront shrink (a growing wavefront overwrites everything its slot held before).
        if constexpr (HOT && !BANDED && !ENDSFREE) {
          if (e == 1 && !touched_ever) {
            const int s_in = s, lo_in = last_lo, hi_in = last_hi;
            // lo(s) = max(lo_in - (s - s_in), wlo, s + c_lo), hi(s) = min(hi_in + (s - s_in), whi, c_hi - s)
            const int c_lo = bounded ? kend - budget : INT_MIN / 2, c_hi = bounded ? kend + budget : INT_MAX / 2;
            // first score at which a limit can move inwards (the reach bound has caught up with the window or the growing
            // front); from dm scores before... after it on, the slots written hold cells beyond the new limits
            int s_clear = INT_MAX;
            if (bounded) {
              const int t_lo = min(wlo - c_lo, (lo_in + s_in - c_lo) >> 1), t_hi = min(c_hi - whi, (c_hi - hi_in + s_in) >> 1);
              s_clear = min(t_lo, t_hi) - 1;
            }
            s_clear = __builtin_amdgcn_readfirstlane(s_clear);     // (a scalar, whatever unit the compiler formed it on)
            const uint32_t rsb = (uint32_t)rs * 2u;
            const uint32_t a_first = lds_addr(m_first), a_end = lds_addr(m_end);
            uint32_t a_m = lds_addr(p_m), a_x = lds_addr(p_x), a_oe = lds_addr(p_oe);
            uint32_t a_ic = lds_addr(p_ic), a_ip = lds_addr(p_ip);
            const uint32_t a_iswap = a_ic ^ a_ip;
            // the D row of an I row: further up in LDS, or (hybrid ring) the same offset into the global D ring, which is laid out like
            // the I ring
            uint32_t d_delta = HYBRID ? 0u - lds_addr(i_first) : (uint32_t)(de * rs) * 2u;
            // (formed here, next to the loop that uses them in every chunk: defined further out they are the first
            // scalars the register allocator gives up, and every chunk then fetches them back from a vector register)
            uint32_t pw_addr = lds_addr(Pw), tw_addr = lds_addr(Tw), a_hm = lds_addr(hm_row0);
            asm volatile("" : "+s"(pw_addr), "+s"(tw_addr), "+s"(a_hm), "+s"(d_delta));
            int lo = lo_in, hi = hi_in;
            int t_lo = s_in + c_lo, t_hi = c_hi - s_in, f_lo = max(wlo, t_lo), f_hi = min(whi, t_hi);
            unsigned long long touch = 0;
            uint32_t a_last = a_m;
            // address of this lane's origin byte in the row of the current score (64-bit, bumped by the row size)
            GlobalBytes code_addr = nullptr;
            uint32_t need_prev = 0;
            if constexpr (TILED) code_addr = tile_row(s);      // (the tile row of the current score: a scalar)
            else if constexpr (BT) code_addr = (GlobalBytes)(uintptr_t)p.arena + ((size_t)chunk_cur * 16u + (uint32_t)stid);
            const uint32_t tile_pitch = tile_cols * 64u - 48u;      // (TILED: from in-tile row 3 of a group to row 0 of the next)
            if constexpr (NW > 1) {
              // "a cell touched a sequence end": one LDS word, set by the waves that see it, read after the score's barrier
              if (tid == 0) { *touch_flag(0) = 0u; *touch_flag(1) = 0u; }
              __syncthreads();
            }
            // why the loop ends: 1 = the reach interval is empty, 2 = arena exhausted, 3 = a cell touched a sequence end
            // (one exit at the bottom: several would be funnelled through a guard variable anyway)
            int why = 0;
            const bool far_is_oe = oe >= x;
            do {
              // (everything is updated in place -- no second set of registers to copy back at the bottom; when the loop
              // ends without having computed this score, the state of the last computed one is re-derived below)
              // (f_lo = max(wlo, s + c_lo) and f_hi = min(whi, c_hi - s), carried along: four loop constants fewer for the
              // scalar registers, which this loop runs out of -- a spilled one comes back through the vector unit)
              ++s; ++t_lo; --t_hi;
              f_lo = max(f_lo, t_lo); f_hi = min(f_hi, t_hi);
              asm volatile("" : "+s"(f_lo), "+s"(f_hi));   // (keeps the chains off v_max3/v_min3)
              lo = max(lo - 1, f_lo); hi = min(hi + 1, f_hi);
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
              // (the M ring holds max(x, o + e) + 1 rows: the new M row is the slot the farther of the two read pointers has just left)
              a_m = far_is_oe ? a_oe : a_x;
              a_x += rsb;  if (a_x == a_end) a_x = a_first;
              a_oe += rsb; if (a_oe == a_end) a_oe = a_first;
              a_ic ^= a_iswap; a_ip ^= a_iswap;
              ncells += (uint32_t)wm1;            // (+ 1 per score when the loop is left)
              if constexpr (BT && !TILED) {
                row_s = chunk_cur; chunk_cur += need; chunk_left -= need; need_prev = need;
                if constexpr (NW == 1) {
                  // row table, buffered by lane: a new group of 64 scores starts at every multiple of 64
                  const int sl = s & 63;
                  if (sl == 0) tab[s - 64 + lane] = make_uint2((uint32_t)tabv_row, (uint32_t)tabv_lo);
                  asm("s_mov_b32 m0, %4\n\tv_writelane_b32 %0, %2, m0\n\tv_writelane_b32 %1, %3, m0"
                      : "+v"(tabv_row), "+v"(tabv_lo) : "s"((int)row_s), "s"(lo), "s"(sl));      // (m0: scratch, the compiler sets it before each use of its own)
                } else {
                  if (tid == 0) tab[s] = make_uint2(row_s, (uint32_t)lo);
                }
              }
              if (__builtin_expect(s >= s_clear, 0)) {
                // the slots written now last held scores s-dm (M) and s-2 (I, D), whose limits lay up to dm diagonals
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
                if constexpr (TIMED) {
                  const bool rec = blockIdx.x == 0 && lane == 0;
                  unsigned long long t_arrive = 0;
                  if (rec) t_arrive = __builtin_amdgcn_s_memtime();
                  __syncthreads();
                  if (rec) {
                    const unsigned long long t_leave = __builtin_amdgcn_s_memtime();
                    ColdParams cp = cold_params();
                    if (dbg_i < cp->dbg_cap) {
                      unsigned long long* rp = cp->dbg_times + ((size_t)dbg_i * NW + (size_t)(tid >> 6)) * 3;
                      rp[0] = t_arrive; rp[1] = t_leave; rp[2] = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)wm1;
                    }
                    ++dbg_i;
                  }
                } else {
                  __syncthreads();
                }
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
            if (why != 3) {
              // the score at which the loop gave up was not computed: back to the limits of the one before
              --s;
              lo = max(max(lo_in - (s - s_in), wlo), s + c_lo); hi = min(min(hi_in + (s - s_in), whi), c_hi - s);
            }
            // back to the general state
            const int n_lean = s - s_in;
            ncells += (uint32_t)n_lean;
            if (touched_ever && n_lean > 0)
              done = ((unsigned)(kend - lo) <= (unsigned)(hi - lo)) &&
                     __builtin_amdgcn_readfirstlane((int)*(LdsRow)(a_last + ((uint32_t)kend << 1))) >= tlen;
            // row book: the last dm scores (older entries are never read again)
            for (int j = max(s_in + 1, s - dm + 1); j <= s; ++j) {
              const int jl = max(max(lo_in - (j - s_in), wlo), j + c_lo), jh = min(min(hi_in + (j - s_in), whi), c_hi - j);
              book.set_a(j & bkm, pack_range(jl, jh));
            }
            if (n_lean > 0) book.copy_a_to_id(tid, NT, bkm);
            regular += n_lean;
            last_lo = lo; last_hi = hi;
            p_m = m_first + (a_m - a_first) / 2; p_x = m_first + (a_x - a_first) / 2; p_oe = m_first + (a_oe - a_first) / 2;
            p_ic = m_first + (a_ic - a_first) / 2; p_ip = m_first + (a_ip - a_first) / 2;
            if (bounded) { rlo += n_lean; rhi -= n_lean; }
            tab_group = s >> 6;
            if (nomem) { status = WFA_ST_NOMEM; break; }
            if (done) break;
          }
        }
