// cells_generic.inc -- cells_of_score: the cells of one score, WFA2 to the letter (careful loop, banded search after a jump, HBM-ring tiers).
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// Reads: the ring rows handed in (rb_*: M[s-x], M[s-o-e], I/D[s-e]), Pw / Tw, plen, tlen, tid, NT.  Writes: the rows of score s (wb_*), one origin
// byte per cell (codes), my_over (a value ran past a sequence end), wave_touch (an M cell sits on a sequence end).
// TWOPIECE: also reads rb2_mo / rb2_ie / rb2_de (M[s-o2-e2], I2 / D2[s-e2]) and writes wb2_i / wb2_d, which the score step sets in front of the call.
      // ---- the cells of one score.  Lanes past the end recompute cell `hi` (same values, same
      // addresses), so no store needs an exec mask.  The vector ALU is the unit this kernel saturates (one
      // integer wave64 instruction holds its SIMD for 4 cycles), so everything uniform is folded into scalar
      // row bases: each LDS address is one v_lshl_add of the diagonal.
      //   rb_mx[k] = M[s-x][k]   rb_mo[k] = M[s-o-e][k-1], rb_mo[k+2] = M[s-o-e][k+1]
      //   rb_ie[k] = I[s-e][k-1] rb_de[k] = D[s-e][k+1]     wb_*[k]: the rows written now
      // LEAN (regular regime, no cell has touched a sequence end yet): no value can run past an end, so the
      // overrun test and the saturation of I are dropped.  wave_touch: lanes whose M cell reached min(plen + k, tlen).
      // (BANDED: wx, wo, we = the windows -- pack_range(lo, hi), ROW_NONE_A for a row that does not exist -- of the rows M[s-x],
      // M[s-o-e] and I/D[s-e]: every read is range-checked against its row's window like the reference's get_offset,
      // lib/kernels/sequence_distance_kernel_aband.cu:28-33, because after a re-centring the rows of neighbouring scores
      // can lie anywhere relative to each other)
      auto cells_of_score = [&](auto lean_tag, const int lo, const int hi, uint8_t* codes, const OffT* rb_mx, const OffT* rb_mo,
                                const OffT* rb_ie, const OffT* rb_de, OffT* wb_m, OffT* wb_i, OffT* wb_d,
                                bool& my_over, unsigned long long& wave_touch, const int wx = 0, const int wo = 0, const int we = 0) {
        constexpr bool LEAN = decltype(lean_tag)::value;
        // (the 16-bit LDS tiers never get here with LEAN set: their lean loops call hot_cells below)
        static_assert(!(LEAN && HOT), "lean cells of the LDS tiers live in hot_cells");
        for (int k0 = lo; k0 <= hi; k0 += NT) {
          const int k = min(k0 + tid, hi);
          // recurrences (wavefront_compute_affine.c:66-84)
          int ins, del, mv0;
          int ins2 = 0, del2 = 0;       // (TWOPIECE: ins and del are I1 and D1, these I2 and D2)
          uint32_t code = 0;
          if constexpr (TWOPIECE) {
            // recurrences of the two pieces (wavefront_compute_affine2p.c:46-106): seven reads.  rb2_mo[k] = M[s-o2-e2][k-1],
            // rb2_mo[k+2] = M[s-o2-e2][k+1], rb2_ie[k] = I2[s-e2][k-1], rb2_de[k] = D2[s-e2][k+1] (set by the score step)
            const int m_x = (int)rb_mx[k];
            const int m_ol = (int)rb_mo[k], m_or = (int)rb_mo[k + 2], i_e = (int)rb_ie[k], d_e = (int)rb_de[k];
            const int m2_ol = (int)rb2_mo[k], m2_or = (int)rb2_mo[k + 2], i2_e = (int)rb2_ie[k], d2_e = (int)rb2_de[k];
            ins = max(m_ol, i_e) + 1; ins2 = max(m2_ol, i2_e) + 1;
            del = max(m_or, d_e); del2 = max(m2_or, d2_e);
            const int mis = m_x + 1;
            mv0 = max(max(del, del2), max(mis, max(ins, ins2)));
            if constexpr (BT) {
              // extension wins over opening on equal offsets (wavefront_compute_affine2p.c:173,191,214,232); M on equal offsets:
              // mismatch, D2, D1, I2, I1 (:251-270, the last assignment stands; wavefront_backtrace.c:49-59)
              code = (i_e >= m_ol ? BT2_I1_EXT : 0u) | (d_e >= m_or ? BT2_D1_EXT : 0u) | (i2_e >= m2_ol ? BT2_I2_EXT : 0u) | (d2_e >= m2_or ? BT2_D2_EXT : 0u);
              code |= (mis == mv0) ? BT2_M_X : (del2 == mv0) ? BT2_M_D2 : (del == mv0) ? BT2_M_D1 : (ins2 == mv0) ? BT2_M_I2 : BT2_M_I1;
            }
          } else {
            int m_x, m_ol, m_or, i_e, d_e;
            if constexpr (BANDED) {
              auto rd = [&](const OffT* base, const int idx, const int kk, const int w) -> int {
                return (kk >= range_lo(w) && kk <= range_hi(w)) ? (int)base[idx] : (int)OffNull<OffT>::value;
              };
              m_x = rd(rb_mx, k, k, wx);
              m_ol = rd(rb_mo, k, k - 1, wo);
              m_or = rd(rb_mo, k + 2, k + 1, wo);
              i_e = rd(rb_ie, k, k - 1, we);
              d_e = rd(rb_de, k, k + 1, we);
            } else {
              m_x = (int)rb_mx[k];
              m_ol = (int)rb_mo[k];
              m_or = (int)rb_mo[k + 2];
              i_e = (int)rb_ie[k];
              d_e = (int)rb_de[k];
            }
            ins = max(m_ol, i_e) + 1;
            del = max(m_or, d_e);
            const int mis = m_x + 1;
            mv0 = max(del, max(mis, ins));
            if constexpr (BT) {
              // tie-breaks: gap extension wins over gap open on equal offsets
              // (wavefront_compute_affine.c:135-143,153-161); for M: mismatch, then deletion, then
              // insertion (wavefront_backtrace.c:48-59)
              // (the M origin of a cell that is not valid is never read: the backtrace only visits valid cells)
              code = (i_e >= m_ol ? BT_I_EXT : 0u) | (d_e >= m_or ? BT_D_EXT : 0u);
              code |= (mis == mv0) ? BT_M_X : ((del == mv0) ? BT_M_D : BT_M_I);
            }
          }
          // !(h > tlen || v > plen), unsigned so that negatives fail too
          const bool ok = ((unsigned)mv0 <= (unsigned)tlen) & ((unsigned)(mv0 - k) <= (unsigned)plen);
          // An I (D) value can only be out of range by running past the text (pattern) end; such
          // values are rare (last scores only) and send the row through the exact trimming pass
          // below.  Everywhere else "invalid" means negative, which already reads as NULL, so the
          // computed limits can stand in for the trimmed ones.
          if constexpr (!LEAN) my_over |= (ins > tlen) || (del - k > plen);
          if constexpr (TWOPIECE) my_over |= (ins2 > tlen) || (del2 - k > plen);
          // extend = longest common prefix from (v,h) (wavefront_extend.c:174-199), PER symbols per step.  No exec
          // mask for the cells that are not valid: a wave instruction costs the same with any lane active, mask
          // bookkeeping costs scalar instructions, and LDS reads at their meaningless addresses are harmless (an
          // address beyond the workgroup's allocation reads as 0); their result is dropped below.  The first step is
          // straight-line code (most cells stop inside their first word); only when some lane matched a whole word
          // with more to go does the wave enter the loop, in which lanes that are done carry left == 0 and idle along.
          int h = mv0;
          constexpr int SH = RAW ? 2 : 4, PER = 1 << SH, BITS = RAW ? 3 : 1;
          // the run cannot pass either sequence end: h <= tlen and v = h - k <= plen
          const int hmax = min(plen + k, tlen);
          {
            const int v = mv0 - k;
            const int rem = hmax - h;
            // word pointers and bit offsets are fixed for the whole run: a lane that goes on has
            // consumed exactly PER symbols = one word
            const char* pp = reinterpret_cast<const char*>(Pw + (v >> SH));
            const char* tp = reinterpret_cast<const char*>(Tw + (h >> SH));
            const uint32_t sa = (uint32_t)v << BITS, sb = (uint32_t)h << BITS;
            uint32_t fb, d0w;
            {
              const uint32_t* pw = reinterpret_cast<const uint32_t*>(pp);
              const uint32_t* tw = reinterpret_cast<const uint32_t*>(tp);
              d0w = __builtin_amdgcn_alignbit(pw[1], pw[0], sa) ^ __builtin_amdgcn_alignbit(tw[1], tw[0], sb);
              // v_ffbl_b32 returns 0xFFFFFFFF for 0, so "all equal" is a huge positive count
              asm("v_ffbl_b32 %0, %1" : "=v"(fb) : "v"(d0w));
            }
            {
              // (one v_min3_i32: the compiler splits the two mins into an unsigned and a signed one)
              int adv;
              asm("v_min3_i32 %0, %1, %2, %3" : "=v"(adv) : "v"((int)(fb >> BITS)), "v"(rem), "n"(PER));
              h += adv;
            }
            // the whole word matched: the run may go on (if anything remains)
            const bool more = ok & (d0w == 0u);
            if (__builtin_amdgcn_ballot_w64(more) != 0ull) {
              int left = more ? max(rem - PER, 0) : 0;
              while (__builtin_amdgcn_ballot_w64(left > 0) != 0ull) {
                pp += 4; tp += 4;
                const uint32_t* pw = reinterpret_cast<const uint32_t*>(pp);
                const uint32_t* tw = reinterpret_cast<const uint32_t*>(tp);
                const uint32_t d = __builtin_amdgcn_alignbit(pw[1], pw[0], sa) ^ __builtin_amdgcn_alignbit(tw[1], tw[0], sb);
                asm("v_ffbl_b32 %0, %1" : "=v"(fb) : "v"(d));
                const int nn = min(min((int)(fb >> BITS), PER), left);
                h += nn;
                left = (nn == PER) ? left - PER : 0;
              }
            }
          }
          const int mv = ok ? h : OffNull<OffT>::value;
          wave_touch |= __builtin_amdgcn_ballot_w64(mv == hmax);      // (NULL never equals it)
          // M and D offsets never exceed the text length, so they fit 16 bits as they are; only an I
          // chain running past the text end keeps growing and is saturated by off_store
          wb_m[k] = (OffT)mv;
          if constexpr (LEAN) wb_i[k] = (OffT)ins; else wb_i[k] = off_store<OffT>(ins);
          wb_d[k] = (OffT)del;
          if constexpr (TWOPIECE) { wb2_i[k] = off_store<OffT>(ins2); wb2_d[k] = (OffT)del2; }
          // (TILED: `codes` is the tile row of the score, the byte of diagonal k sits tile_off(k) into it)
          if constexpr (BT) { if constexpr (TILED) codes[tile_off(k)] = (uint8_t)code; else codes[(uint32_t)(k - lo)] = (uint8_t)code; }
        }
      };
