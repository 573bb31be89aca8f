// cells_hot.inc -- hot_cells: the lean cells of one score for the 16-bit LDS tiers (the hot loop of the whole library: 28 vector instructions per 64 cells).
// Textually included in the body of wfa_align_kernel (../align_kernel.hip), where every name used here is declared.
// Reads: rows as LDS byte addresses of their diagonal 0, pw_addr / tw_addr (staged sequences), a_hm (run-limit row), kq/stid.  Writes: M / I / D
// of score s, one origin byte per cell through `codes`, touch.  Only while no cell has touched a sequence end (no overrun, no trimming).
      // ---- the lean cells of one score for the one-wavefront 16-bit LDS tier: rows given as LDS byte addresses of their
      // diagonal 0 (a_oe: M[s-o-e], a_x: M[s-x], a_ip: I of s-e, a_m / a_ic: the rows written; the D rows: d_delta from the I rows), `codes`:
      // this lane's origin byte in the row of origin bytes (global), wm1 = hi - lo.  Same cells, values and origin bytes
      // as cells_of_score's lean form.
      typedef __attribute__((address_space(3))) OffT* LdsRow;
      typedef __attribute__((address_space(3))) const uint32_t* LdsWords;
      typedef __attribute__((address_space(1))) uint8_t* GlobalBytes;
      typedef __attribute__((address_space(1))) OffT* GlobalRow;
      OffT* const hm_row0 = Mr + (dm + 2 * de) * rs + kidx0;      // (HOT) diagonal 0 of the run-limit row
      auto hot_cells = [&](const int lo, const int wm1, GlobalBytes& codes, const uint32_t a_oe, const uint32_t a_x, const uint32_t a_m,
                           const uint32_t a_ip, const uint32_t a_ic, const uint32_t d_delta, const uint32_t pw_addr, const uint32_t tw_addr,
                           const uint32_t a_hm, unsigned long long& touch) {
        constexpr int SH = RAW ? 2 : 4, PER = 1 << SH, BITS = RAW ? 3 : 1;
        // Every role tag carries TB >= PER besides its origin bits (the backtrace masks them off), so that any tagged value
        // that is valid (offset >= 0) is >= PER and v_med3(value, 0, PER) is PER for a valid cell and 0 for a NULL one.
        constexpr uint32_t TB = 16;
        // two chunks of a row issued together (front, front, back, back: below).  Only where a chunk waits for GLOBAL memory -- the
        // hybrid ring's D row: BASELINE configs[4] main launch 70.51 -> 69.70 ms; the one-wave tier does not move (24.96 / 24.94 ms),
        // the four-wave tier loses (12.85 -> 13.17 ms): alternating builds on one box, bit-exact
        // (round 5: the banded kernels too -- rows of 1024 diagonals on four waves, four chunks per wave and score: ONT-shaped 30 kbp
        // pairs 15.2 -> 14.8 ms; rows of 512 on two or four waves: within the noise)
        constexpr bool PAIRED = HYBRID || BANDED;
        // The last chunk of a row stores under its lane mask instead of selecting NULL into the lanes beyond hi (three v_cndmask per
        // score).  That needs the ring invariant on the upper side as the lower side has always needed it: both lean loops
        // (loop_lean_e1.inc, loop_lean_any.inc; every exact LDS tier and the hybrid ring) keep it with clear_guards.  The banded loops
        // (loop_banded.inc) store rows relative to a window that moves between scores and have no clear_guards; the argument has not
        // been made for them: they stay with the selects.
        constexpr bool MASKED_LAST = !BANDED;
        static_assert(TB >= (uint32_t)PER && (TB & (BT_M_MASK | BT_D_EXT | BT_I_EXT)) == 0, "tag base");
        // a group of up to four chunks from kq (this lane's diagonal; the lane base of every row involved is cell kq - 1:
        // all neighbours are immediates from there) and codes; returns whether the row goes on beyond the group
        auto group = [&](const int kq, const GlobalBytes codes, const int left) -> bool {
          bool more_groups;
          const uint32_t vb = (uint32_t)(kq - 1) << 1;
          const int kq16 = kq << 16;
          // (one v_add each, once per score: the empty asm keeps the compiler from re-forming them in every chunk)
          uint32_t q_mo = vb + a_oe, q_mx = vb + a_x, q_wm = vb + a_m, q_ri = vb + a_ip, q_wi = vb + a_ic;
          // (the D row of an I row sits d_delta bytes from it -- further up in LDS, or the same offset into the global D ring: the two D
          // addresses come from the I addresses, and no loop keeps D row addresses of its own)
          uint32_t q_rd = q_ri + d_delta, q_wd = q_wi + d_delta, q_hm = vb + a_hm;
          asm volatile("" : "+v"(q_mo), "+v"(q_mx), "+v"(q_wm), "+v"(q_ri), "+v"(q_wi), "+v"(q_rd), "+v"(q_wd), "+v"(q_hm));
          const LdsRow r_mo = (LdsRow)q_mo, r_mx = (LdsRow)q_mx, w_m = (LdsRow)q_wm;
          const LdsRow r_i = (LdsRow)q_ri, w_i = (LdsRow)q_wi, r_hm = (LdsRow)q_hm;
          // the D rows: LDS like the others, or (hybrid ring) global memory, where a_dp / a_dc are byte offsets into the ring
          auto d_row = [&](const uint32_t q) {
            if constexpr (HYBRID) return (GlobalRow)((GlobalBytes)(uintptr_t)d_first + (ptrdiff_t)(int32_t)q);      // (diagonals below 0: negative offsets)
            else return (LdsRow)q;
          };
          const auto r_d = d_row(q_rd), w_d = d_row(q_wd);
          // (TILED: `codes` is the tile row of the score -- one address for the whole wavefront, a scalar --, this lane's byte sits
          // d + 3 (d & ~15) bytes into it, d = k - wlo: tile column d >> 4, byte d & 15 of the score's 16; 64 diagonals on = 256 bytes on)
          uint32_t t_off = 0;
          if constexpr (TILED) { t_off = tile_off(kq); asm volatile("" : "+v"(t_off)); }
          // A chunk in two halves.  front: the ring loads, the recurrences, the origin byte and the FIRST 16-base step of the run
          // (straight-line code); back: the (rare) continuation of the run and the stores.  Two chunks of a row are issued as
          // front, front, back, back: the chunks of a score are independent of each other (they read rows of earlier scores only),
          // and with both fronts in one basic block the scheduler puts the second chunk's loads under the first one's arithmetic.
          struct ChunkState { int h, rem, hmax, ins_c, del_t; uint32_t pa, ta, sa, sb, code; bool more; };
          auto front = [&](auto uc) -> ChunkState {
            constexpr int O = decltype(uc)::value * NT;
            ChunkState c;
            const int k = kq + O;
            const uint32_t u_ol = (uint16_t)r_mo[O], u_or = (uint16_t)r_mo[O + 2], u_ie = (uint16_t)r_i[O],
                           u_de = (uint16_t)r_d[O + 2], u_x = (uint16_t)r_mx[O + 1];
            // min(plen + k, tlen): how far a run on this diagonal can go
            c.hmax = HM_ROW ? (int)(uint16_t)r_hm[O + 1] : min(plen + k, tlen);
            c.ins_c = max((int)((u_ol << 16) + (0x10000u | TB | BT_M_I)), (int)((u_ie << 16) + (0x10000u | TB | BT_M_I | BT_I_EXT)));
            c.del_t = max((int)((u_or << 16) | (TB | BT_M_D)), (int)((u_de << 16) | (TB | BT_M_D | BT_D_EXT)));
            const int mis_c = (int)((u_x << 16) + (0x10000u | TB | BT_M_X));
            const int mv_t = max(c.del_t, max(mis_c, c.ins_c));
            c.code = 0;
            if constexpr (BT) {
              uint32_t c1;
              asm("v_bfi_b32 %0, 2, %1, %2" : "=v"(c1) : "v"(c.del_t), "v"(mv_t));      // bit 1 from the deletion winner
              asm("v_bfi_b32 %0, 1, %1, %2" : "=v"(c.code) : "v"(c.ins_c), "v"(c1));    // bit 0 from the insertion winner
            }
            const int mv0 = mv_t >> 16;
            // Nothing has touched a sequence end: "not valid" = NULL = negative.  A NULL cell gets a run length of 0 and is
            // stored as it is -- NULL plus at most one per score, which stays negative for every score 16 bits can hold.
            int cap;
            asm("v_med3_i32 %0, %1, 0, %2" : "=v"(cap) : "v"(mv_t), "n"(PER));
            c.h = mv0;
            c.rem = c.hmax - c.h;
            if constexpr (!RAW) {
              // (gfx950 issues v_add/v_sub/v_and/v_or/v_xor and the RIGHT shifts at one wave instruction per ~2.5 cycles,
              // left shifts, min/max, compares, every three-operand and every SDWA form at one per ~4.2 --
              // profiles/r04/valu_classes.txt: v and h are taken from the tagged value with subtractions and right shifts.
              // The tag occupies bits 4:0 and bit 15 is clear, so (x >> 15) is twice the high half.)
              const int vt = mv_t - kq16 - (O << 16);             // (h - k) << 16 | tag
              asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(c.pa) : "v"(vt >> (16 + SH)), "s"(pw_addr));
              asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(c.ta) : "v"(mv_t >> (16 + SH)), "s"(tw_addr));
              c.sa = (uint32_t)vt >> 15; c.sb = (uint32_t)mv_t >> 15;
            } else {
              const int v = mv0 - k;
              asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(c.pa) : "v"(v >> SH), "s"(pw_addr));
              asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(c.ta) : "v"(c.h >> SH), "s"(tw_addr));
              c.sa = (uint32_t)v << BITS; c.sb = (uint32_t)c.h << BITS;
            }
            uint32_t fb;
            {
              const LdsWords pw = (LdsWords)c.pa; const LdsWords tw = (LdsWords)c.ta;
              const uint32_t d0w = __builtin_amdgcn_alignbit(pw[1], pw[0], c.sa) ^ __builtin_amdgcn_alignbit(tw[1], tw[0], c.sb);
              asm("v_ffbl_b32 %0, %1" : "=v"(fb) : "v"(d0w));       // (0xFFFFFFFF for 0: "all equal" is a huge count)
            }
            int adv;
            asm("v_min3_i32 %0, %1, %2, %3" : "=v"(adv) : "v"((int)(fb >> BITS)), "v"(c.rem), "v"(cap));
            c.h += adv;
            // a whole word matched (a valid cell with at least a word to go): the run may go on
            c.more = adv == PER;
            return c;
          };
          auto back = [&](auto uc, auto partial_tag, const unsigned long long act, ChunkState& c) {
            constexpr int O = decltype(uc)::value * NT;
            constexpr bool PARTIAL = decltype(partial_tag)::value;
            if (__builtin_amdgcn_ballot_w64(c.more) != 0ull) {
              // The lanes whose run goes on (a whole word matched, bases left) stay in the loop, the others leave it through the
              // execution mask: one back-edge, and no lane has to be kept inert.  togo = hmax - h of the lane while it is inside,
              // so nothing but togo is carried: h follows from it when the lane leaves.  10 vector instructions and the two LDS
              // reads per further word (a ballot loop with togo kept at 0 in the lanes that were done: 14 and three branches).
              // (formed here, behind the branch: the full chunk does not pay for the test)
              int togo = c.rem - PER;
              asm volatile("" : "+v"(togo));
              if (c.more && togo > 0) {
                int m;
                for (;;) {
                  c.pa += 4; c.ta += 4;
                  const LdsWords pw = (LdsWords)c.pa; const LdsWords tw = (LdsWords)c.ta;
                  const uint32_t d = __builtin_amdgcn_alignbit(pw[1], pw[0], c.sa) ^ __builtin_amdgcn_alignbit(tw[1], tw[0], c.sb);
                  uint32_t fb;
                  asm("v_ffbl_b32 %0, %1" : "=v"(fb) : "v"(d));
                  // (first mismatch or bases left, whichever is less; more than a word: the word matched and the run goes on)
                  m = min((int)(fb >> BITS), togo);
                  togo -= PER;      // (before the test: one register for togo, the last step is taken back below)
                  asm volatile("" : "+v"(togo));      // (or the compiler keeps the value from before the step in a second one: a v_mov per word)
                  if (m <= PER) break;
                }
                c.h = (c.hmax + m - PER) - togo;
              }
            }
            auto stores = [&](const int mv, const int ins_c, const int del_t) {
              w_m[O + 1] = (OffT)mv;
              w_i[O + 1] = (OffT)(ins_c >> 16);     // (high halves: ds_write_b16_d16_hi, no unpacking)
              w_d[O + 1] = (OffT)(del_t >> 16);
              if constexpr (BT) {
                // (a 32-bit sum: the store keeps its scalar base + 32-bit vector offset form for every chunk -- a 64-bit sum is a vector pair add)
                if constexpr (TILED) codes[(size_t)(t_off + (uint32_t)(O * 4))] = (uint8_t)c.code;
                else codes[O] = (uint8_t)c.code;
              }
            };
            if constexpr (PARTIAL && MASKED_LAST) {
              // The lanes beyond hi store nothing.  Their cells hold NULL already (the ring invariant: a row holds NULL outside the limits
              // it was last written with -- a growing row's slot held a narrower row before, and once a limit can move inwards
              // clear_guards NULLs the dm cells beyond each end), exactly what the cells below lo rely on, which no lane ever covers.
              // (touch: a scalar, formed outside the masked part; the lanes beyond hi are taken out of it with the mask itself)
              touch |= __builtin_amdgcn_ballot_w64(c.h == c.hmax) & act;
              if (__builtin_amdgcn_inverse_ballot_w64(act)) stores(c.h, c.ins_c, c.del_t);
            } else if constexpr (PARTIAL) {
              const bool active = __builtin_amdgcn_inverse_ballot_w64(act);
              const int mv = active ? c.h : OffNull<OffT>::value;
              touch |= __builtin_amdgcn_ballot_w64(mv == c.hmax);      // (a NULL never equals it)
              stores(mv, active ? c.ins_c : (int)0x80000000u, active ? c.del_t : (int)0x80000000u);
            } else {
              touch |= __builtin_amdgcn_ballot_w64(c.h == c.hmax);      // (a NULL never equals it)
              stores(c.h, c.ins_c, c.del_t);
            }
          };
          auto chunk = [&](auto uc, auto partial_tag, const unsigned long long act) {
            ChunkState c = front(uc);
            back(uc, partial_tag, act, c);
          };
          auto chunk_pair = [&](auto uc, auto uc2, auto partial2_tag, const unsigned long long act2) {
            ChunkState c0 = front(uc), c1 = front(uc2);
            back(uc, std::false_type{}, 0ull, c0);
            back(uc2, partial2_tag, act2, c1);
          };
          // chunks 0..3 of the group, nested so that every decision is one scalar compare and branch
          more_groups = false;
          auto from = [&](auto&& self, auto uc) -> void {
            constexpr int Uc = decltype(uc)::value;
            const int n_act = left - Uc * NT;       // cells of the row from this wave's chunk on (wave-uniform)
            if (n_act >= 64) {
              if constexpr (Uc < 3 && PAIRED) {
                // this chunk and, where the row goes on, the next one of this wave together
                const int n2 = n_act - NT;
                if (n2 >= 64) {
                  chunk_pair(uc, std::integral_constant<int, Uc + 1>{}, std::false_type{}, 0ull);
                  if constexpr (Uc + 1 < 3) { if (n2 > NT) self(self, std::integral_constant<int, Uc + 2>{}); }
                  else more_groups = n2 > NT;
                } else if (n2 > 0) {
                  chunk_pair(uc, std::integral_constant<int, Uc + 1>{}, std::true_type{}, (1ull << n2) - 1ull);
                } else {
                  chunk(uc, std::false_type{}, 0ull);
                }
              } else {
              chunk(uc, std::false_type{}, 0ull);
              if constexpr (Uc < 3) { if (n_act > NT) self(self, std::integral_constant<int, Uc + 1>{}); }
              else more_groups = n_act > NT;
              }
            } else if (NW == 1 || n_act > 0) {
              chunk(uc, std::true_type{}, (1ull << n_act) - 1ull);
            }
          };
          from(from, std::integral_constant<int, 0>{});
          return more_groups;
        };
        // (several waves: each one's count of remaining cells starts at its own first diagonal)
        const int left0 = wm1 + 1 - ((NW == 1) ? 0 : __builtin_amdgcn_readfirstlane(stid & ~63));
        // (`codes` is advanced in place and put back: a second copy of the 64-bit address would not fit the registers)
        int kq = stid + lo, left = left0;
        if constexpr (NW == 1) {
          if (__builtin_expect(group(kq, codes, left), 0)) {
            // (wider than four chunks: rare in this tier, kept out of the way of the common case)
            constexpr uint32_t STEP = TILED ? 0u : 4u * NT;      // (TILED: the byte's place follows from kq, the tile row does not move)
            uint32_t adv = 0;
            do { kq += 4 * NT; codes += STEP; adv += STEP; left -= 4 * NT; } while (group(kq, codes, left));
            codes -= adv;
          }
        } else {
          uint32_t adv = 0;
          while (group(kq, codes, left)) { kq += 4 * NT; codes += 4 * NT; adv += 4u * NT; left -= 4 * NT; }
          codes -= adv;
        }
      };
