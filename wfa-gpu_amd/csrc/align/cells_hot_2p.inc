// cells_hot_2p.inc -- hot_cells_2p: the lean cells of one score under two-piece penalties (16-bit LDS tiers 0, 1 and 2), for the regime
// before any M cell has touched a sequence end (loop_lean_2p.inc): no overrun tests, no saturation, no trimming.
// Textually included in the body of wfa_align_kernel (../align_kernel.hip) behind cells_hot.inc, whose address-space typedefs it uses.
// The extend part is cells_hot.inc's, as two lambdas of this file (hot2p_extend_first, hot2p_extend_more): calling them from hot_cells too
// changed 140 instructions of the gap-affine kernels, which must stay what they are (EXPERIMENTS.md R20), so cells_hot.inc keeps its text.
// Reads: rows as LDS byte addresses of their diagonal 0, pw_addr / tw_addr (staged sequences), a_hm (run-limit row, one-wave tier), stid.
// Writes: M / I1 / D1 / I2 / D2 of score s, one BT2_* origin byte per cell through `codes`, touch.
      // ---- Seven LDS reads per cell -- M[s-x][k], M[s-o1-e1][k-1], [k+1], M[s-o2-e2][k-1], [k+1], I1[s-e1][k-1], D1[s-e1][k+1], I2[s-e2][k-1],
      // D2[s-e2][k+1]: the two neighbours of an M row come from one lane base -- and five stores.  Every row is addressed as one lane base
      // (cell kq - 1 of the row) plus immediates; the D rows sit d_delta (d2_delta) bytes behind their I rows.
      // Values and ties.  Each candidate is carried as (offset << 16 | tag) and every choice is one signed max: on equal offsets the larger
      // tag wins.  The tags are the BT2_* bits themselves: an extension carries its piece's EXT bit on top of the tag of the opening, so
      // extension wins or ties exactly where the careful cells say i_e >= m_ol (cells_generic.inc; wavefront_compute_affine2p.c:173-232), and
      // the M sources order as WFA2's M > D2 > D1 > I2 > I1 (BT2_M_X = 5 << 4 ... BT2_M_I1 = 1 << 4; :251-270) whatever EXT bits ride below
      // them.  Every tag holds a source >= 1 << 4 = 16 >= PER, so v_med3(value, 0, PER) is PER for a valid cell and 0 for a NULL one as in
      // hot_cells, and bit 15 is clear.  The origin byte: bits 6:4 of the winner, and each EXT bit from the tagged value of its own component.
      // first step of the run of the cells of chunk uc, straight-line: c.hmax set, mv_t = the tagged M value (offset << 16 | tag, every tag of
      // a valid cell >= PER, bit 15 clear), kq = the lane's diagonal in chunk 0, kq16 = kq << 16
      auto hot2p_extend_first = [&](auto uc, auto& c, const int mv_t, const int kq, const int kq16, const uint32_t pw_addr, const uint32_t tw_addr) {
        constexpr int SH = RAW ? 2 : 4, PER = 1 << SH, BITS = RAW ? 3 : 1;
        constexpr int O = decltype(uc)::value * NT;
        [[maybe_unused]] const int k = kq + O;
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
          // The tag occupies the low bits and bit 15 is clear, so (x >> 15) is twice the high half.)
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
      };
      // the (rare) continuation of the runs of a chunk: c.h of every lane is final afterwards
      auto hot2p_extend_more = [&](auto& c) {
        constexpr int SH = RAW ? 2 : 4, PER = 1 << SH, BITS = RAW ? 3 : 1;
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
      };
      auto hot_cells_2p = [&](const int lo, const int wm1, GlobalBytes& codes, const uint32_t a_oe, const uint32_t a_oe2, const uint32_t a_x, const uint32_t a_m,
                              const uint32_t a_ip, const uint32_t a_ic, const uint32_t d_delta, const uint32_t a_ip2, const uint32_t a_ic2, const uint32_t d2_delta,
                              const uint32_t pw_addr, const uint32_t tw_addr, const uint32_t a_hm, unsigned long long& touch) {
        constexpr int PER = RAW ? 4 : 16;
        static_assert(BT2_M_I1 >= (uint32_t)PER && ((BT2_M_MASK | BT2_D2_EXT | BT2_I2_EXT | BT2_D1_EXT | BT2_I1_EXT) & 0xFF80u) == 0, "tags: >= PER, below bit 7");
        // what a chunk carries from its front to its back (cells_hot.inc's ChunkState and the tagged I2 and D2 values)
        struct ChunkState2p { int h, rem, hmax, ins_c, del_t, ins2_c, del2_t; uint32_t pa, ta, sa, sb, code; bool more; };
        auto group = [&](const int kq, const GlobalBytes codes, const int left) -> bool {
          bool more_groups = false;
          const uint32_t vb = (uint32_t)(kq - 1) << 1;
          const int kq16 = kq << 16;
          // (one v_add each, once per score: the empty asm keeps the compiler from re-forming them in every chunk)
          uint32_t q_mo = vb + a_oe, q_mo2 = vb + a_oe2, q_mx = vb + a_x, q_wm = vb + a_m, q_ri = vb + a_ip, q_wi = vb + a_ic, q_ri2 = vb + a_ip2, q_wi2 = vb + a_ic2;
          uint32_t q_rd = q_ri + d_delta, q_wd = q_wi + d_delta, q_rd2 = q_ri2 + d2_delta, q_wd2 = q_wi2 + d2_delta, q_hm = vb + a_hm;
          asm volatile("" : "+v"(q_mo), "+v"(q_mo2), "+v"(q_mx), "+v"(q_wm), "+v"(q_ri), "+v"(q_wi), "+v"(q_ri2), "+v"(q_wi2));
          asm volatile("" : "+v"(q_rd), "+v"(q_wd), "+v"(q_rd2), "+v"(q_wd2), "+v"(q_hm));
          const LdsRow r_mo = (LdsRow)q_mo, r_mo2 = (LdsRow)q_mo2, r_mx = (LdsRow)q_mx, w_m = (LdsRow)q_wm, r_hm = (LdsRow)q_hm;
          const LdsRow r_i = (LdsRow)q_ri, w_i = (LdsRow)q_wi, r_d = (LdsRow)q_rd, w_d = (LdsRow)q_wd;
          const LdsRow r_i2 = (LdsRow)q_ri2, w_i2 = (LdsRow)q_wi2, r_d2 = (LdsRow)q_rd2, w_d2 = (LdsRow)q_wd2;
          // front: ring loads, recurrences, origin byte, first step of the run; back: run continuation, stores (as in hot_cells)
          auto front = [&](auto uc) -> ChunkState2p {
            constexpr int O = decltype(uc)::value * NT;
            ChunkState2p c;
            const int k = kq + O;
            const uint32_t u_ol = (uint16_t)r_mo[O], u_or = (uint16_t)r_mo[O + 2], u2_ol = (uint16_t)r_mo2[O], u2_or = (uint16_t)r_mo2[O + 2];
            const uint32_t u_ie = (uint16_t)r_i[O], u_de = (uint16_t)r_d[O + 2], u2_ie = (uint16_t)r_i2[O], u2_de = (uint16_t)r_d2[O + 2];
            const uint32_t u_x = (uint16_t)r_mx[O + 1];
            // min(plen + k, tlen): how far a run on this diagonal can go
            c.hmax = HM_ROW ? (int)(uint16_t)r_hm[O + 1] : min(plen + k, tlen);
            c.ins_c = max((int)((u_ol << 16) + (0x10000u | BT2_M_I1)), (int)((u_ie << 16) + (0x10000u | BT2_M_I1 | BT2_I1_EXT)));
            c.ins2_c = max((int)((u2_ol << 16) + (0x10000u | BT2_M_I2)), (int)((u2_ie << 16) + (0x10000u | BT2_M_I2 | BT2_I2_EXT)));
            c.del_t = max((int)((u_or << 16) | BT2_M_D1), (int)((u_de << 16) | (BT2_M_D1 | BT2_D1_EXT)));
            c.del2_t = max((int)((u2_or << 16) | BT2_M_D2), (int)((u2_de << 16) | (BT2_M_D2 | BT2_D2_EXT)));
            const int mis_c = (int)((u_x << 16) + (0x10000u | BT2_M_X));
            const int mv_t = max(max(c.del_t, c.del2_t), max(mis_c, max(c.ins_c, c.ins2_c)));
            c.code = 0;
            if constexpr (BT) {
              uint32_t c1, c2, c3;
              asm("v_bfi_b32 %0, 8, %1, %2" : "=v"(c1) : "v"(c.del2_t), "v"(mv_t));        // bit 3 from the D2 winner
              asm("v_bfi_b32 %0, 4, %1, %2" : "=v"(c2) : "v"(c.ins2_c), "v"(c1));          // bit 2 from the I2 winner
              asm("v_bfi_b32 %0, 2, %1, %2" : "=v"(c3) : "v"(c.del_t), "v"(c2));           // bit 1 from the D1 winner
              asm("v_bfi_b32 %0, 1, %1, %2" : "=v"(c.code) : "v"(c.ins_c), "v"(c3));       // bit 0 from the I1 winner
            }
            hot2p_extend_first(uc, c, mv_t, kq, kq16, pw_addr, tw_addr);
            return c;
          };
          auto chunk = [&](auto uc, auto partial_tag, const unsigned long long act) {
            constexpr int O = decltype(uc)::value * NT;
            constexpr bool PARTIAL = decltype(partial_tag)::value;
            ChunkState2p c = front(uc);
            hot2p_extend_more(c);
            auto stores = [&]() {
              w_m[O + 1] = (OffT)c.h;
              w_i[O + 1] = (OffT)(c.ins_c >> 16);     // (high halves: ds_write_b16_d16_hi, no unpacking)
              w_d[O + 1] = (OffT)(c.del_t >> 16);
              w_i2[O + 1] = (OffT)(c.ins2_c >> 16);
              w_d2[O + 1] = (OffT)(c.del2_t >> 16);
              if constexpr (BT) codes[O] = (uint8_t)c.code;      // (bit 7 is clear: no tag reaches it)
            };
            if constexpr (PARTIAL) {
              // The lanes beyond hi store nothing: their cells hold NULL already (the ring invariant, kept on the upper side by
              // loop_lean_2p.inc's guard clearing as cells_hot.inc says under MASKED_LAST); touch: the mask takes them out.
              touch |= __builtin_amdgcn_ballot_w64(c.h == c.hmax) & act;
              if (__builtin_amdgcn_inverse_ballot_w64(act)) stores();
            } else {
              touch |= __builtin_amdgcn_ballot_w64(c.h == c.hmax);      // (a NULL never equals it)
              stores();
            }
          };
          // chunks 0..3 of the group, nested so that every decision is one scalar compare and branch
          auto from = [&](auto&& self, auto uc) -> void {
            constexpr int Uc = decltype(uc)::value;
            const int n_act = left - Uc * NT;       // cells of the row from this wave's chunk on (wave-uniform)
            if (n_act >= 64) {
              chunk(uc, std::false_type{}, 0ull);
              if constexpr (Uc < 3) { if (n_act > NT) self(self, std::integral_constant<int, Uc + 1>{}); }
              else more_groups = n_act > NT;
            } else if (NW == 1 || n_act > 0) {
              chunk(uc, std::true_type{}, (1ull << n_act) - 1ull);
            }
          };
          from(from, std::integral_constant<int, 0>{});
          return more_groups;
        };
        // (several waves: each one's count of remaining cells starts at its own first diagonal)
        int left = wm1 + 1 - ((NW == 1) ? 0 : __builtin_amdgcn_readfirstlane(stid & ~63));
        // (`codes` is advanced in place and put back: a second copy of the 64-bit address would not fit the registers)
        int kq = stid + lo;
        uint32_t adv = 0;
        while (group(kq, codes, left)) { kq += 4 * NT; codes += 4 * NT; adv += 4u * NT; left -= 4 * NT; }
        codes -= adv;
      };
