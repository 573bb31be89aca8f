"""A Python model of the wf-adaptive score step (wfa-gpu_amd/csrc/align/loop_careful_ad.inc) as it is written -- limits from the row book,
clipping by the sequences, trimmed limits of M, I and D, WFA2's cut-off, I and D narrowed to M's limits, origin codes and the backward walk
-- run against WFA2's stored answers (tests/golden/wfadaptive.<set>.alg): mismatching scores and CIGARs per set, once narrowing I and D
behind every cut-off call (WFA2's code, what the kernel does) and once only behind due ones.  No GPU needed; a minute per 400 short pairs.
   scratch/wfadaptive_model.py [set ...]      (default: small)"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import wfadaptive_ref as wa

NULL = -(1 << 30)


def lcp(p, t, v, h):
    n = 0
    while v + n < len(p) and h + n < len(t) and p[v + n] == t[h + n]:
        n += 1
    return n


def align(p, t, pen, heur, equate_always=True):
    x, o, e = pen
    oe = o + e
    dm = max(x, oe) + 1
    min_len, thr, steps = heur
    plen, tlen = len(p), len(t)
    kend = tlen - plen
    M, I, D, CODE = {}, {}, {}, {}

    def row(lo, hi, vals):
        return None if lo > hi else (lo, hi, vals)

    def get(r, lo_all, ks):
        out = np.full(len(ks), NULL, dtype=np.int64)
        if r is None:
            return out
        lo, hi, (base, vals) = r
        sel = (ks >= lo) & (ks <= hi)
        out[sel] = vals[ks[sel] - base]
        return out

    h0 = lcp(p, t, 0, 0)
    M[0] = (0, 0, (0, np.array([h0])))
    CODE[0] = (0, np.array([0]), np.array([0]), np.array([h0]))
    if kend == 0 and h0 >= tlen:
        return 0, "%dM" % h0 if h0 else ""
    steps_wait = steps - 1
    if steps_wait <= 0 and 1 >= min_len:
        steps_wait = steps
    s = 0
    null_steps = 0
    while True:
        s += 1
        if s > 100000:
            return -1, None
        mx, mo, ie, de = M.get(s - x), M.get(s - oe), I.get(s - e), D.get(s - e)
        if mx is None and mo is None and ie is None and de is None:
            null_steps += 1
            if null_steps > dm:
                return -2, None
            continue
        null_steps = 0
        los = [r[0] + d for r, d in ((mx, 0), (mo, -1), (ie, 1), (de, -1)) if r is not None]
        his = [r[1] + d for r, d in ((mx, 0), (mo, 1), (ie, 1), (de, -1)) if r is not None]
        lo, hi = max(min(los), -plen), min(max(his), tlen)
        if lo > hi:
            continue
        have_i = not (mo is None and ie is None)
        have_d = not (mo is None and de is None)
        ks = np.arange(lo, hi + 1)
        m_x = get(mx, lo, ks)
        m_ol, m_or = get(mo, lo, ks - 1), get(mo, lo, ks + 1)
        i_e, d_e = get(ie, lo, ks - 1), get(de, lo, ks + 1)
        ins = np.maximum(m_ol, i_e) + 1
        dl = np.maximum(m_or, d_e)
        mis = m_x + 1
        mv0 = np.maximum(dl, np.maximum(mis, ins))
        code = np.where(i_e >= m_ol, 1, 0) | np.where(d_e >= m_or, 2, 0)
        code |= np.where(mis == mv0, 12, np.where(dl == mv0, 8, 4))
        ok = (mv0 >= 0) & (mv0 <= tlen) & (mv0 - ks >= 0) & (mv0 - ks <= plen)
        mv = np.full(len(ks), NULL, dtype=np.int64)
        for j in np.nonzero(ok)[0]:
            mv[j] = mv0[j] + lcp(p, t, int(mv0[j] - ks[j]), int(mv0[j]))
        i_ok = (ins >= 0) & (ins <= tlen) & (ins - ks >= 0) & (ins - ks <= plen) & have_i
        d_ok = (dl >= 0) & (dl <= tlen) & (dl - ks >= 0) & (dl - ks <= plen) & have_d

        def lim(b):
            nz = np.nonzero(b)[0]
            return (lo + nz[0], lo + nz[-1]) if len(nz) else (1, -1)
        (mlo, mhi), (ilo, ihi), (dlo, dhi) = lim(ok), lim(i_ok), lim(d_ok)
        dist = np.where(mv >= 0, np.maximum(plen - (mv - ks), tlen - mv), 1 << 30)
        min_d = min(int(dist.min()), max(plen, tlen))
        done = lo <= kend <= hi and mv[kend - lo] >= tlen
        CODE[s] = (lo, code, mv0, mv)
        if not done and mlo <= mhi:
            steps_wait -= 1
            cut = False
            if steps_wait <= 0 and mhi - mlo + 1 >= min_len:
                within = np.nonzero((dist - min_d <= thr) & (ks >= mlo) & (ks <= mhi))[0]
                f = lo + within[0] if len(within) else 1 << 30
                l = lo + within[-1] if len(within) else -(1 << 30)
                nlo = min(f, max(mlo, min(kend, mhi)))
                nhi = max(l, min(mhi, max(kend, nlo)))
                mlo, mhi = nlo, nhi
                steps_wait = steps
                cut = True
            if equate_always or cut:
                ilo, ihi, dlo, dhi = max(ilo, mlo), min(ihi, mhi), max(dlo, mlo), min(dhi, mhi)
        M[s], I[s], D[s] = row(mlo, mhi, (lo, mv)), row(ilo, ihi, (lo, ins)), row(dlo, dhi, (lo, dl))
        for old in (s - dm - 2,):
            M.pop(old, None); I.pop(old, None); D.pop(old, None)
        if done:
            break
    final = s
    # backtrace
    ops = []
    k, st = kend, "M"
    while True:
        lo, code, mv0, mv = CODE[s]
        c = int(code[k - lo])
        if st == "M":
            ops.append("M" * int(mv[k - lo] - mv0[k - lo]))
            if s == 0:
                break
            m = c & 12
            if m == 12:
                ops.append("X"); s -= x
            elif m == 8:
                st = "D"
            else:
                st = "I"
        elif st == "I":
            ops.append("I")
            if c & 1:
                s -= e; k -= 1
            else:
                s -= oe; k -= 1; st = "M"
        else:
            ops.append("D")
            if c & 2:
                s -= e; k += 1
            else:
                s -= oe; k += 1; st = "M"
    txt = "".join(reversed(ops))
    out, i = [], 0
    while i < len(txt):
        j = i
        while j < len(txt) and txt[j] == txt[i]:
            j += 1
        out.append("%d%s" % (j - i, txt[i])); i = j
    return final, "".join(out)


if __name__ == "__main__":
    names = sys.argv[1:] or ["small"]
    for name in names:
        g = wa.read_golden(name)
        for eq in (True, False):
            bad_s = bad_c = 0
            for i, ((p, t), heur, pen) in enumerate(zip(g["pairs"], g["heurs"], g["pens"])):
                s, c = align(p, t, pen, heur, eq)
                bad_s += s != g["scores"][i]
                bad_c += c != g["cigars"][i]
            print(name, "equate_always" if eq else "equate_on_cut", "score mismatches", bad_s, "cigar mismatches", bad_c, "of", len(g["pairs"]))
