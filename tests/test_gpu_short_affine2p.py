"""Tier 5 under two-piece penalties, end to end (short_kernel_2p.hip: groups of 16 or 32 lanes, M, I1, D1, I2 and D2 rings in registers)
through the existing doors, against WFA2's scores and CIGAR bytes (tests/golden/affine2p.*.alg; the sets are described in
tests/affine2p_ref.py) and, for the tiny pairs, against the five-matrix dynamic program and the one-wave kernels."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import affine2p_ref as a2
import wfagpu

pytestmark = pytest.mark.gpu
# the penalty sets of wfa_short_2p_supported's table, as a caller writes them (the library divides a common factor out first)
TABLE = {(4, 6, 2, 24, 1), (2, 4, 2, 12, 1), (5, 3, 4, 10, 1), (4, 6, 2, 24, 2), (3, 8, 2, 8, 2), (1, 1, 2, 4, 1), (3, 2, 3, 9, 1), (6, 9, 3, 30, 3),
         (4, 6, 2, 3, 1), (2, 1, 1, 1, 3), (4, 24, 1, 6, 2)}
gold = functools.lru_cache(None)(a2.read_golden)


def _call(al, pairs, pen, max_error, cigar=True):
    buf, meta = wfagpu.layout_pairs(pairs)
    s, c = al.align(al.upload(buf, meta), None, max_error=max_error, compute_cigar=cigar, affine2p=pen)
    return s, c, al.stats()


def _is_raw(pair):
    return bool(set(pair[0] + pair[1]) - set(b"ACGT"))


@pytest.mark.parametrize("max_error,lanes", [(30, 16), (52, 32)])
@pytest.mark.parametrize("no_fused_pack", [0, 1])
def test_small_default(max_error, lanes, no_fused_pack):
    """400 pairs of 0 to 300 bases under WFA2's defaults, score-only and with CIGARs, from ASCII and from packed words: WFA2's scores and
    bytes; every ACGT pair within the budget finishes on tier 5 on the planned lanes, every pair above it comes back."""
    g = gold(a2.ONE_PEN_SET)
    raw = sum(map(_is_raw, g["pairs"]))
    over = g["scores"] > max_error
    on5 = sum(1 for pr, o in zip(g["pairs"], over) if not o and not _is_raw(pr))
    al = wfagpu.DeviceAligner(0, no_fused_pack=no_fused_pack)
    try:
        for cigar in (False, True):
            s, c, st = _call(al, g["pairs"], a2.DEFAULT_PEN, max_error, cigar)
            assert np.array_equal(s, g["scores"]) and (not cigar or c == g["cigars"])
            assert (st.pairs_tier[5], st.pairs_raw, st.pairs_retried) == (on5, raw, int(over.sum())), list(st.pairs_tier)
            # (main_launch_tier is the call's LONGEST launch -- above, the re-run of the unrelated half on the one-wave tiers -- and
            # the byte-compare class, which launches last, leaves its own waves_per_simd_tier0: both asked of the pairs the tier finishes)
            keep = [i for i, pr in enumerate(g["pairs"]) if not over[i] and not _is_raw(pr)]
            s, c, st = _call(al, [g["pairs"][i] for i in keep], a2.DEFAULT_PEN, max_error, cigar)
            assert np.array_equal(s, g["scores"][keep]) and (not cigar or c == [g["cigars"][i] for i in keep])
            assert (st.pairs_tier[5], st.main_launch_tier, st.waves_per_simd_tier0) == (on5, 5, lanes)
    finally:
        al.close()


def _widest_budget(pen):
    """The largest budget whose window bound -- R(S) + 3 diagonals and one to spare, R(S) the longest gap S pays for -- fits 32 lanes."""
    return max(S for S in range(1, 200) if max([n for n in range(1, 40) if a2.gap_cost(n, pen) <= S], default=0) + 3 + 1 <= 32)


@pytest.mark.parametrize("name", ["small", a2.SWEEP_SET])
def test_penalty_groups(name):
    """Each penalty group under the largest budget whose window bound fits 32 lanes, with CIGARs: WFA2's bytes; pairs on tier 5 exactly
    for the sets of the table."""
    g = gold(name)
    al = wfagpu.DeviceAligner(0)
    try:
        for pen, idx in a2.groups(g).items():
            s, c, st = _call(al, [g["pairs"][i] for i in idx], pen, _widest_budget(pen))
            assert np.array_equal(s, g["scores"][idx]) and c == [g["cigars"][i] for i in idx], pen
            assert (st.pairs_tier[5] > 0) == (pen in TABLE), (pen, list(st.pairs_tier))
    finally:
        al.close()


@pytest.mark.parametrize("pen", [(1, 1, 2, 4, 1), (2, 1, 1, 1, 3)])
def test_tiny_pairs(pen):
    """All 961 pairs over {A, C} of up to four bases, and each again with one G: gap values run past a sequence's end in most of them (tier
    5 nulls them at once, WFA2 keeps them inside the row: DESIGN.md section 4.16).  The dynamic program's score, a valid CIGAR of that
    cost, and the bytes of the one-wave kernels (min_tier = 1), which the goldens pin to WFA2."""
    words = [bytes(w) for n in range(5) for w in itertools.product(b"AC", repeat=n)]
    pairs = [(p, t) for p in words for t in words]
    pairs += [(p[:len(p) // 2] + b"G" + p[len(p) // 2:], t) if i % 2 else (p, t[:len(t) // 2] + b"G" + t[len(t) // 2:]) for i, (p, t) in enumerate(pairs)]
    assert len(pairs) == 2 * 961
    al, wide = wfagpu.DeviceAligner(0), wfagpu.DeviceAligner(0, min_tier=1)
    try:
        s, c, st = _call(al, pairs, pen, 16)
        assert st.pairs_tier[5] == len(pairs) and st.pairs_retried == 0
        s1, c1, st1 = _call(wide, pairs, pen, 16)
        assert st1.pairs_tier[5] == 0 and np.array_equal(s, s1) and c == c1
        for (p, t), score, cigar in zip(pairs, s, c):
            assert score == a2.dp_affine2p_score(p, t, pen), (p, t)
            assert a2.check_cigar2p(p, t, cigar, pen) == (True, score), (p, t, cigar)
    finally:
        al.close()
        wide.close()


def test_mixed_batch():
    """2051 pairs -- small_default tiled and shuffled -- under max_error = 52: several pipeline iterations, a partial last wavefront, and
    empty, identical, over-budget and N-flagged pairs side by side."""
    g = gold(a2.ONE_PEN_SET)
    order = np.random.default_rng(20261126).permutation(2051) % len(g["pairs"])
    pairs = [g["pairs"][i] for i in order]
    over = g["scores"][order] > 52
    raw = np.array([_is_raw(pr) for pr in pairs])
    # (an arena that holds the re-run of the unrelated pairs at once: a pair that runs out of arena starts over in a pass of its own and
    # counts as retried again)
    al = wfagpu.DeviceAligner(0, arena_bytes=1 << 30)
    try:
        s, c, st = _call(al, pairs, a2.DEFAULT_PEN, 52)
        assert np.array_equal(s, g["scores"][order]) and c == [g["cigars"][i] for i in order]
        assert (st.pairs_tier[5], st.pairs_raw, st.pairs_retried) == (int((~over & ~raw).sum()), int(raw.sum()), int(over.sum())), st.sub_batches
    finally:
        al.close()


_FRESH_PROCESS = r"""
import wfagpu
lib = wfagpu.load()
buf, meta = wfagpu.generate_pairs(64, 150, 0.02, seed=11)
al = wfagpu.DeviceAligner(0)
assert lib.wfagpu_amd_prime(al.ctx) == 0
batch = al.upload(buf, meta)
al.align(batch, (2, 3, 1), max_error=14, compute_cigar=True)
al.align(batch, (4, 6, 2), max_error=200, compute_cigar=False)
al.align(batch, None, max_error=400, compute_cigar=False, affine2p=(4, 6, 2, 24, 1))
print("wide", al.stats().pairs_tier[5], lib.wfagpu_amd_debug_code_objects() & 4102)
al.align(batch, None, max_error=30, compute_cigar=False, affine2p=(4, 6, 2, 24, 1))
print("short", al.stats().pairs_tier[5] > 0, lib.wfagpu_amd_debug_code_objects() & 4100)
al.close()
"""


def test_only_a_two_piece_call_that_fits_loads_the_code_object():
    """A fresh process, score-only: after prime with nothing configured, gap-affine calls and a two-piece call under max_error = 400, bit
    12 of wfagpu_amd_debug_code_objects is clear (bit 1, the one-wave unit, is set); the call under max_error = 30 sets it and leaves bit
    2, the two-piece backtrace, clear."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _FRESH_PROCESS], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["wide", "0", "2", "short", "True", "4096"], r.stdout
