"""The per-score work of the lean cells that is not cells (align/cells_hot.inc): the last chunk of a row storing under its lane mask
(offsets into the ring, origin bytes into tiles or rows -- and what the backtrace kernels then read there), the run continuation as
a loop over the execution mask.  Every result -- scores and CIGAR bytes -- against the CPU checker."""
import random

import numpy as np
import pytest

import oracle_lib
import wfagpu

pytestmark = pytest.mark.gpu

PEN = (2, 3, 1)


def _check(al, buf, meta, pen, max_error, want, idx=None):
    s, c = al.align(al.upload(buf, meta), pen, max_error=max_error, compute_cigar=True)
    so, co = want
    if idx is not None:
        so, co = so[idx], [co[i] for i in idx]
    assert np.array_equal(s, so), (pen, max_error, np.nonzero(s != so)[0][:8])
    assert c == co, (pen, max_error, [i for i in range(len(c)) if c[i] != co[i]][:8])


def _mutate(rng, n, length, err, indel_frac):
    """n pairs: a random text and a pattern with length * err edits, indel_frac of them single-base insertions and deletions"""
    out = []
    for _ in range(n):
        t = bytes(rng.choice(b"ACGT") for _ in range(length))
        p = bytearray(t)
        for _ in range(int(length * err)):
            at = rng.randrange(len(p))
            if rng.random() >= indel_frac:
                p[at] = rng.choice(b"ACGT")
            elif rng.random() < 0.5:
                del p[at]
            else:
                p.insert(at, rng.choice(b"ACGT"))
        out.append((bytes(p), t))
    return out


@pytest.fixture(scope="module")
def edges():
    """256 pairs of 400 bp at 12 %: under (2,3,1) every pair's rows grow by two diagonals a score through 63, 65, 127 and 129 cells
    (last-chunk masks of 63 lanes and of 1, the second chunk's first lane) and, clipped by the window of max_error 200, through the
    even widths (a full last chunk)."""
    buf, meta = wfagpu.generate_pairs(256, 400, 0.12, seed=1212)
    want = {pen: oracle_lib.oracle_batch(buf, meta, pen, cigar=True, nthreads=8)[:2] for pen in (PEN, (5, 3, 2))}
    return buf, meta, want


@pytest.fixture(scope="module")
def exact():
    al = wfagpu.DeviceAligner(0, no_auto_budget=1)
    yield al
    al.close()


def test_chunk_edges(exact, edges):
    buf, meta, want = edges
    assert want[PEN][0].min() > 128 // 2      # (a score s has a row of 2 s + 1 cells: every pair gets past 129)
    _check(exact, buf, meta, PEN, 200, want[PEN])
    st = exact.stats()
    assert st.pairs_tier[0] == len(meta), list(st.pairs_tier)      # (the one-wave tier: tiles)


@pytest.mark.parametrize("slack", [0, 3])
def test_shrinking_rows(exact, edges, slack):
    """Budgets equal to each pair's own score (and 3 more): the reach of the budget shrinks the rows from half the score on, the
    masked stores of the last chunk and the guard cells' re-NULLing together keep the ring invariant."""
    buf, meta, want = edges
    pairs = wfagpu.pairs_from_layout(buf, meta)
    so = want[PEN][0]
    groups = {}
    for i in range(len(pairs)):
        groups.setdefault(int(so[i]), []).append(i)
    for score, idx in sorted(groups.items()):
        sb, sm = wfagpu.layout_pairs([pairs[i] for i in idx])
        _check(exact, sb, sm, PEN, score + slack, want[PEN], idx)
        assert exact.stats().pairs_retried == 0, (score, slack)


def test_budget_misses_are_rerun(exact, edges):
    """The median score as everybody's budget: half the batch finishes under a tight budget, the other half misses it and is re-run."""
    buf, meta, want = edges
    so = want[PEN][0]
    me = int(np.median(so))
    _check(exact, buf, meta, PEN, me, want[PEN])
    assert exact.stats().pairs_retried == int((so > me).sum()) > 0


@pytest.fixture(scope="module")
def walks():
    """Paths for the tile readers: scores below and above 124 (the one-kernel backtrace's bound), and pairs at 50 % indels whose
    paths wander over the diagonals -- across tile columns (d & 15 = 15 -> 0) and groups of scores (s & 3 = 3 -> 0) both ways."""
    rng = random.Random(4242)
    low = _mutate(rng, 96, 400, 0.03, 0.5) + _mutate(rng, 32, 400, 0.05, 1.0)
    high = _mutate(rng, 96, 400, 0.20, 0.5) + _mutate(rng, 32, 400, 0.16, 1.0)
    out = {}
    for name, pairs in (("low", low), ("high", high)):
        buf, meta = wfagpu.layout_pairs(pairs)
        out[name] = (buf, meta, oracle_lib.oracle_batch(buf, meta, PEN, cigar=True, nthreads=8)[:2])
    return out


@pytest.mark.parametrize("trace_mode", [0, 1])
def test_tile_readers(walks, trace_mode):
    al = wfagpu.DeviceAligner(0, no_auto_budget=1, trace_mode=trace_mode)
    try:
        buf, meta, want = walks["low"]
        assert want[0].max() <= 124
        _check(al, buf, meta, PEN, 124, want)
        assert al.stats().pairs_tier[0] == len(meta)
        buf, meta, want = walks["high"]
        assert want[0].min() > 124 and want[0].max() <= 400
        _check(al, buf, meta, PEN, 400, want)
        assert al.stats().pairs_tier[0] == len(meta)
    finally:
        al.close()


def test_wave_per_alignment_walker_reads_tiles():
    """8 pairs of 6 kbp at 3 %: too long to stage 64 pairs a wavefront, the wave-per-alignment kernel walks them -- a row of 32 origin
    bytes per lane out of two tiles -- on the one-wave tier (t0_min_blocks 1: the planner would give rings of this size four waves)."""
    buf, meta = wfagpu.generate_pairs(8, 6000, 0.03, seed=63)
    want = oracle_lib.oracle_batch(buf, meta, PEN, cigar=True, nthreads=8)[:2]
    me = int(want[0].max()) + 8
    assert me <= 1000      # (a window of me - 2 diagonals, at most 1024: the one-wave tier)
    al = wfagpu.DeviceAligner(0, no_auto_budget=1, t0_min_blocks=1)
    try:
        _check(al, buf, meta, PEN, me, want)
        st = al.stats()
        assert st.pairs_tier[0] == len(meta) and st.pairs_retried == 0, list(st.pairs_tier)
    finally:
        al.close()


def test_more_than_four_chunks_per_row(exact):
    """32 pairs of 1 kbp at 20 %: rows wider than 256 cells, the cells' group() runs again"""
    buf, meta = wfagpu.generate_pairs(32, 1000, 0.20, seed=2020)
    want = oracle_lib.oracle_batch(buf, meta, PEN, cigar=True, nthreads=8)[:2]
    assert want[0].max() > 128 and want[0].max() <= 600
    _check(exact, buf, meta, PEN, 600, want)


def test_byte_compare_class(exact):
    """64 pairs of 400 bp with N bytes sprinkled in: the byte-compare instantiation (four bytes a step in the run continuation)"""
    rng = random.Random(78)
    pairs = []
    for p, t in _mutate(rng, 64, 400, 0.06, 0.3):
        p, t = bytearray(p), bytearray(t)
        for _ in range(3):
            p[rng.randrange(len(p))] = ord("N")
            t[rng.randrange(len(t))] = ord("N")
        pairs.append((bytes(p), bytes(t)))
    pairs += [(b"ACGN" * 100, b"ACGN" * 100), (b"N" * 400, b"N" * 399 + b"A")]      # (long runs of the byte-compare class)
    buf, meta = wfagpu.layout_pairs(pairs)
    want = oracle_lib.oracle_batch(buf, meta, PEN, cigar=True, nthreads=8)[:2]
    _check(exact, buf, meta, PEN, 300, want)
    assert exact.stats().pairs_raw == len(pairs)


@pytest.mark.parametrize("pen,min_tier", [((5, 3, 2), 0), (PEN, 1), (PEN, 2), ((5, 3, 2), 1)])
def test_shared_cells_elsewhere(edges, pen, min_tier):
    """The same cells under a gap extension of 2 (loop_lean_any.inc) and on the four- and sixteen-wave tiers (rows behind a row table:
    their walk is untouched), budgets wide and tight."""
    buf, meta, want = edges
    al = wfagpu.DeviceAligner(0, no_auto_budget=1, min_tier=min_tier)
    try:
        for me in (int(want[pen][0].max()), 3 * int(want[pen][0].max()) // 2):
            _check(al, buf, meta, pen, me, want[pen])
            st = al.stats()
            assert sum(st.pairs_tier[t] for t in range(min_tier)) == 0, list(st.pairs_tier)
    finally:
        al.close()


def test_long_runs(exact):
    """Runs of 1000 and 500 bases in the continuation loop, and runs that end exactly on a sequence end: identical pairs, a mismatch
    at base 500, a text one base longer (the run limit is the pattern's end), lengths on both sides of a multiple of 16."""
    rng = random.Random(1000)
    pairs = []
    for i in range(64):
        t = bytes(rng.choice(b"ACGT") for _ in range(1000 - (i & 15)))
        pairs.append((t, t))
    for i in range(64):
        t = bytes(rng.choice(b"ACGT") for _ in range(1000 + (i & 15)))
        p = bytearray(t)
        p[500] = ord("A") if t[500] != ord("A") else ord("C")
        pairs.append((bytes(p), t))
    for i in range(16):
        t = bytes(rng.choice(b"ACGT") for _ in range(992 + i))
        pairs += [(t[:-1], t), (t, t[:-1]), (t[1:], t)]
    buf, meta = wfagpu.layout_pairs(pairs)
    want = oracle_lib.oracle_batch(buf, meta, PEN, cigar=True, nthreads=8)[:2]
    assert list(want[0][:64]) == [0] * 64 and list(want[0][64:128]) == [2] * 64
    _check(exact, buf, meta, PEN, 100, want)
