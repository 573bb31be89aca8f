"""The lean score loop of the exact end-to-end two-piece kernels (align/loop_lean_2p.inc, align/cells_hot_2p.inc; LDS tiers 0, 1, 2).
Scores against the plain dynamic program (affine2p_ref.dp_affine2p_score); CIGARs valid with cost == score and byte for byte those of
the same call under tuning.careful_only, whose bytes the goldens of test_gpu_affine2p.py pin to WFA2's."""
import random

import numpy as np
import pytest

import affine2p_ref as a2
import wfagpu

pytestmark = pytest.mark.gpu

PEN = a2.DEFAULT_PEN      # (4, 6, 2, 24, 1)


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


def _dp(pairs, pen):
    return np.array([a2.dp_affine2p_score(p, t, pen) for p, t in pairs], dtype=np.int64)


@pytest.fixture(scope="module")
def careful():
    al = wfagpu.DeviceAligner(0, careful_only=1)
    yield al
    al.close()


@pytest.fixture(scope="module")
def lean():
    al = wfagpu.DeviceAligner(0)
    yield al
    al.close()


@pytest.fixture(scope="module")
def edges():
    """48 pairs of 400 bp at 12 %, and the dynamic program's scores under every penalty set of affine2p_ref.PENS"""
    pairs = _mutate(random.Random(2020), 48, 400, 0.12, 0.3)
    return pairs, {pen: _dp(pairs, pen) for pen in a2.PENS}


def _check(al, careful, pairs, pen, max_error, want, tiers=(0, 1, 2), cigar=True):
    """One call on `al`: scores == want, on the given tiers; CIGARs valid, cost == score, and the careful loop's bytes."""
    buf, meta = wfagpu.layout_pairs(pairs)
    s, c = al.align(al.upload(buf, meta), None, max_error=max_error, compute_cigar=cigar, affine2p=pen)
    st = al.stats()
    assert sum(st.pairs_tier[t] for t in tiers) == len(pairs) or st.pairs_retried, (tiers, list(st.pairs_tier))
    assert np.array_equal(s, want), (pen, max_error, np.nonzero(s != want)[0][:8])
    if cigar:
        _, cc = careful.align(careful.upload(buf, meta), None, max_error=max_error, compute_cigar=True, affine2p=pen)
        for i, (p, t) in enumerate(pairs):
            ok, cost = a2.check_cigar2p(p, t, c[i], pen)
            assert ok and cost == want[i] and c[i] == cc[i], (pen, i, c[i], cc[i])
    return st


@pytest.mark.parametrize("cigar", [False, True])
@pytest.mark.parametrize("pen,more", [((2, 3, 1, 40, 1), True), (PEN, False)])
def test_lean_loop_runs(lean, careful, edges, pen, more, cigar):
    """As shipped against careful_only: the same scores and CIGAR bytes, and another count of cells.  Without the lean loop both calls
    run the same loop and count the same cells.  Under (2,3,1,40,1) the lean rows are WFA2's rows plus the scores WFA2 has no wavefront
    for (1 and 3: one NULL cell each): more cells.  Under (4,6,2,24,1) WFA2's own limits are the wider ones: from score o2 + e2 on its
    I2 / D2 carry the limits of the whole wavefront and push them out by a diagonal a score, cells no gap of that score's cost reaches
    and the lean interval [-U(s), U(s)] leaves out: fewer cells."""
    pairs, want = edges
    cells = _check(lean, careful, pairs, pen, 600, want[pen], cigar=cigar).cells
    buf, meta = wfagpu.layout_pairs(pairs)
    s, _ = careful.align(careful.upload(buf, meta), None, max_error=600, compute_cigar=cigar, affine2p=pen)
    assert np.array_equal(s, want[pen])
    print(f"cells as shipped {cells}, careful_only {careful.stats().cells}")
    assert (cells > careful.stats().cells) if more else (cells < careful.stats().cells), (cells, careful.stats().cells)


@pytest.mark.parametrize("cigar", [False, True])
@pytest.mark.parametrize("tier", [0, 1, 2])
def test_chunk_edges(careful, edges, tier, cigar):
    """Scores above 100: the rows, 2 U(s) + 1 cells wide with U(s) = s - 24 from score 42 on, grow through 63, 65, 127 and 129 cells
    (last-chunk masks of 63 lanes and of 1, the second chunk's first lane) on one, four and sixteen waves."""
    pairs, want = edges
    assert want[PEN].min() > 100
    al = wfagpu.DeviceAligner(0, **({"t0_min_blocks": 1} if tier == 0 else {"min_tier": tier}))
    try:
        # (the one-wave tier takes rings up to 40 KB: a budget just above the scores keeps the 37 rows that narrow)
        _check(al, careful, pairs, PEN, 600 if tier else int(want[PEN].max()) + 1, want[PEN], tiers=(tier,), cigar=cigar)
    finally:
        al.close()


@pytest.mark.parametrize("pen", a2.PENS)
def test_penalty_shapes(lean, careful, edges, pen):
    """e2 = 2, o1 + e1 > x, x > o1 + e1, a second piece that wins late: each set has another farthest M read and other gap-ring depths."""
    pairs, want = edges
    _check(lean, careful, pairs, pen, int(want[pen].max()) + 1, want[pen])


@pytest.mark.parametrize("slack", [0, 3])
def test_shrinking_rows(lean, careful, edges, slack):
    """Budgets equal to each pair's own score (and 3 more): the reach interval closes from half-way on, the masked stores of the last
    chunk and the re-NULLing of the guard cells of five slots together keep the ring invariant."""
    pairs, want = edges
    groups = {}
    for i, sc in enumerate(want[PEN]):
        groups.setdefault(int(sc), []).append(i)
    for score, idx in sorted(groups.items()):
        st = _check(lean, careful, [pairs[i] for i in idx], PEN, score + slack, want[PEN][idx])
        assert st.pairs_retried == 0, (score, slack)


def test_budget_misses_are_rerun(lean, careful, edges):
    """The median score as everybody's budget: half the batch finishes under a tight budget, the other half misses it and is re-run."""
    pairs, want = edges
    me = int(np.median(want[PEN]))
    st = _check(lean, careful, pairs, PEN, me, want[PEN])
    assert st.pairs_retried == int((want[PEN] > me).sum()) > 0


def test_hand_over(lean, careful):
    """Where the lean loop hands over: never entered (identical pairs touch at score 0), after one mismatch, after a one-base gap to the
    end diagonal, and after a 70-base insertion or deletion that only the second piece pays for -- the path runs on I2 / D2 up to the
    touch and the first careful score reads rows the lean loop wrote; lengths on both sides of a multiple of 16."""
    rng = random.Random(70)
    pairs = []
    for i in range(8):
        t = bytes(rng.choice(b"ACGT") for _ in range(316 + i))
        p = bytearray(t)
        p[150] = ord("A") if t[150] != ord("A") else ord("C")
        gap = bytes(rng.choice(b"ACGT") for _ in range(70))
        pairs += [(t, t), (bytes(p), t), (t[:-1], t), (t, t[:-1]), (t[1:], t), (t[:150] + t[220:], t), (t[:150] + gap + t[150:], t)]
    want = _dp(pairs, PEN)
    assert list(want[:7]) == [0, 4, 8, 8, 8, 24 + 70, 24 + 70]
    _check(lean, careful, pairs, PEN, 200, want)


def test_byte_compare_class(lean, careful):
    """Pairs with N bytes: the byte-compare instantiations (four bytes a step in the shared run continuation)."""
    rng = random.Random(78)
    pairs = []
    for p, t in _mutate(rng, 16, 300, 0.06, 0.3):
        p, t = bytearray(p), bytearray(t)
        for _ in range(3):
            p[rng.randrange(len(p))] = ord("N")
            t[rng.randrange(len(t))] = ord("N")
        pairs.append((bytes(p), bytes(t)))
    pairs += [(b"ACGN" * 80, b"ACGN" * 80), (b"N" * 320, b"N" * 319 + b"A")]
    st = _check(lean, careful, pairs, PEN, 300, _dp(pairs, PEN))
    assert st.pairs_raw == len(pairs)
