"""Two-piece gap-affine alignment on the GPU: wfagpu_amd_align_device_2p, wfagpu_amd_configure_affine2p behind the launch_alignments*
seam and the CLI, against WFA2's gap_affine_2p scores and CIGARs (tests/golden/affine2p.*, made by
tests/golden/make_golden_affine2p.py; the sets are described in tests/affine2p_ref.py)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import affine2p_ref as a2
import oracle_lib
import wfagpu
from endsfree_ref import sweep_budget_groups, sweep_over

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(wfagpu.LIB_PATH)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")
# score budgets of the first tier: above every golden score of the set (small: 662, gaps: 822, ties: 50)
MAX_ERROR = {"small": 800, "gaps": 1000, "ties": 200, a2.ONE_PEN_SET: 800}


@pytest.fixture(scope="module")
def sets():
    return {name: a2.read_golden(name) for name in a2.SETS + (a2.ONE_PEN_SET, a2.LONG_SET)}


def _run_set(al, g, cigar, max_error, only=None):
    """Every penalty group of a golden set as one call -> scores, cigars in the set's order (only: a subset of indices).  No pair is
    skipped: every index must have come back."""
    n = len(g["pairs"])
    scores = np.full(n, -12345, dtype=np.int64)
    cigars = [None] * n
    seen = 0
    stats = []
    for pen, idx in a2.groups(g).items():
        if only is not None:
            idx = [i for i in idx if i in only]
            if not idx:
                continue
        buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
        batch = al.upload(buf, meta)
        s, c = al.align(batch, None, max_error=max_error, compute_cigar=cigar, affine2p=pen)
        stats.append(al.stats())
        for j, i in enumerate(idx):
            scores[i] = s[j]
            cigars[i] = c[j] if cigar else None
        seen += len(idx)
    assert seen == (n if only is None else len(only))
    return scores, cigars, stats


def _check_set(g, scores, cigars, cigar, only=None):
    for i in (range(len(g["pairs"])) if only is None else sorted(only)):
        p, t = g["pairs"][i]
        pen = g["pens"][i]
        where = (i, len(p), len(t), pen)
        assert scores[i] == g["scores"][i], where
        if cigar:
            assert cigars[i] == g["cigars"][i], where
            ok, cost = a2.check_cigar2p(p, t, cigars[i], pen)
            assert ok and cost == scores[i], where + (cigars[i],)


@pytest.mark.parametrize("name", a2.SETS + (a2.ONE_PEN_SET,))
@pytest.mark.parametrize("cigar", [False, True])
def test_golden_sets(sets, name, cigar):
    """score == WFA2's, CIGAR == WFA2's byte for byte, valid, and its cost (gap runs priced by the cheaper piece) is the score."""
    g = sets[name]
    al = wfagpu.DeviceAligner(0)
    try:
        scores, cigars, _ = _run_set(al, g, cigar, MAX_ERROR[name])
        _check_set(g, scores, cigars, cigar)
    finally:
        al.close()


@pytest.mark.parametrize("variant", ["min_tier1", "min_tier2", "min_tier3", "max_error8", "small_arena", "trace_mode1", "trace_mode2",
                                     "trace_mode3", "trace_mode4"])
def test_gaps_and_ties_on_every_path(sets, variant):
    """The same batches forced through the wider tiers, through escalation (a budget of 8: most pairs miss it), through several
    arena-bound passes, and through every mapping of the backtrace: the same bytes."""
    kw, max_error = {}, None
    if variant.startswith("min_tier"):
        kw["min_tier"] = int(variant[-1])
    elif variant.startswith("trace_mode"):
        kw["trace_mode"] = int(variant[-1])
    elif variant == "max_error8":
        max_error = 8
    elif variant == "small_arena":
        kw["arena_bytes"] = 1 << 20      # (a fixed arena of 1 MiB: a group of `gaps` does not fit it at once)
    al = wfagpu.DeviceAligner(0, **kw)
    try:
        passes = retried = 0
        for name in ("gaps", "ties"):
            g = sets[name]
            scores, cigars, stats = _run_set(al, g, True, max_error or MAX_ERROR[name])
            _check_set(g, scores, cigars, True)
            passes = max(passes, max(st.sub_batches for st in stats))
            retried += sum(st.pairs_retried for st in stats)
            if variant.startswith("min_tier"):
                t = int(variant[-1])
                assert all(sum(st.pairs_tier[:t]) == 0 for st in stats)
        if variant == "max_error8":
            assert retried > 60
        if variant == "small_arena":
            assert passes > 1
    finally:
        al.close()


def test_one_wave_tier_and_byte_compare_class(sets):
    """ties fits the one-wave tier; the pairs of small with N / IUPAC bytes run in the byte-compare kernels (WFA2 compares bytes as they
    are)."""
    al = wfagpu.DeviceAligner(0)
    try:
        g = sets["ties"]
        scores, cigars, stats = _run_set(al, g, True, MAX_ERROR["ties"])
        _check_set(g, scores, cigars, True)
        assert sum(st.pairs_tier[0] for st in stats) == len(g["pairs"])
        g = sets["small"]
        only = {i for i, (p, t) in enumerate(g["pairs"]) if set(p + t) - set(b"ACGT")}
        assert len(only) >= 8
        for cigar in (False, True):
            scores, cigars, stats = _run_set(al, g, cigar, MAX_ERROR["small"], only=only)
            _check_set(g, scores, cigars, cigar, only=only)
            assert sum(st.pairs_raw for st in stats) == len(only)
    finally:
        al.close()


def test_sequences_beyond_16_bit_offsets(sets):
    """33.5 kbp pairs: the tier whose ring holds 32-bit offsets in global memory."""
    g = sets[a2.LONG_SET]
    al = wfagpu.DeviceAligner(0)
    try:
        for cigar in (False, True):
            scores, cigars, stats = _run_set(al, g, cigar, 3000)
            _check_set(g, scores, cigars, cigar)
            assert sum(st.pairs_tier[3] for st in stats) == len(g["pairs"])
    finally:
        al.close()


def test_equal_pieces_are_the_gap_affine_alignment(golden_dir):
    """(x, o, e, o, e) on the reference's 1 kbp pairs: scores and CIGAR bytes of wfagpu_amd_align_device under (x, o, e) on the same
    context.  (WFA2 agrees with itself here: tests/test_affine2p_cpu.py, test_wfa2_with_equal_pieces_agrees_with_its_gap_affine_self.)"""
    pairs = wfagpu.read_seq_file(os.path.join(golden_dir, "seq1k.seq"))
    buf, meta = wfagpu.layout_pairs(pairs)
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        for x, o, e in ((2, 3, 1), (5, 3, 2)):
            gold = -np.loadtxt(os.path.join(golden_dir, f"seq1k.x{x}o{o}e{e}.scores"), dtype=np.int64)
            s0, c0 = al.align(batch, (x, o, e), max_error=1000, compute_cigar=True)
            s1, c1 = al.align(batch, None, max_error=1000, compute_cigar=True, affine2p=(x, o, e, o, e))
            assert np.array_equal(s0, gold[:len(s0)])
            assert np.array_equal(s1, s0) and c1 == c0
            s2, _ = al.align(batch, None, max_error=1000, compute_cigar=False, affine2p=(x, o, e, o, e))
            assert np.array_equal(s2, s0)
    finally:
        al.close()


def test_a_second_piece_that_never_wins_gives_the_gap_affine_scores(golden_dir):
    """(x, o1, e1, 40, e1): o2 + n e2 > o1 + n e1 for every n, so the scores are those of gap-affine (x, o1, e1)."""
    pairs = wfagpu.read_seq_file(os.path.join(golden_dir, "seq1k.seq"))
    buf, meta = wfagpu.layout_pairs(pairs)
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        gold = -np.loadtxt(os.path.join(golden_dir, "seq1k.x2o3e1.scores"), dtype=np.int64)
        s, _ = al.align(batch, None, max_error=1000, compute_cigar=False, affine2p=(2, 3, 1, 40, 1))
        assert np.array_equal(s, gold[:len(s)])
    finally:
        al.close()


def test_big_batch():
    """8192 pairs of ~150 bases in one call (where a gap-affine call would draw a sample for score budgets): the scores of the same pairs
    in batches of 512, and of the dynamic program on a seeded sample of 256."""
    rng = a2.Rng(20260204)
    pairs = []
    for i in range(8192):
        p = rng.seq(rng.integer(120, 181))
        pairs.append((p, rng.mutate(p, 0.06) if i % 4 else rng.seq(rng.integer(120, 181))))
    pen = a2.DEFAULT_PEN
    al = wfagpu.DeviceAligner(0)
    try:
        buf, meta = wfagpu.layout_pairs(pairs)
        batch = al.upload(buf, meta)
        s_all, _ = al.align(batch, None, max_error=600, compute_cigar=False, affine2p=pen)
        assert al.stats().auto_budget == 0      # (no budgets from a sample under two pieces)
        parts = []
        for lo in range(0, len(pairs), 512):
            buf, meta = wfagpu.layout_pairs(pairs[lo:lo + 512])
            batch = al.upload(buf, meta)
            parts.append(al.align(batch, None, max_error=600, compute_cigar=False, affine2p=pen)[0])
        assert np.array_equal(s_all, np.concatenate(parts))
        for i in (a2.Rng(7).u64(256) % np.uint64(len(pairs))).astype(np.int64):
            assert s_all[i] == a2.dp_affine2p_score(pairs[i][0], pairs[i][1], pen), i
    finally:
        al.close()


def _launch(pairs, pen, cigar, max_error, batch_size, band=-1, band_width=0):
    lib = wfagpu.load()
    buf, meta = wfagpu.layout_pairs(pairs)
    n = len(pairs)
    res = C.POINTER(wfagpu.AlignmentResult)()
    assert lib.initialize_wfa_results(C.byref(res), n, 256 if cigar else 1)
    opt = wfagpu.Options(max_error=max_error, threads_per_block=band_width, num_workers=1, band=band, batch_size=batch_size,
                         num_alignments=n, penalties=wfagpu.Penalties(*pen), compute_cigar=cigar)
    fn = lib.launch_alignments if cigar else lib.launch_alignments_distance
    fn(buf.ctypes.data, buf.nbytes, meta.ctypes.data, res, opt, False)
    scores = np.array([res[i].error for i in range(n)], dtype=np.int64)
    cigars = [C.string_at(res[i].cigar.buffer).decode() for i in range(n)] if cigar else None
    lib.destroy_wfa_results(res, n)
    return scores, cigars


def test_configured_penalties_behind_the_launch_seam(sets):
    """wfagpu_amd_configure_affine2p: launch_alignments and launch_alignments_distance on two device slots with a batch size that cuts
    the call, the gap-affine penalties of the options ignored; a band that is asked for gives the exact results; after configure(NULL)
    the very same call gives the gap-affine (2,3,1) answers of the oracle again."""
    g = sets[a2.ONE_PEN_SET]
    buf, meta = wfagpu.layout_pairs(g["pairs"])
    ga_scores, ga_cigars, _ = oracle_lib.oracle_batch(buf, meta, (2, 3, 1), cigar=True)
    assert not np.array_equal(ga_scores, g["scores"])      # (the two models do differ on these pairs)
    try:
        wfagpu.configure_launch(virtual_devices=2)
        wfagpu.configure_affine2p(a2.DEFAULT_PEN)
        s, c = _launch(g["pairs"], (2, 3, 1), True, 800, 37)
        assert np.array_equal(s, g["scores"]) and c == g["cigars"]
        s, _ = _launch(g["pairs"], (2, 3, 1), False, 800, 37)
        assert np.array_equal(s, g["scores"])
        s, c = _launch(g["pairs"], (2, 3, 1), True, 800, 150, band=25, band_width=64)
        assert np.array_equal(s, g["scores"]) and c == g["cigars"]
        wfagpu.configure_affine2p()
        s, c = _launch(g["pairs"], (2, 3, 1), True, 800, 37)
        assert np.array_equal(s, ga_scores) and c == list(ga_cigars)
        s, _ = _launch(g["pairs"], (2, 3, 1), False, 800, 37)
        assert np.array_equal(s, ga_scores)
    finally:
        wfagpu.configure_affine2p()


def test_cli_affine2p(sets, tmp_path):
    """--affine2p with -x -c -o on small_default written as a .seq file: the output file is the golden .alg byte for byte, and the -c
    verification (gap runs priced by the cheaper piece, score against the five-table CPU program) finds nothing wrong.  A .seq file
    cannot carry an empty sequence: the two pairs of the set that have one (the empty pattern, the empty text) are left out of the
    input, and their two lines out of the golden bytes."""
    g = sets[a2.ONE_PEN_SET]
    seq = tmp_path / "nonempty.seq"
    keep = [i for i, (p, t) in enumerate(g["pairs"]) if p and t]
    assert len(keep) == len(g["pairs"]) - 2
    with open(seq, "wb") as f:
        for i in keep:
            f.write(b">" + g["pairs"][i][0] + b"\n<" + g["pairs"][i][1] + b"\n")
    out = tmp_path / "res.out"
    r = subprocess.run([CLI, "-i", str(seq), "--affine2p", ",".join(str(v) for v in a2.DEFAULT_PEN), "-e", "800", "-x", "-c",
                        "-b", "150", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Incorrect=0" in r.stderr and all(tok == "Incorrect=0" for tok in r.stderr.split() if tok.startswith("Incorrect="))
    golden_lines = open(a2.golden_path(a2.ONE_PEN_SET), "rb").read().splitlines(keepends=True)
    assert open(out, "rb").read() == b"".join(golden_lines[i] for i in keep)


_FRESH_PROCESS = r"""
import sys
import numpy as np
import wfagpu
lib = wfagpu.load()
buf, meta = wfagpu.generate_pairs(64, 300, 0.05, seed=11)
al = wfagpu.DeviceAligner(0)
assert lib.wfagpu_amd_prime(al.ctx) == 0
batch = al.upload(buf, meta)
for cigar in (False, True):
    al.align(batch, (2, 3, 1), max_error=100, compute_cigar=cigar)
    al.align(batch, (4, 6, 2), max_error=200, compute_cigar=cigar, band=25, band_width=64)
print("gap-affine", lib.wfagpu_amd_debug_code_objects())
s, _ = al.align(batch, None, max_error=400, compute_cigar=False, affine2p=(4, 6, 2, 24, 1))
print("two-piece scores", lib.wfagpu_amd_debug_code_objects())
al.align(batch, None, max_error=400, compute_cigar=True, affine2p=(4, 6, 2, 24, 1))
print("two-piece cigars", lib.wfagpu_amd_debug_code_objects())
al.close()
"""


def test_gap_affine_calls_never_load_the_two_piece_code_objects():
    """A fresh process: wfagpu_amd_prime with nothing configured and gap-affine calls (exact and banded, with and without CIGARs) enter
    neither of the two-piece code objects nor the ends-free one (wfagpu_amd_debug_code_objects: every host function that launches,
    queries or primes a kernel of such a unit sets its bit); a score-only two-piece call enters the wavefront unit (bit 1) alone, one
    with CIGARs the backtrace unit (bit 2) too."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _FRESH_PROCESS], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = dict(line.rsplit(" ", 1) for line in r.stdout.splitlines() if line[:3] in ("gap", "two"))
    assert seen == {"gap-affine": "0", "two-piece scores": "2", "two-piece cigars": "6"}, r.stdout


# ---- the sweep: eleven penalty sets and tight budgets (affine2p_ref.SWEEP_PENS) ---------------------------------------------------
SWEEP_PATHS = ["as shipped", "min_tier1", "min_tier2", "min_tier3", "max_error8"]


@pytest.fixture(scope="module")
def sweep():
    return a2.read_golden(a2.SWEEP_SET)


def _factor(pen):
    return math.gcd(*pen)


@pytest.mark.parametrize("cigar", [False, True])
@pytest.mark.parametrize("path", SWEEP_PATHS)
def test_sweep_golden(sweep, cigar, path):
    """Every penalty set of the sweep as one call under a budget of its largest golden score plus 1 (max_error8: of 8) -- as shipped and
    forced through the wider tiers: WFA2's scores and CIGAR bytes."""
    g = sweep
    al = wfagpu.DeviceAligner(0, **({"min_tier": int(path[-1])} if path.startswith("min_tier") else {}))
    try:
        for pen, idx in a2.groups(g).items():
            budget = 8 if path == "max_error8" else int(g["scores"][idx].max()) + 1
            scores, cigars, (st,) = _run_set(al, g, cigar, budget, only=set(idx))
            _check_set(g, scores, cigars, cigar, only=set(idx))
            if path.startswith("min_tier"):
                assert sum(st.pairs_tier[:int(path[-1])]) == 0, pen
            if path == "max_error8":
                assert st.pairs_retried >= sweep_over(g["scores"][idx], 8, _factor(pen)), pen
    finally:
        al.close()


def test_ring_depth_on_either_side_of_the_one_wave_limit(sweep):
    """plan_tier keeps an M ring of more than 64 rows (max(x, o1 + e1, o2 + e2) + 1: affine2p_ref.ring_depth) off the one-wave tier: as
    shipped, under a budget just above its golden scores, a penalty set whose ring has at most 64 rows -- (2,3,1,62,1) -- has pairs
    on tier 0 and one with a deeper ring -- (2,3,1,63,1), (2,3,1,64,1) -- has none, and both give WFA2's bytes."""
    g = sweep
    al = wfagpu.DeviceAligner(0)
    try:
        depths = set()
        for pen, idx in a2.groups(g).items():
            scores, cigars, (st,) = _run_set(al, g, True, int(g["scores"][idx].max()) + 1, only=set(idx))
            _check_set(g, scores, cigars, True, only=set(idx))
            depth = a2.ring_depth(pen)
            depths.add(depth)
            assert (st.pairs_tier[0] > 0) == (depth <= 64), (pen, depth, list(st.pairs_tier))
        assert {64, 65, 66} <= depths
    finally:
        al.close()


def test_score_budget_window_is_exact(sweep):
    """The counterpart of test_gpu_parity.py's test_score_budget_window_is_exact: the pairs of a penalty set that share a golden score run
    under a budget of exactly that score -- the ring of window_width_2p has to hold them: no pair comes back for a wider one -- and
    of one less -- every pair does --, and give WFA2's bytes both times.  (6,9,3,30,3) runs as (2,3,1,10,1) with the budget divided by
    3, rounded down: score and score - 1 still fall on either side."""
    g = sweep
    chosen = sweep_budget_groups(g["pens"], g["scores"], _factor, seed=20261012)
    assert {k for k, _, _ in chosen} == set(a2.SWEEP_PENS) and len(chosen) <= 48
    al = wfagpu.DeviceAligner(0)
    try:
        for pen, score, idx in chosen:
            for budget in (score, score - 1):
                scores, cigars, (st,) = _run_set(al, g, True, budget, only=set(idx))
                _check_set(g, scores, cigars, True, only=set(idx))
                assert st.pairs_retried == (0 if budget == score else len(idx)), (pen, score, budget, len(idx))
    finally:
        al.close()


def test_sweep_behind_the_launch_seam(sweep):
    """wfagpu_amd_configure_affine2p with penalties that have a common factor and with a ring deeper than 64 rows, through
    launch_alignments with a batch size that cuts the call: the golden bytes."""
    g = sweep
    groups = a2.groups(g)
    try:
        for pen in ((6, 9, 3, 30, 3), (2, 3, 1, 64, 1)):
            idx = groups[pen]
            wfagpu.configure_affine2p(pen)
            s, c = _launch([g["pairs"][i] for i in idx], (2, 3, 1), True, int(g["scores"][idx].max()) + 1, 7)
            assert np.array_equal(s, g["scores"][idx]) and c == [g["cigars"][i] for i in idx], pen
    finally:
        wfagpu.configure_affine2p()
