"""Two-piece gap-affine alignment under an ends-free span on the GPU: wfagpu_amd_align_device_2p_span, wfagpu_amd_configure_affine2p_span
behind the launch_alignments* seam and the CLI's --affine2p-ends-free, against WFA2's scores and CIGARs (tests/golden/affine2p_ef.*;
the sets and their writer are in tests/affine2p_endsfree_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import affine2p_endsfree_ref as r2
import affine2p_ref as a2
import endsfree_ref as er
import wfagpu

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(os.path.dirname(wfagpu.LIB_PATH), "bin", "wfa.affine.gpu")
INT32_MIN = -(2**31)
# score budgets of the first tier: above every golden score of the set (asserted in test_golden_sets)
MAX_ERROR = {"small": 800, "small_t50": 800, "wide": 500, "gaps": 300, "ties": 100, "long": 2000}
CHILD_ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), HERE, os.environ.get("PYTHONPATH", "")]))


@pytest.fixture(scope="module")
def sets():
    return {name: r2.read_golden(name) for name in r2.SETS + (r2.ONE_SET, r2.LONG_SET)}


def _run_set(al, g, cigar, max_error, only=None):
    """Every (penalties, span) group of a golden set as one call -> scores, cigars, ends in the set's order, and the calls' stats."""
    n = len(g["pairs"])
    scores, cigars, ends, stats = np.full(n, -12345, dtype=np.int64), [None] * n, np.zeros((n, 2), dtype=np.int64), []
    for (pen, span), idx in r2.groups(g).items():
        idx = [i for i in idx if only is None or i in only]
        if not idx:
            continue
        buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
        s, c, e = al.align(al.upload(buf, meta), None, max_error=max_error, compute_cigar=cigar, affine2p=pen, span=span, fetch_ends=True)
        stats.append(al.stats())
        for j, i in enumerate(idx):
            scores[i], cigars[i], ends[i] = s[j], (c[j] if cigar else None), e[j]
    return scores, cigars, ends, stats


def _check_set(g, scores, cigars, ends, cigar, only=None):
    """score == WFA2's, CIGAR == WFA2's byte for byte, the diagonals consistent with the CIGAR's free runs; no pair is skipped."""
    todo = range(len(g["pairs"])) if only is None else sorted(only)
    for i in todo:
        (p, t), pen, span = g["pairs"][i], g["pens"][i], g["spans"][i]
        where = (i, len(p), len(t), pen, span)
        assert scores[i] == g["scores"][i], where
        _, pe, _, te = er.clamp_span(span, len(p), len(t))
        k0, k1 = int(ends[i][0]), int(ends[i][1])
        assert len(t) - len(p) - te <= k1 <= len(t) - len(p) + pe, where
        if cigar:
            assert cigars[i] == g["cigars"][i], where
            ok, cost = r2.check_cigar2p_span(p, t, cigars[i], pen, span, ends=(k0, k1))
            assert ok and cost == scores[i], where + (k0, k1, cigars[i])
        else:
            assert k0 == INT32_MIN, where      # (the start diagonal is the backtrace's to find)


# ---- 1. goldens, 6. tiers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", r2.SETS + (r2.ONE_SET, r2.LONG_SET))
@pytest.mark.parametrize("cigar", [False, True])
def test_golden_sets(sets, name, cigar):
    g = sets[name]
    assert MAX_ERROR[name] > int(g["scores"].max())
    al = wfagpu.DeviceAligner(0)
    try:
        scores, cigars, ends, stats = _run_set(al, g, cigar, MAX_ERROR[name])
        _check_set(g, scores, cigars, ends, cigar)
        if name == r2.LONG_SET:      # (sequences beyond 32766 bases: the ring of 32-bit offsets in global memory)
            assert sum(st.pairs_tier[3] for st in stats) == len(g["pairs"]) == 1
        if name == "small":          # (the pairs with N / IUPAC bytes run in the byte-compare kernels)
            raw = sum(1 for p, t in g["pairs"] if set(p + t) - set(b"ACGT"))
            assert raw > 0 and sum(st.pairs_raw for st in stats) == raw
    finally:
        al.close()


# ---- 2. every path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["min_tier1", "min_tier2", "min_tier3", "max_error8", "small_arena", "trace_mode1", "trace_mode2",
                                     "trace_mode3", "trace_mode4"])
def test_ties_and_wide_on_every_path(sets, variant):
    """The same batches forced through the wider tiers, through escalation (a budget of 8: every pair of wide misses it), through several
    arena-bound passes (small_t50 in a fixed arena of 1 MiB), and through every mapping of the backtrace: the same bytes."""
    kw, max_error = {}, None
    if variant.startswith("min_tier"):
        kw["min_tier"] = int(variant[-1])
    elif variant.startswith("trace_mode"):
        kw["trace_mode"] = int(variant[-1])
    elif variant == "max_error8":
        max_error = 8
    else:
        kw["arena_bytes"] = 1 << 20
    al = wfagpu.DeviceAligner(0, **kw)
    try:
        passes = retried = 0
        for name in ("ties", "wide") + ((r2.ONE_SET,) if variant == "small_arena" else ()):
            g = sets[name]
            scores, cigars, ends, stats = _run_set(al, g, True, max_error or MAX_ERROR[name])
            _check_set(g, scores, cigars, ends, True)
            passes = max(passes, max(st.sub_batches for st in stats))
            retried += sum(st.pairs_retried for st in stats)
            if variant.startswith("min_tier"):
                assert all(sum(st.pairs_tier[:int(variant[-1])]) == 0 for st in stats)
        assert variant != "max_error8" or retried >= len(sets["wide"]["pairs"])
        assert variant != "small_arena" or passes > 1
    finally:
        al.close()


# ---- 3. a span of zeros, 4. equal pieces --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", a2.ONE_PEN_SET])
def test_a_span_of_zeros_gives_the_end_to_end_bytes(name):
    """affine2p=pen, span=(0,0,0,0) on affine2p_ref's sets: tests/golden/affine2p.<set>.alg byte for byte (through the ends-free kernels:
    a start row of one cell, one end diagonal, today's two-piece window), ends = (0, tlen - plen)."""
    g = a2.read_golden(name)
    al = wfagpu.DeviceAligner(0)
    try:
        for pen, idx in a2.groups(g).items():
            buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
            batch = al.upload(buf, meta)
            kend = meta["text_len"].astype(np.int64) - meta["pattern_len"].astype(np.int64)
            s, c, e = al.align(batch, None, max_error=1000, compute_cigar=True, affine2p=pen, span=(0, 0, 0, 0), fetch_ends=True)
            assert np.array_equal(s, g["scores"][idx]) and c == [g["cigars"][i] for i in idx], pen
            assert not e[:, 0].any() and np.array_equal(e[:, 1], kend), pen
            s, _, e = al.align(batch, None, max_error=1000, compute_cigar=False, affine2p=pen, span=(0, 0, 0, 0), fetch_ends=True)
            assert np.array_equal(s, g["scores"][idx]) and np.array_equal(e[:, 1], kend) and (e[:, 0] == INT32_MIN).all(), pen
    finally:
        al.close()


def test_equal_pieces_score_like_gap_affine_under_the_span(sets):
    """(3,8,2,8,2) under (0,0,50,50) on the pairs of small: the scores of gap-affine (3,8,2) under that span on the existing kernels."""
    buf, meta = wfagpu.layout_pairs(sets["small"]["pairs"])
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        s1, _ = al.align(batch, (3, 8, 2), max_error=1000, compute_cigar=False, span=(0, 0, 50, 50))
        s2, _ = al.align(batch, None, max_error=1000, compute_cigar=False, affine2p=(3, 8, 2, 8, 2), span=(0, 0, 50, 50))
        assert len(s2) == 200 and np.array_equal(s1, s2)
    finally:
        al.close()


# ---- 5. the window is exact ---------------------------------------------------------------------------------------------------------
def test_score_budget_window_is_exact(sets):
    """Pairs that share (penalties, span, golden score) under a budget of exactly that score -- the narrowest window and the tightest
    feasibility test that have to let them through: WFA2's bytes and no pair comes back -- and of one less: every pair comes back.  A
    window one diagonal too narrow or a bisection off by one fails the first; a budget stop one score late fails the second."""
    chosen = r2.budget_groups()
    assert 24 <= len(chosen) <= 32 and set(r2.GAPS_PENS) <= {k[0] for k, _, _, _ in chosen}
    al = wfagpu.DeviceAligner(0)
    try:
        for key, score, name, idx in chosen:
            for budget in (score, score - 1):
                scores, cigars, ends, (st,) = _run_set(al, sets[name], True, budget, only=set(idx))
                _check_set(sets[name], scores, cigars, ends, True, only=set(idx))
                assert st.pairs_retried == (0 if budget == score else len(idx)), (key, score, budget, len(idx), st.pairs_retried)
    finally:
        al.close()


# ---- 7. seam and CLI ------------------------------------------------------------------------------------------------------------------
_SEAM_CHILD = r"""
import ctypes as C
import numpy as np
import affine2p_endsfree_ref as r2
import wfagpu
lib = wfagpu.load()
g = r2.read_golden(r2.ONE_SET)
buf, meta = wfagpu.layout_pairs(g["pairs"])
n = len(g["pairs"])
def launch(cigar, batch_size):
    res = C.POINTER(wfagpu.AlignmentResult)()
    assert lib.initialize_wfa_results(C.byref(res), n, 256 if cigar else 1)
    opt = wfagpu.Options(max_error=1000, threads_per_block=0, num_workers=1, band=-1, batch_size=batch_size, num_alignments=n,
                         penalties=wfagpu.Penalties(2, 3, 1), compute_cigar=cigar)
    (lib.launch_alignments if cigar else lib.launch_alignments_distance)(buf.ctypes.data, buf.nbytes, meta.ctypes.data, res, opt, False)
    scores = np.array([res[i].error for i in range(n)], dtype=np.int64)
    cigars = [C.string_at(res[i].cigar.buffer).decode() for i in range(n)] if cigar else None
    lib.destroy_wfa_results(res, n)
    return scores, cigars
try:
    wfagpu.configure_launch(virtual_devices=2)
    wfagpu.configure_affine2p(r2.ONE_PEN, span=r2.ONE_SPAN)
    s, c = launch(True, 37)
    assert np.array_equal(s, g["scores"]) and c == g["cigars"]
    s, _ = launch(False, 37)
    assert np.array_equal(s, g["scores"])
    print("seam pairs", len(s))
finally:
    wfagpu.configure_affine2p()
"""


def test_two_pieces_configured_with_a_span_behind_the_launch_seam():
    r = subprocess.run([sys.executable, "-c", _SEAM_CHILD], capture_output=True, text=True, timeout=300, env=CHILD_ENV)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "seam pairs 200" in r.stdout


def test_cli_affine2p_ends_free(sets, tmp_path):
    """--affine2p 4,6,2,24,1 --affine2p-ends-free 0,0,50,50 with -x -c -o on the non-empty pairs (a .seq file carries no empty
    sequence): the golden lines, and the -c verification finds nothing wrong."""
    g = sets[r2.ONE_SET]
    keep = [i for i, (p, t) in enumerate(g["pairs"]) if p and t]
    seq, out = tmp_path / "nonempty.seq", tmp_path / "res.out"
    with open(seq, "wb") as f:
        for i in keep:
            f.write(b">" + g["pairs"][i][0] + b"\n<" + g["pairs"][i][1] + b"\n")
    r = subprocess.run([CLI, "-i", str(seq), "--affine2p", "4,6,2,24,1", "--affine2p-ends-free", "0,0,50,50", "-e", "800", "-x", "-c",
                        "-b", "150", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Incorrect=0" in r.stderr and all(tok == "Incorrect=0" for tok in r.stderr.split() if tok.startswith("Incorrect="))
    assert open(out).read().splitlines() == [f"{-int(g['scores'][i])}\t{g['cigars'][i]}" for i in keep]


# ---- 8. code objects ------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
import wfagpu
lib = wfagpu.load()
buf, meta = wfagpu.generate_pairs(64, 300, 0.05, seed=11)
al = wfagpu.DeviceAligner(0)
batch = al.upload(buf, meta)
if sys.argv[1] == "others":
    assert lib.wfagpu_amd_prime(al.ctx) == 0
    for cigar in (False, True):
        al.align(batch, (2, 3, 1), max_error=100, compute_cigar=cigar)
        al.align(batch, (2, 3, 1), max_error=100, compute_cigar=cigar, span=(0, 0, 20, 20))
        al.align(batch, None, max_error=200, compute_cigar=cigar, affine2p=(4, 6, 2, 24, 1))
        al.align(batch, None, max_error=100, compute_cigar=cigar, linear=("edit",))
else:
    al.align(batch, None, max_error=200, compute_cigar=True, affine2p=(4, 6, 2, 24, 1), span=(0, 0, 20, 20))
bits = lib.wfagpu_amd_debug_code_objects()
print(sys.argv[1], bits & 1024, bits & 4, bits & 3)
al.close()
"""


@pytest.mark.parametrize("which,want", [("others", "others 0 4 3"), ("combined", "combined 1024 4 0")])
def test_only_the_combined_call_loads_its_code_object(which, want):
    """wfagpu_amd_debug_code_objects: a process of prime, gap-affine, span, end-to-end two-piece and metric calls never enters the new unit
    (bit 1024); a process of one combined call with CIGARs enters it and the two-piece backtrace (bit 4), not the gap-affine ends-free
    (bit 1) or the end-to-end two-piece (bit 2) kernels."""
    r = subprocess.run([sys.executable, "-c", _CHILD, which], capture_output=True, text=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr[-2000:]
    assert want in r.stdout, r.stdout
