"""Edit, indel and gap-linear distances under an ends-free span on the GPU: wfagpu_amd_align_device_linear_span,
wfagpu_amd_configure_linear_span behind the launch_alignments* seam and the CLI's --metric-ends-free, against WFA2's scores and CIGARs
(tests/golden/linef.*, made by tests/golden/make_golden_linear_endsfree.py; the sets are described in tests/linear_endsfree_ref.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import endsfree_ref as er
import linear_endsfree_ref as ler
import linear_ref as lr
import wfagpu

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(wfagpu.LIB_PATH)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")
INT32_MIN = -(2**31)
# score budgets of the first tier, above the set's largest golden score (small: 780, small_edit_t50: 296, wide: 224, ties: 2, long: 480)
MAX_ERROR = {"small": 1000, "small_edit_t50": 400, "wide": 400, "ties": 100, "long": 1000}
CHILD_ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), HERE, os.environ.get("PYTHONPATH", "")]))


@pytest.fixture(scope="module")
def sets():
    return {name: ler.read_golden(name) for name in ler.SETS + (ler.LONG_SET,)}


@pytest.fixture(scope="module")
def sweep():
    return ler.read_golden(ler.SWEEP_SET)


def test_the_budgets_lie_above_the_golden_scores(sets):
    assert {n: int(sets[n]["scores"].max()) for n in MAX_ERROR} == {"small": 780, "small_edit_t50": 296, "wide": 224, "ties": 2, "long": 480}
    assert all(MAX_ERROR[n] > int(sets[n]["scores"].max()) for n in MAX_ERROR)


def _run_set(al, g, cigar, max_error, only=None):
    """Every (metric, span) group of a golden set as one call -> scores, cigars, ends in the set's order (only: a subset of indices).
    No pair is skipped: every index must have come back."""
    n = len(g["pairs"])
    scores = np.full(n, -12345, dtype=np.int64)
    cigars = [None] * n
    ends = np.zeros((n, 2), dtype=np.int64)
    seen = 0
    stats = []
    for (metric, span), idx in ler.groups(g).items():
        if only is not None:
            idx = [i for i in idx if i in only]
            if not idx:
                continue
        buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
        batch = al.upload(buf, meta)
        s, c, e = al.align(batch, None, max_error=max_error, compute_cigar=cigar, linear=metric, span=span, fetch_ends=True)
        stats.append(al.stats())
        for j, i in enumerate(idx):
            scores[i] = s[j]
            cigars[i] = c[j] if cigar else None
            ends[i] = e[j]
        seen += len(idx)
    assert seen == (n if only is None else len(only))
    return scores, cigars, ends, stats


def _check_set(g, scores, cigars, ends, cigar, only=None):
    checked = 0
    for i in (range(len(g["pairs"])) if only is None else sorted(only)):
        p, t = g["pairs"][i]
        metric, span = g["metrics"][i], g["spans"][i]
        where = (i, len(p), len(t), metric, span)
        assert scores[i] == g["scores"][i], where
        pb, pe, tb, te = er.clamp_span(span, len(p), len(t))
        kend = len(t) - len(p)
        k0, k1 = int(ends[i][0]), int(ends[i][1])
        assert kend - te <= k1 <= kend + pe, where
        if cigar:
            assert cigars[i] == g["cigars"][i], where
            ok, cost = ler.check_cigar_linear_span(p, t, cigars[i], metric, span, ends=(k0, k1))
            assert ok and cost == scores[i], where + (k0, k1, cigars[i])
        else:
            assert k0 == INT32_MIN, where      # (the start diagonal is the backtrace's to find)
        checked += 1
    assert checked == (len(g["pairs"]) if only is None else len(only))


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ler.SETS)
@pytest.mark.parametrize("cigar", [False, True])
def test_golden_sets(sets, name, cigar):
    """score == WFA2's, CIGAR == WFA2's byte for byte, the diagonals consistent with the CIGAR's free runs."""
    g = sets[name]
    al = wfagpu.DeviceAligner(0)
    try:
        scores, cigars, ends, _ = _run_set(al, g, cigar, MAX_ERROR[name])
        _check_set(g, scores, cigars, ends, cigar)
    finally:
        al.close()


# ---- 2. every path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["min_tier1", "min_tier2", "min_tier3", "max_error8", "small_arena", "trace_mode1", "trace_mode2",
                                     "trace_mode3", "trace_mode4"])
def test_ties_and_wide_on_every_path(sets, variant):
    """The same batches forced through the wider tiers, through escalation (a budget of 8: every pair of wide misses it), through
    several arena-bound passes (small_edit_t50 too: 400 pairs in one call), and through every mapping of the backtrace: the same bytes."""
    kw, max_error = {}, None
    if variant.startswith("min_tier"):
        kw["min_tier"] = int(variant[-1])
    elif variant.startswith("trace_mode"):
        kw["trace_mode"] = int(variant[-1])
    elif variant == "max_error8":
        max_error = 8
    elif variant == "small_arena":
        kw["arena_bytes"] = 1 << 20      # (a fixed arena of 1 MiB: small_edit_t50 does not fit it at once)
    al = wfagpu.DeviceAligner(0, **kw)
    try:
        passes = retried = 0
        for name in ("ties", "wide") + (("small_edit_t50",) if variant == "small_arena" else ()):
            g = sets[name]
            scores, cigars, ends, stats = _run_set(al, g, True, max_error or MAX_ERROR[name])
            _check_set(g, scores, cigars, ends, True)
            passes = max(passes, max(st.sub_batches for st in stats))
            retried += sum(st.pairs_retried for st in stats)
            if variant.startswith("min_tier"):
                t = int(variant[-1])
                assert all(sum(st.pairs_tier[:t]) == 0 for st in stats)
        if variant == "max_error8":
            assert retried >= len(sets["wide"]["pairs"])
        if variant == "small_arena":
            assert passes > 1
    finally:
        al.close()


def test_one_wave_tier_and_byte_compare_class(sets):
    """ties runs entirely on the one-wave tier; the pairs of small with N / IUPAC bytes run in the byte-compare kernels."""
    al = wfagpu.DeviceAligner(0)
    try:
        g = sets["ties"]
        scores, cigars, ends, stats = _run_set(al, g, True, MAX_ERROR["ties"])
        _check_set(g, scores, cigars, ends, True)
        assert sum(st.pairs_tier[0] for st in stats) == len(g["pairs"])
        g = sets["small"]
        only = {i for i, (p, t) in enumerate(g["pairs"]) if set(p + t) - set(b"ACGT")}
        assert len(only) == 13
        for cigar in (False, True):
            scores, cigars, ends, stats = _run_set(al, g, cigar, MAX_ERROR["small"], only=only)
            _check_set(g, scores, cigars, ends, cigar, only=only)
            assert sum(st.pairs_raw for st in stats) == len(only)
    finally:
        al.close()


# ---- 3. ring depth, 4. the window is exact (the sweep) ---------------------------------------------------------------------------------
def _factor(key):
    return math.gcd(*lr.pens_of(key[0]))


def test_ring_depth_on_either_side_of_the_one_wave_limit(sweep):
    """plan_tier keeps an M ring of more than 64 rows off the one-wave tier: under budgets just above the golden scores a metric whose
    ring has at most 64 rows -- (63,1), (1,63) -- has pairs on tier 0 and no call of one with a deeper ring -- (64,1), (1,64) -- has any;
    both give WFA2's bytes.  Counted per metric over its five spans, as for the gap-affine span: the all-free span of a 700-base pair
    is every diagonal there is, which no one-wave ring holds."""
    g = sweep
    al = wfagpu.DeviceAligner(0)
    try:
        tier0, depths, seen = {}, {}, set()
        for (metric, span), idx in ler.groups(g).items():
            scores, cigars, ends, (st,) = _run_set(al, g, True, int(g["scores"][idx].max()) + 1, only=set(idx))
            _check_set(g, scores, cigars, ends, True, only=set(idx))
            seen |= set(idx)
            depths[metric] = lr.ring_depth(metric)
            tier0[metric] = tier0.get(metric, 0) + st.pairs_tier[0]
            assert depths[metric] <= 64 or st.pairs_tier[0] == 0, (metric, span, list(st.pairs_tier))
        assert len(seen) == len(g["pairs"]) == 310
        assert set(tier0) == set(lr.SWEEP_METRICS) and {64, 65} <= set(depths.values())
        for metric in lr.SWEEP_METRICS:
            assert (tier0[metric] > 0) == (depths[metric] <= 64), (metric, depths[metric], tier0[metric])
    finally:
        al.close()


def test_score_budget_window_is_exact(sweep):
    """The pairs of a (metric, span) group that share a golden score run under a budget of exactly that score -- the narrowest window and
    the tightest feasibility test that have to let them through: WFA2's bytes, and no pair comes back for a wider ring (plan_tier's
    bound, S / g + 1 diagonals plus the free bases, holds every pair's own window: hull or quotient, both are below it) -- and of one less:
    every pair is "not within the budget" and comes back.  A window one diagonal too narrow or a feasibility test off by one fails the
    first; a budget stop that is one score late fails the second.  (6,3) and (9,9) run as (2,1) and (1,1) with the budget divided by 3
    and 9, rounded down: score and score - 1 still fall on either side.  The all-free span scores 0 everywhere: no budget to run under."""
    g = sweep
    chosen = er.sweep_budget_groups(list(zip(map(tuple, g["metrics"]), map(tuple, g["spans"]))), g["scores"], _factor, seed=20261021, limit=64)
    assert {k[0] for k, _, _ in chosen} == set(lr.SWEEP_METRICS) and {k[1] for k, _, _ in chosen} == set(er.SWEEP_SPANS[:4])
    assert 48 <= len(chosen) <= 64
    al = wfagpu.DeviceAligner(0)
    try:
        ran = 0
        for key, score, idx in chosen:
            for budget in (score, score - 1):
                scores, cigars, ends, (st,) = _run_set(al, g, True, budget, only=set(idx))
                _check_set(g, scores, cigars, ends, True, only=set(idx))
                assert st.pairs_retried == (0 if budget == score else len(idx)), (key, score, budget, len(idx), st.pairs_retried)
            ran += len(idx)
        assert ran == sum(len(idx) for _, _, idx in chosen)
    finally:
        al.close()


# ---- 5. zero span, 6. the emulation, 7. the 32-bit tier ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", "lanes"])
def test_a_span_of_zeros_gives_the_end_to_end_bytes(name):
    """linear=m, span=(0,0,0,0) on linear_ref's sets: tests/golden/linear.<set>.alg byte for byte (through the ends-free kernels: a
    start row of one cell, one end diagonal), ends = (0, tlen - plen)."""
    g = lr.read_golden(name)
    al = wfagpu.DeviceAligner(0)
    try:
        seen = 0
        for metric, idx in lr.groups(g).items():
            buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
            batch = al.upload(buf, meta)
            kend = meta["text_len"].astype(np.int64) - meta["pattern_len"].astype(np.int64)
            budget = {"ties": 100, "lanes": 700}[name]      # (test_gpu_linear.py's: above the largest golden scores, 12 and 464)
            s, c, e = al.align(batch, None, max_error=budget, compute_cigar=True, linear=metric, span=(0, 0, 0, 0), fetch_ends=True)
            assert np.array_equal(s, g["scores"][idx]) and c == [g["cigars"][i] for i in idx], metric
            assert np.array_equal(e[:, 0], np.zeros(len(idx))) and np.array_equal(e[:, 1], kend), metric
            s, _, e = al.align(batch, None, max_error=budget, compute_cigar=False, linear=metric, span=(0, 0, 0, 0), fetch_ends=True)
            assert np.array_equal(s, g["scores"][idx]) and np.array_equal(e[:, 1], kend) and (e[:, 0] == INT32_MIN).all(), metric
            seen += len(idx)
        assert seen == len(g["pairs"])
    finally:
        al.close()


def test_edit_against_the_emulation_on_the_gap_affine_ends_free_kernels(sets):
    """small_edit_t50: the scores of gap-affine (1, 0, 1) under the same span on the existing ends-free kernels; the CIGAR bytes where
    WFA2 agrees with itself there (linear_endsfree_ref.SMALL_EDIT_T50_CIGARS_AGREE, found on the CPU)."""
    g = sets["small_edit_t50"]
    buf, meta = wfagpu.layout_pairs(g["pairs"])
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        s0, c0 = al.align(batch, ler.EMULATION_PEN, max_error=MAX_ERROR["small_edit_t50"], compute_cigar=True, span=ler.ONE_SPAN)
        s1, c1 = al.align(batch, None, max_error=MAX_ERROR["small_edit_t50"], compute_cigar=True, linear=lr.EDIT, span=ler.ONE_SPAN)
        assert len(s1) == len(g["pairs"]) == 400
        assert np.array_equal(s1, s0) and np.array_equal(s1, g["scores"])
        if ler.SMALL_EDIT_T50_CIGARS_AGREE:
            assert c1 == c0
    finally:
        al.close()


def test_sequences_beyond_16_bit_offsets(sets):
    """33.5 kbp patterns inside their windows: the tier whose ring holds 32-bit offsets in global memory."""
    g = sets[ler.LONG_SET]
    al = wfagpu.DeviceAligner(0)
    try:
        for cigar in (False, True):
            scores, cigars, ends, stats = _run_set(al, g, cigar, MAX_ERROR["long"])
            _check_set(g, scores, cigars, ends, cigar)
            assert sum(st.pairs_tier[3] for st in stats) == len(g["pairs"]) == 2
    finally:
        al.close()


# ---- 8. seam and CLI ------------------------------------------------------------------------------------------------------------------
_SEAM_CHILD = r"""
import ctypes as C
import numpy as np
import linear_endsfree_ref as ler
import linear_ref as lr
import wfagpu
lib = wfagpu.load()
g = ler.read_golden("small_edit_t50")
pairs = g["pairs"]
buf, meta = wfagpu.layout_pairs(pairs)
n = len(pairs)
def launch(cigar, batch_size):
    res = C.POINTER(wfagpu.AlignmentResult)()
    assert lib.initialize_wfa_results(C.byref(res), n, 256 if cigar else 1)
    opt = wfagpu.Options(max_error=400, threads_per_block=0, num_workers=1, band=-1, batch_size=batch_size, num_alignments=n,
                         penalties=wfagpu.Penalties(2, 3, 1), compute_cigar=cigar)
    (lib.launch_alignments if cigar else lib.launch_alignments_distance)(buf.ctypes.data, buf.nbytes, meta.ctypes.data, res, opt, False)
    scores = np.array([res[i].error for i in range(n)], dtype=np.int64)
    cigars = [C.string_at(res[i].cigar.buffer).decode() for i in range(n)] if cigar else None
    lib.destroy_wfa_results(res, n)
    return scores, cigars
try:
    wfagpu.configure_launch(virtual_devices=2)
    wfagpu.configure_linear(lr.EDIT, span=ler.ONE_SPAN)
    s, c = launch(True, 37)
    assert np.array_equal(s, g["scores"]) and c == g["cigars"]
    s, _ = launch(False, 37)
    assert np.array_equal(s, g["scores"])
    print("seam pairs", len(s))
finally:
    wfagpu.configure_linear()
"""


def test_a_metric_configured_with_a_span_behind_the_launch_seam():
    """wfagpu_amd_configure_linear_span(edit, (0,0,50,50)): launch_alignments and launch_alignments_distance on two device slots with
    a batch size that cuts the call give small_edit_t50 -- in a child process, the configuration cleared in its finally."""
    r = subprocess.run([sys.executable, "-c", _SEAM_CHILD], capture_output=True, text=True, timeout=300, env=CHILD_ENV)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "seam pairs 400" in r.stdout


def test_cli_metric_ends_free(sets, tmp_path):
    """--edit --metric-ends-free 0,0,50,50 with -x -c -o: the golden lines, exit code 0, and the -c verification (the CIGAR priced under
    the metric without its free runs, the score against the one-table program with free borders) finds nothing wrong.  (A .seq file
    carries no empty sequence: the two pairs that have one are left out.)"""
    g = sets["small_edit_t50"]
    seq = tmp_path / "nonempty.seq"
    keep = [i for i, (p, t) in enumerate(g["pairs"]) if p and t]
    assert len(keep) == len(g["pairs"]) - 2
    with open(seq, "wb") as f:
        for i in keep:
            f.write(b">" + g["pairs"][i][0] + b"\n<" + g["pairs"][i][1] + b"\n")
    out = tmp_path / "res.out"
    r = subprocess.run([CLI, "-i", str(seq), "--edit", "--metric-ends-free", ",".join(str(v) for v in ler.ONE_SPAN), "-e", "400", "-x", "-c",
                        "-b", "150", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Incorrect=0" in r.stderr and all(tok == "Incorrect=0" for tok in r.stderr.split() if tok.startswith("Incorrect="))
    got = open(out).read().splitlines()
    assert got == [f"{-int(g['scores'][i])}\t{g['cigars'][i]}" for i in keep]


# ---- 9. code objects ------------------------------------------------------------------------------------------------------------------
_OTHERS_CHILD = r"""
import wfagpu
lib = wfagpu.load()
buf, meta = wfagpu.generate_pairs(64, 300, 0.05, seed=11)
al = wfagpu.DeviceAligner(0)
assert lib.wfagpu_amd_prime(al.ctx) == 0
batch = al.upload(buf, meta)
for cigar in (False, True):
    al.align(batch, (2, 3, 1), max_error=100, compute_cigar=cigar)
    al.align(batch, (2, 3, 1), max_error=100, compute_cigar=cigar, span=(0, 0, 20, 20))
    al.align(batch, None, max_error=100, compute_cigar=cigar, linear=("edit",))
    al.align(batch, None, max_error=200, compute_cigar=cigar, linear=("linear", 4, 2))
print("others", lib.wfagpu_amd_debug_code_objects() & 64, lib.wfagpu_amd_debug_code_objects() & 17)
al.close()
"""

_COMBINED_CHILD = r"""
import wfagpu
lib = wfagpu.load()
buf, meta = wfagpu.generate_pairs(64, 300, 0.05, seed=11)
al = wfagpu.DeviceAligner(0)
batch = al.upload(buf, meta)
al.align(batch, None, max_error=100, compute_cigar=True, linear=("edit",), span=(0, 0, 20, 20))
print("combined", lib.wfagpu_amd_debug_code_objects() & 64, lib.wfagpu_amd_debug_code_objects() & 1)
al.close()
"""


def test_only_the_combined_call_loads_its_code_object():
    """wfagpu_amd_debug_code_objects: a process of gap-affine, span and end-to-end metric calls never enters the new unit (bit 6) --
    it does enter the ends-free (bit 0) and one-component (bit 4) ones --; a process of one combined call enters bit 6 and not the
    gap-affine ends-free kernels (bit 0)."""
    r = subprocess.run([sys.executable, "-c", _OTHERS_CHILD], capture_output=True, text=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "others 0 17" in r.stdout, r.stdout
    r = subprocess.run([sys.executable, "-c", _COMBINED_CHILD], capture_output=True, text=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "combined 64 0" in r.stdout, r.stdout
