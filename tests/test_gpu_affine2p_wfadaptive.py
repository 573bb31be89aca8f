"""The wf-adaptive heuristic under two-piece penalties on the GPU: wfagpu_amd_align_device_2p_adaptive,
wfagpu_amd_configure_affine2p_wfadaptive behind the launch_alignments* seam and the CLI, against WFA2's scores and CIGARs under the same
penalties and heuristic (tests/golden/affine2p_ad.*; the sets are described in tests/affine2p_wfadaptive_ref.py), byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import affine2p_ref as a2
import affine2p_wfadaptive_ref as ar
import wfagpu
from test_gpu_affine2p import _launch

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(wfagpu.LIB_PATH), "bin", "wfa.affine.gpu")
UNIT_2PAD = 2048
# score budgets of the first tier: above every golden score of the set (small: 738, indel: 546, long: 4530)
MAX_ERROR = {"small": 800, "indel": 700, "long": 4800}


@pytest.fixture(scope="module")
def sets():
    return {name: ar.read_golden(name) for name in ar.SETS}


def _run_set(al, g, cigar, max_error):
    """Every (heuristic, penalties) group of a golden set as one call -> scores, cigars in the set's order, and the calls' stats."""
    n = len(g["pairs"])
    scores, cigars, stats = np.full(n, -12345, dtype=np.int64), [None] * n, []
    for (h, pen), idx in ar.groups(g).items():
        buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
        s, c = al.align(al.upload(buf, meta), None, max_error=max_error, compute_cigar=cigar, affine2p=pen, wfadaptive=h)
        stats.append(al.stats())
        for j, i in enumerate(idx):
            scores[i], cigars[i] = s[j], (c[j] if cigar else None)
    return scores, cigars, stats


def _check_set(g, scores, cigars, cigar):
    for i, (p, t) in enumerate(g["pairs"]):
        where = (i, len(p), len(t), g["pens"][i], g["heurs"][i])
        assert scores[i] == g["scores"][i], where
        if cigar:
            assert cigars[i] == g["cigars"][i], where


@pytest.mark.parametrize("name", ar.SETS)
@pytest.mark.parametrize("cigar", [False, True])
def test_golden_sets(sets, name, cigar):
    g = sets[name]
    al = wfagpu.DeviceAligner(0)
    try:
        scores, cigars, stats = _run_set(al, g, cigar, MAX_ERROR[name])
        _check_set(g, scores, cigars, cigar)
        if name == "long":
            assert sum(st.pairs_tier[3] for st in stats) == len(g["pairs"])
        assert all(st.pairs_tier[4] == 0 and st.pairs_tier[5] == 0 and st.pairs_banded == 0 and st.auto_budget == 0 for st in stats)
        assert wfagpu.load().wfagpu_amd_debug_code_objects() & UNIT_2PAD
    finally:
        al.close()


@pytest.mark.parametrize("variant", ["min_tier1", "min_tier2", "min_tier3", "max_error8", "small_arena"])
def test_small_and_indel_on_every_path(sets, variant):
    """Forced through the multi-wave tiers (the ten-limit reduction) and the ring in global memory, through escalation (a budget of 8:
    every pair that differs misses it) and through several arena-bound passes: the same bytes."""
    kw = {"min_tier": int(variant[-1])} if variant.startswith("min_tier") else {"arena_bytes": 4 << 20} if variant == "small_arena" else {}
    al = wfagpu.DeviceAligner(0, **kw)
    try:
        passes = retried = 0
        for name in ("small", "indel"):
            g = sets[name]
            scores, cigars, stats = _run_set(al, g, True, 8 if variant == "max_error8" else MAX_ERROR[name])
            _check_set(g, scores, cigars, True)
            passes = max(passes, max(st.sub_batches for st in stats))
            retried += sum(st.pairs_retried for st in stats)
            if variant.startswith("min_tier"):
                assert all(sum(st.pairs_tier[:int(variant[-1])]) == 0 for st in stats)
        if variant == "max_error8":
            assert retried >= int((sets["small"]["scores"] > 8).sum()) + 32
        if variant == "small_arena":
            assert passes > 1
    finally:
        al.close()


@pytest.mark.parametrize("heur", [(10, 1 << 20, 1), (1 << 20, 50, 1)], ids=["threshold", "min_length"])
@pytest.mark.parametrize("name", ["small", "gaps"])
def test_a_heuristic_that_never_cuts_gives_the_exact_two_piece_goldens(name, heur):
    """The existing exact goldens through the new kernels.  One pair is not exact under WFA2 itself: pair 18 of `small`, 41 bases against
    an empty text.  Its only M cell is the one of score 0, so every later cut-off call returns before it equates, but the trimmed limits
    of the gap components still rule: WFA2 reports 75 with the CIGAR 41D (the exact search: 65) under both heuristics, and so must we."""
    g = a2.read_golden(name)
    if name == "small":
        assert g["pairs"][18][1] == b"" and g["scores"][18] == 65 and g["cigars"][18] == "41D"
        g["scores"][18] = 75
    al = wfagpu.DeviceAligner(0)
    try:
        for pen, idx in a2.groups(g).items():
            buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
            s, c = al.align(al.upload(buf, meta), None, max_error=int(g["scores"][idx].max()) + 1, compute_cigar=True, affine2p=pen, wfadaptive=heur)
            assert np.array_equal(s, g["scores"][idx]) and list(c) == [g["cigars"][i] for i in idx], pen
    finally:
        al.close()


def test_the_heuristic_computes_fewer_cells_than_the_exact_two_piece_search(sets):
    buf, meta = wfagpu.layout_pairs(sets["long"]["pairs"])
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        al.align(batch, None, max_error=4800, compute_cigar=False, affine2p=ar.DEFAULT_PEN)
        exact_cells = al.stats().cells
        al.align(batch, None, max_error=4800, compute_cigar=False, affine2p=ar.DEFAULT_PEN, wfadaptive=(10, 50, 1))
        assert 0 < al.stats().cells < exact_cells
    finally:
        al.close()


def test_configured_pair_behind_the_launch_seam_and_wfagpu_align(sets):
    """indel (one heuristic; its pairs under the default penalties are the group taken) behind launch_alignments* with a batch size that
    cuts the call and a band that is not used, and behind wfagpu_align; after un-configuring, the exact two-piece answers."""
    g = sets["indel"]
    idx = ar.groups(g)[((4, 5, 3), ar.DEFAULT_PEN)]
    pairs = [g["pairs"][i] for i in idx]
    try:
        wfagpu.configure_affine2p(ar.DEFAULT_PEN, wfadaptive=(4, 5, 3))
        for kw in ({}, {"band": 25, "band_width": 64}):
            s, c = _launch(pairs, (2, 3, 1), True, 700, 3, **kw)
            assert np.array_equal(s, g["scores"][idx]) and c == [g["cigars"][i] for i in idx]
        s, _ = _launch(pairs, (2, 3, 1), False, 700, 3)
        assert np.array_equal(s, g["scores"][idx])
        lib = wfagpu.load()
        ali = wfagpu.Aligner()
        assert lib.wfagpu_initialize_aligner(C.byref(ali))
        for p, t in pairs:
            assert lib.wfagpu_add_sequences(C.byref(ali), p, t)
        assert lib.wfagpu_initialize_parameters(C.byref(ali), wfagpu.Penalties(2, 3, 1)) and lib.wfagpu_align(C.byref(ali))
        assert [ali.results[i].error for i in range(len(pairs))] == [int(g["scores"][i]) for i in idx]
        lib.wfagpu_destroy_aligner(C.byref(ali))
        wfagpu.configure_affine2p()
        wfagpu.configure_affine2p(ar.DEFAULT_PEN)
        s, c = _launch(pairs, (2, 3, 1), True, 700, 3)
        assert [int(v) for v in s] == [a2.dp_affine2p_score(p, t, ar.DEFAULT_PEN) for p, t in pairs]
        assert all(a2.check_cigar2p(p, t, cg, ar.DEFAULT_PEN) == (True, int(sc)) for (p, t), cg, sc in zip(pairs, c, s))
    finally:
        wfagpu.configure_affine2p()


def test_configure_is_mutually_exclusive():
    lib = wfagpu.load()
    pen, heur = wfagpu.Penalties2p(*ar.DEFAULT_PEN), wfagpu.WfAdaptive(10, 50, 1)
    cfg = lib.wfagpu_amd_configure_affine2p_wfadaptive
    try:
        assert cfg(C.byref(pen), C.byref(wfagpu.WfAdaptive(0, 50, 1))) == -1 and cfg(C.byref(wfagpu.Penalties2p(4, 6, 0, 24, 1)), C.byref(heur)) == -1
        assert cfg(C.byref(pen), C.byref(heur)) == 0
        assert lib.wfagpu_amd_configure_span(C.byref(wfagpu.Span(0, 0, 5, 5))) == -1 and lib.wfagpu_amd_configure_affine2p(C.byref(pen)) == -1
        assert lib.wfagpu_amd_configure_wfadaptive(C.byref(heur)) == -1
        assert cfg(None, None) == 0
        for other, arg in ((lib.wfagpu_amd_configure_span, wfagpu.Span(0, 0, 5, 5)), (lib.wfagpu_amd_configure_affine2p, pen), (lib.wfagpu_amd_configure_wfadaptive, heur)):
            assert other(C.byref(arg)) == 0 and cfg(C.byref(pen), C.byref(heur)) == -1 and other(None) == 0
    finally:
        cfg(None, None)


_FRESH_PROCESS = r"""
import sys, wfagpu
lib = wfagpu.load()
if sys.argv[1] == "prime":
    wfagpu.configure_affine2p((4, 6, 2, 24, 1), wfadaptive=(10, 50, 1))
al = wfagpu.DeviceAligner(0)
assert lib.wfagpu_amd_prime(al.ctx) == 0
print("prime", lib.wfagpu_amd_debug_code_objects())
batch = al.upload(*wfagpu.generate_pairs(64, 300, 0.05, seed=11))
for cigar in (False, True):
    al.align(batch, (2, 3, 1), max_error=100, compute_cigar=cigar)
    al.align(batch, (2, 3, 1), max_error=100, compute_cigar=cigar, span=(0, 0, 5, 5))
    al.align(batch, None, max_error=400, compute_cigar=cigar, affine2p=(4, 6, 2, 24, 1))
    al.align(batch, (2, 3, 1), max_error=100, compute_cigar=cigar, wfadaptive=(10, 50, 1))
print("others", lib.wfagpu_amd_debug_code_objects() & 2048)
al.align(batch, None, max_error=400, compute_cigar=False, affine2p=(4, 6, 2, 24, 1), wfadaptive=(10, 50, 1))
print("call", lib.wfagpu_amd_debug_code_objects() & 2048)
"""


@pytest.mark.parametrize("mode,want", [("calls", ["prime 0", "others 0", f"call {UNIT_2PAD}"]), ("prime", [f"prime {UNIT_2PAD | 4}"])])
def test_code_object_accounting(mode, want):
    """Fresh processes: prime with nothing configured, gap-affine, span, plain two-piece and plain adaptive calls never enter the new
    unit, a call under the pair does; prime does once the pair is configured (with the two-piece backtrace, bit 4, and nothing else)."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _FRESH_PROCESS, mode], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert all(w in r.stdout.splitlines() for w in want), r.stdout


@pytest.mark.parametrize("key", sorted(ar.groups(ar.read_golden("small"))), ids=lambda k: "-".join(map(str, k[0] + k[1])))
def test_cli(sets, tmp_path, key):
    """--affine2p with --affine2p-wfa-adaptive on every (heuristic, penalties) group of `small`, without the two empty-sequence pairs (a
    .seq file cannot carry one), -x -c -o: the golden bytes; Incorrect=0 although texts of some groups cost less than their score; the
    count above the optimum that -c reports is the one the goldens and the dynamic program give."""
    g = sets["small"]
    heur, pen = key
    keep = [i for i in ar.groups(g)[key] if g["pairs"][i][0] and g["pairs"][i][1]]
    seq, out = tmp_path / "in.seq", tmp_path / "res.out"
    seq.write_bytes(b"".join(b">" + g["pairs"][i][0] + b"\n<" + g["pairs"][i][1] + b"\n" for i in keep))
    r = subprocess.run([CLI, "-i", str(seq), "--affine2p", ",".join(map(str, pen)), "--affine2p-wfa-adaptive", ",".join(map(str, heur)), "-e", "800",
                        "-x", "-c", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"correct={len(keep)} Incorrect=0" in r.stderr, r.stderr[-2000:]
    above = sum(int(g["scores"][i]) > a2.dp_affine2p_score(*g["pairs"][i], pen) for i in keep)
    assert f"wf-adaptive: {above} pairs above the optimum" in r.stderr, r.stderr[-2000:]
    golden_lines = open(ar.golden_path("small"), "rb").read().splitlines(keepends=True)
    assert out.read_bytes() == b"".join(golden_lines[i] for i in keep)
