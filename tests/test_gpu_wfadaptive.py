"""The wf-adaptive heuristic on the GPU: wfagpu_amd_align_device_adaptive, wfagpu_amd_configure_wfadaptive behind the launch_alignments*
seam and the CLI, against WFA2's scores and CIGARs under the same heuristic (tests/golden/wfadaptive.*, made by
tests/golden/make_golden_wfadaptive.py; the sets are described in tests/wfadaptive_ref.py).  The heuristic is deterministic: every
comparison is byte for byte."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import wfadaptive_ref as wa
import wfagpu
from endsfree_ref import sweep_budget_groups, sweep_over

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(wfagpu.LIB_PATH)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")
# score budgets of the first tier.  small: 400 keeps the ring within the one-wave tier (golden scores reach 658: the rest is escalated);
# the others lie above every golden score of their set (indel: 516, defaults1k: 2348, long: 3410, beyond16: 1002, small_default: 353)
MAX_ERROR = {"small": 400, "indel": 700, "defaults1k": 2600, "long": 3600, "beyond16": 1200, wa.ONE_SET: 400}


@pytest.fixture(scope="module")
def sets():
    return {name: wa.read_golden(name) for name in wa.ALL_SETS}


def _run_set(al, g, cigar, max_error, only=None, heur=None):
    """Every (heuristic, penalties) group of a golden set as one call -> scores, cigars in the set's order (only: a subset of indices;
    heur: one heuristic for all instead of the set's).  No pair is skipped: every index must have come back."""
    n = len(g["pairs"])
    scores = np.full(n, -12345, dtype=np.int64)
    cigars = [None] * n
    seen = 0
    stats = []
    for (h, pen), idx in wa.groups(g).items():
        if only is not None:
            idx = [i for i in idx if i in only]
            if not idx:
                continue
        buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
        batch = al.upload(buf, meta)
        s, c = al.align(batch, pen, max_error=max_error, compute_cigar=cigar, wfadaptive=heur or h)
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
        where = (i, len(p), len(t), g["pens"][i], g["heurs"][i])
        assert scores[i] == g["scores"][i], where
        if cigar:
            assert cigars[i] == g["cigars"][i], where


@pytest.mark.parametrize("name", wa.ALL_SETS)
@pytest.mark.parametrize("cigar", [False, True])
def test_golden_sets(sets, name, cigar):
    """score == WFA2's and CIGAR == WFA2's, byte for byte (the files' CIGARs are valid and cost their score: test_wfadaptive_cpu.py)."""
    g = sets[name]
    al = wfagpu.DeviceAligner(0)
    try:
        scores, cigars, stats = _run_set(al, g, cigar, MAX_ERROR[name])
        _check_set(g, scores, cigars, cigar)
        if name == "small":
            assert sum(st.pairs_tier[0] for st in stats) > 300 and sum(st.pairs_raw for st in stats) >= 8
        if name == "beyond16":
            assert sum(st.pairs_tier[3] for st in stats) == len(g["pairs"])
        assert all(st.pairs_tier[4] == 0 and st.pairs_tier[5] == 0 and st.pairs_banded == 0 and st.auto_budget == 0 for st in stats)
    finally:
        al.close()


@pytest.mark.parametrize("variant", ["min_tier1", "min_tier2", "min_tier3", "max_error8", "small_arena", "trace_mode1", "trace_mode2"])
def test_indel_defaults1k_and_long_on_every_path(sets, variant):
    """The same batches forced through the wider tiers, through escalation (a budget of 8: every pair misses it), through several
    arena-bound passes, and through the mappings of the backtrace: the same bytes."""
    kw, max_error = {}, None
    if variant.startswith("min_tier"):
        kw["min_tier"] = int(variant[-1])
    elif variant.startswith("trace_mode"):
        kw["trace_mode"] = int(variant[-1])
    elif variant == "max_error8":
        max_error = 8
    elif variant == "small_arena":
        # (a fixed arena of 4 MiB: a pair of defaults1k under (10,50,10) writes up to 1 MB of origin bytes -- ten scores of growth between
        # cut-offs, rows of 1600 diagonals --, so one alignment fits and a group of eight such pairs does not)
        kw["arena_bytes"] = 4 << 20
    al = wfagpu.DeviceAligner(0, **kw)
    try:
        passes = retried = 0
        for name in ("indel", "defaults1k", "long"):
            g = sets[name]
            scores, cigars, stats = _run_set(al, g, True, max_error or MAX_ERROR[name])
            _check_set(g, scores, cigars, True)
            passes = max(passes, max(st.sub_batches for st in stats))
            retried += sum(st.pairs_retried for st in stats)
            if variant.startswith("min_tier"):
                t = int(variant[-1])
                assert all(sum(st.pairs_tier[:t]) == 0 for st in stats)
        if variant == "max_error8":
            assert retried >= 64 + 48 + 8
        if variant == "small_arena":
            assert passes > 1
    finally:
        al.close()


# the penalties the gap-affine goldens were made under (tests/test_oracle.py: PENS)
UTEST_PENS = {"p0": (1, 2, 1), "p1": (3, 1, 4), "p2": (5, 3, 2)}


@pytest.mark.parametrize("heur", [(10, 1 << 20, 1), (1 << 20, 50, 1)], ids=["threshold", "min_length"])
def test_a_heuristic_that_never_cuts_gives_the_gap_affine_goldens(golden_dir, heur):
    """A threshold no distance exceeds, and separately a length no row reaches: the existing gap-affine goldens (utest.affine.p0/p1/p2:
    WFA2's exact answers), byte for byte, through the adaptive kernels."""
    pairs = wfagpu.read_seq_file(os.path.join(golden_dir, "wfa.utest.seq"))
    buf, meta = wfagpu.layout_pairs(pairs)
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        for tag in ("p0", "p1", "p2"):
            gs, gc = oracle_lib.read_alg(os.path.join(golden_dir, f"utest.affine.{tag}.alg"))
            pen = UTEST_PENS[tag]
            s, c = al.align(batch, pen, max_error=int(gs.max()) + 1, compute_cigar=True, wfadaptive=heur)
            assert np.array_equal(s, gs[:len(s)]) and list(c) == list(gc[:len(c)]), (tag, pen)
            assert wfagpu.load().wfagpu_amd_debug_code_objects() & 8
            s, _ = al.align(batch, pen, max_error=int(gs.max()) + 1, compute_cigar=False, wfadaptive=heur)
            assert np.array_equal(s, gs[:len(s)]), (tag, pen)
    finally:
        al.close()


def test_the_heuristic_computes_fewer_cells_than_the_exact_search(sets):
    """long under WFA2's defaults (10,50,1) against the same batch's exact run held to the careful loop: an inequality only."""
    g = sets["long"]
    buf, meta = wfagpu.layout_pairs(g["pairs"])
    al = wfagpu.DeviceAligner(0, careful_only=1)
    try:
        batch = al.upload(buf, meta)
        al.align(batch, (2, 3, 1), max_error=3600, compute_cigar=False)
        exact_cells = al.stats().cells
        al.align(batch, (2, 3, 1), max_error=3600, compute_cigar=False, wfadaptive=wa.DEFAULTS)
        assert 0 < al.stats().cells < exact_cells
    finally:
        al.close()


def test_big_batch(sets):
    """20 000 copies drawn from small_default in one call, score-only and with CIGARs: every copy gets its original's answer."""
    g = sets[wa.ONE_SET]
    pick = (wa.Rng(20260906).u64(20000) % np.uint64(len(g["pairs"]))).astype(np.int64)
    buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in pick])
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        s, _ = al.align(batch, wa.ONE_PEN, max_error=MAX_ERROR[wa.ONE_SET], compute_cigar=False, wfadaptive=wa.ONE_HEUR)
        assert al.stats().auto_budget == 0      # (no budgets from a sample under the heuristic)
        assert np.array_equal(s, g["scores"][pick])
        s, c = al.align(batch, wa.ONE_PEN, max_error=MAX_ERROR[wa.ONE_SET], compute_cigar=True, wfadaptive=wa.ONE_HEUR)
        assert np.array_equal(s, g["scores"][pick]) and list(c) == [g["cigars"][i] for i in pick]
    finally:
        al.close()


def test_bad_members_and_a_null_heuristic(sets):
    """-1 for a bad member; heuristic == NULL: wfagpu_amd_align_device with BAND_NONE (the exact answers)."""
    g = sets["indel"]
    buf, meta = wfagpu.layout_pairs(g["pairs"][:16])
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        for bad in ((0, 50, 1), (10, -1, 1), (10, 50, 0)):
            with pytest.raises(RuntimeError):
                al.align(batch, (2, 3, 1), max_error=700, compute_cigar=False, wfadaptive=bad)
        torch = al.torch
        d_scores = torch.empty(16, dtype=torch.int32, device=torch.device("cuda", al.device))
        t, o, l = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = al.lib.wfagpu_amd_align_device_adaptive(al.ctx, C.byref(batch), wfagpu.Penalties(2, 3, 1), 700, None, True, d_scores.data_ptr(),
                                                     C.byref(t), C.byref(o), C.byref(l))
        assert rc == 0
        s_ref, _, _ = oracle_lib.oracle_batch(buf, meta, (2, 3, 1), cigar=False)
        assert np.array_equal(d_scores.cpu().numpy(), s_ref)
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


def test_configured_heuristic_behind_the_launch_seam(sets):
    """wfagpu_amd_configure_wfadaptive: launch_alignments and launch_alignments_distance on two device slots with a batch size that cuts
    the call; a band that is asked for is not used; after configure(NULL) the very same call gives the exact answers of the oracle again."""
    g = sets[wa.ONE_SET]
    buf, meta = wfagpu.layout_pairs(g["pairs"])
    ex_scores, ex_cigars, _ = oracle_lib.oracle_batch(buf, meta, wa.ONE_PEN, cigar=True)
    assert not np.array_equal(ex_scores, g["scores"])      # (the heuristic does change answers on these pairs)
    try:
        wfagpu.configure_launch(virtual_devices=2)
        wfagpu.configure_wfadaptive(wa.ONE_HEUR)
        s, c = _launch(g["pairs"], wa.ONE_PEN, True, 400, 37)
        assert np.array_equal(s, g["scores"]) and c == g["cigars"]
        s, _ = _launch(g["pairs"], wa.ONE_PEN, False, 400, 37)
        assert np.array_equal(s, g["scores"])
        s, c = _launch(g["pairs"], wa.ONE_PEN, True, 400, 150, band=25, band_width=64)
        assert np.array_equal(s, g["scores"]) and c == g["cigars"]
        wfagpu.configure_wfadaptive()
        s, c = _launch(g["pairs"], wa.ONE_PEN, True, 400, 37)
        assert np.array_equal(s, ex_scores) and c == list(ex_cigars)
    finally:
        wfagpu.configure_wfadaptive()


def _api_align(pairs, pen, cigar, batch=None, max_error=None):
    """The wfagpu_* C API of lib/aligner.c, as tests/test_gpu_api_cli.py drives it."""
    lib = wfagpu.load()
    al = wfagpu.Aligner()
    assert lib.wfagpu_initialize_aligner(C.byref(al))
    for p, t in pairs:
        assert lib.wfagpu_add_sequences(C.byref(al), p, t)
    assert lib.wfagpu_initialize_parameters(C.byref(al), wfagpu.Penalties(*pen))
    if batch:
        assert lib.wfagpu_set_batch_size(C.byref(al), batch)
    if max_error:
        al.alignment_options.max_error = max_error
    al.alignment_options.compute_cigar = cigar
    assert lib.wfagpu_align(C.byref(al))
    n = al.num_sequence_pairs
    scores = np.array([al.results[i].error for i in range(n)], dtype=np.int64)
    cigars = [C.string_at(al.results[i].cigar.buffer).decode() for i in range(n)] if cigar else None
    lib.wfagpu_destroy_aligner(C.byref(al))
    return scores, cigars


def test_configured_heuristic_behind_wfagpu_align(sets):
    """wfagpu_initialize_aligner / wfagpu_add_sequences / wfagpu_initialize_parameters / wfagpu_align under
    wfagpu_amd_configure_wfadaptive: small_default score-only and with CIGARs, byte for byte; after configure(NULL) the same calls give
    the exact answers of the oracle again."""
    g = sets[wa.ONE_SET]
    buf, meta = wfagpu.layout_pairs(g["pairs"])
    ex_scores, ex_cigars, _ = oracle_lib.oracle_batch(buf, meta, wa.ONE_PEN, cigar=True)
    try:
        wfagpu.configure_wfadaptive(wa.ONE_HEUR)
        s, _ = _api_align(g["pairs"], wa.ONE_PEN, False, batch=150, max_error=400)
        assert np.array_equal(s, g["scores"])
        s, c = _api_align(g["pairs"], wa.ONE_PEN, True, batch=150, max_error=400)
        assert np.array_equal(s, g["scores"]) and c == g["cigars"]
        wfagpu.configure_wfadaptive()
        s, _ = _api_align(g["pairs"], wa.ONE_PEN, False, batch=150, max_error=400)
        assert np.array_equal(s, ex_scores)
        s, c = _api_align(g["pairs"], wa.ONE_PEN, True, batch=150, max_error=400)
        assert np.array_equal(s, ex_scores) and c == list(ex_cigars)
    finally:
        wfagpu.configure_wfadaptive()


_BAND_UNDER_HEURISTIC = r"""
import ctypes as C
import wfagpu
lib = wfagpu.load()
buf, meta = wfagpu.generate_pairs(64, 300, 0.05, seed=11)
wfagpu.configure_wfadaptive((10, 50, 1))
for _ in range(2):
    res = C.POINTER(wfagpu.AlignmentResult)()
    assert lib.initialize_wfa_results(C.byref(res), 64, 1)
    opt = wfagpu.Options(max_error=100, threads_per_block=64, num_workers=1, band=25, batch_size=40, num_alignments=64,
                         penalties=wfagpu.Penalties(2, 3, 1), compute_cigar=False)
    lib.launch_alignments_distance(buf.ctypes.data, buf.nbytes, meta.ctypes.data, res, opt, False)
    lib.destroy_wfa_results(res, 64)
print("entered", lib.wfagpu_amd_debug_code_objects())
"""


def test_a_band_under_the_configured_heuristic_is_said_once():
    """A fresh process: two launch_alignments_distance calls of two batches each with -B 25 -t 64 under the configured heuristic run on
    the adaptive kernels alone (bit 3, nothing else entered) and say so on stderr exactly once."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _BAND_UNDER_HEURISTIC], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "entered 8" in r.stdout, r.stdout
    assert r.stderr.count("WARNING: the adaptive band is not combined with the wf-adaptive heuristic") == 1, r.stderr[-2000:]


def test_cli_wfa_adaptive(sets, tmp_path):
    """--wfa-adaptive with -x -c -o on small_default written as a .seq file: the output file is the golden .alg byte for byte; the -c
    verification finds nothing wrong and says how many pairs lie above the optimum.  A .seq file cannot carry an empty sequence: the
    two pairs of the set that have one are left out of the input, and their two lines out of the golden bytes."""
    g = sets[wa.ONE_SET]
    seq = tmp_path / "nonempty.seq"
    keep = [i for i, (p, t) in enumerate(g["pairs"]) if p and t]
    assert len(keep) == len(g["pairs"]) - 2
    with open(seq, "wb") as f:
        for i in keep:
            f.write(b">" + g["pairs"][i][0] + b"\n<" + g["pairs"][i][1] + b"\n")
    out = tmp_path / "res.out"
    r = subprocess.run([CLI, "-i", str(seq), "--wfa-adaptive", ",".join(str(v) for v in wa.ONE_HEUR), "-g", "2,3,1", "-e", "400", "-x", "-c",
                        "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Incorrect=0" in r.stderr and all(tok == "Incorrect=0" for tok in r.stderr.split() if tok.startswith("Incorrect="))
    opt, _ = wa.exact_answers([g["pairs"][i] for i in keep], [wa.ONE_PEN] * len(keep))
    above = int((g["scores"][keep] > opt).sum())
    assert above > 0 and f"wf-adaptive: {above} pairs above the optimum" in r.stderr, r.stderr[-2000:]
    golden_lines = open(wa.golden_path(wa.ONE_SET), "rb").read().splitlines(keepends=True)
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
al.align(batch, (2, 3, 1), max_error=100, compute_cigar=True, span=(0, 0, 20, 20))
al.align(batch, None, max_error=400, compute_cigar=True, affine2p=(4, 6, 2, 24, 1))
print("others", lib.wfagpu_amd_debug_code_objects())
al.close()
"""

_FRESH_ADAPTIVE = r"""
import wfagpu
lib = wfagpu.load()
buf, meta = wfagpu.generate_pairs(64, 300, 0.05, seed=11)
al = wfagpu.DeviceAligner(0)
batch = al.upload(buf, meta)
al.align(batch, (2, 3, 1), max_error=100, compute_cigar=False, wfadaptive=(10, 50, 1))
print("adaptive scores", lib.wfagpu_amd_debug_code_objects())
al.align(batch, (2, 3, 1), max_error=100, compute_cigar=True, wfadaptive=(10, 50, 1))
print("adaptive cigars", lib.wfagpu_amd_debug_code_objects())
al.close()
wfagpu.configure_wfadaptive((10, 50, 1))
al = wfagpu.DeviceAligner(0)
assert lib.wfagpu_amd_prime(al.ctx) == 0
print("primed", lib.wfagpu_amd_debug_code_objects())
al.close()
"""


def _fresh(script):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(line.rsplit(" ", 1) for line in r.stdout.splitlines() if " " in line), r.stdout


def test_only_adaptive_calls_load_the_adaptive_code_object():
    """Fresh processes.  wfagpu_amd_prime with nothing configured and gap-affine (exact and banded), ends-free and two-piece calls never set
    bit 3 of wfagpu_amd_debug_code_objects; an adaptive call, score-only or with CIGARs (the gap-affine backtrace kernels serve it),
    sets bit 3 and none of the others; so does wfagpu_amd_prime once the heuristic is configured."""
    seen, out = _fresh(_FRESH_PROCESS)
    assert seen == {"gap-affine": "0", "others": "7"}, out
    seen, out = _fresh(_FRESH_ADAPTIVE)
    assert seen == {"adaptive scores": "8", "adaptive cigars": "8", "primed": "8"}, out


# ---- the sweep: seven penalty sets under five heuristics and tight budgets (wfadaptive_ref.SWEEP_PENS, SWEEP_HEUR) -----------------
SWEEP_PATHS = ["as shipped", "min_tier1", "min_tier2", "min_tier3", "max_error8"]


@pytest.fixture(scope="module")
def sweep():
    return wa.read_golden(wa.SWEEP_SET)


def _factor(key):
    return math.gcd(*key[1])


@pytest.mark.parametrize("cigar", [False, True])
@pytest.mark.parametrize("path", SWEEP_PATHS)
def test_sweep_golden(sweep, cigar, path):
    """Every (heuristic, penalties) group of the sweep as one call under a budget of its largest golden score plus 1 (max_error8: of 8) --
    as shipped and forced through the wider tiers: WFA2's scores and CIGAR bytes under the same heuristic."""
    g = sweep
    al = wfagpu.DeviceAligner(0, **({"min_tier": int(path[-1])} if path.startswith("min_tier") else {}))
    try:
        for key, idx in wa.groups(g).items():
            budget = 8 if path == "max_error8" else int(g["scores"][idx].max()) + 1
            scores, cigars, (st,) = _run_set(al, g, cigar, budget, only=set(idx))
            _check_set(g, scores, cigars, cigar, only=set(idx))
            if path.startswith("min_tier"):
                assert sum(st.pairs_tier[:int(path[-1])]) == 0, key
            if path == "max_error8":
                assert st.pairs_retried >= sweep_over(g["scores"][idx], 8, _factor(key)), key
    finally:
        al.close()


def test_ring_depth_on_either_side_of_the_one_wave_limit(sweep):
    """plan_tier keeps an M ring of more than 64 rows (max(x, o + e) + 1: endsfree_ref.ring_depth) off the one-wave tier: as shipped,
    under budgets just above the golden scores, a penalty set whose ring has at most 64 rows -- (2,62,1) has 64 -- has pairs on
    tier 0 and no call of one with a deeper ring -- (2,64,1) has 66 -- has any, and both give WFA2's bytes.  Counted per penalty set, over its five heuristics (the ring of window_width_ad is twice the exact one: a
    call with a 700-base pair may outgrow the one-wave tier whatever the depth)."""
    g = sweep
    al = wfagpu.DeviceAligner(0)
    try:
        tier0, depths = {}, {}
        for (heur, pen), idx in wa.groups(g).items():
            scores, cigars, (st,) = _run_set(al, g, True, int(g["scores"][idx].max()) + 1, only=set(idx))
            _check_set(g, scores, cigars, True, only=set(idx))
            depths[pen] = wa.ring_depth(pen)
            tier0[pen] = tier0.get(pen, 0) + st.pairs_tier[0]
            assert depths[pen] <= 64 or st.pairs_tier[0] == 0, (heur, pen, list(st.pairs_tier))
        assert set(tier0) == set(wa.SWEEP_PENS) and {64, 66} <= set(depths.values())
        for pen in wa.SWEEP_PENS:
            assert (tier0[pen] > 0) == (depths[pen] <= 64), (pen, depths[pen], tier0[pen])
    finally:
        al.close()


def test_score_budget_window_is_exact(sweep):
    """The counterpart of test_gpu_parity.py's test_score_budget_window_is_exact: the pairs of a (heuristic, penalties) group that share
    a golden score -- the heuristic's own, not the optimum -- run under a budget of exactly that score -- the ring of window_width_ad
    has to hold them: no pair comes back for a wider one -- and of one less -- every pair does --, and give WFA2's bytes both times.
    (6,9,3) runs as (2,3,1) with the budget divided by 3, rounded down, and the steps between cut-offs counted in the reduced scores:
    score and score - 1 still fall on either side."""
    g = sweep
    chosen = sweep_budget_groups(list(zip(g["heurs"], g["pens"])), g["scores"], _factor, seed=20261014)
    assert {k for k, _, _ in chosen} == {(h, pen) for h in wa.SWEEP_HEUR for pen in wa.SWEEP_PENS} and len(chosen) <= 48
    al = wfagpu.DeviceAligner(0)
    try:
        for key, score, idx in chosen:
            for budget in (score, score - 1):
                scores, cigars, (st,) = _run_set(al, g, True, budget, only=set(idx))
                _check_set(g, scores, cigars, True, only=set(idx))
                assert st.pairs_retried == (0 if budget == score else len(idx)), (key, score, budget, len(idx))
    finally:
        al.close()


def test_sweep_behind_the_launch_seam(sweep):
    """wfagpu_amd_configure_wfadaptive with each heuristic of the sweep under penalties that have a common factor and under a ring
    deeper than 64 rows, through launch_alignments with a batch size that cuts the call: the golden bytes."""
    g = sweep
    groups = wa.groups(g)
    try:
        for pen in ((6, 9, 3), (2, 64, 1)):
            for heur in wa.SWEEP_HEUR:
                idx = groups[(heur, pen)]
                wfagpu.configure_wfadaptive(heur)
                s, c = _launch([g["pairs"][i] for i in idx], pen, True, int(g["scores"][idx].max()) + 1, 3)
                assert np.array_equal(s, g["scores"][idx]) and c == [g["cigars"][i] for i in idx], (heur, pen)
    finally:
        wfagpu.configure_wfadaptive()
