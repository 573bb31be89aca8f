"""Does wf-adaptive pay under two pieces?  The exact two-piece call (wfagpu_amd_align_device_2p) against the heuristic (10,50,1)
(wfagpu_amd_align_device_2p_adaptive) under (4,6,2,24,1) on the same resident batches: 100k x 1 kbp at 5 %, 1024 x 10 kbp and
1024 x 30 kbp at 10 %, score-only and with CIGARs, same session.  WFAGPU_PROBE_EXACT_ONLY=1: the exact legs alone (what a checkout of
the parent commit can run).
   profiles/r18/affine2p_wfadaptive_probe.py [repeats]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "wfa-gpu_amd", "bindings"))
import numpy as np, torch, wfagpu
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2
exact_only = os.environ.get("WFAGPU_PROBE_EXACT_ONLY") == "1"
pen2, heur = (4, 6, 2, 24, 1), (10, 50, 1)
SHAPES = ((100_000, 1000, 0.05, 600), (1024, 10_000, 0.10, 8000), (1024, 30_000, 0.10, 24000))


def leg(name, batch, al, me, cigar, **kw):
    scores = None
    for i in range(reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        d_scores, _ = al.align(batch, None, max_error=me, compute_cigar=cigar, fetch=False, affine2p=pen2, **kw)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        st = al.stats()
        scores = d_scores.cpu().numpy().copy()
        if i:
            print(f"{name}: step {dt * 1e3:.2f} ms, wavefront kernels {st.align_ms:.2f} ms, backtrace {st.trace_ms:.2f} ms, cells {st.cells}, "
                  f"pairs by tier {list(st.pairs_tier)[:6]}, passes {st.sub_batches}, retried {st.pairs_retried}", flush=True)
    return scores


for n, length, err, me in SHAPES:
    buf, meta = wfagpu.generate_pairs(n, length, err, seed=4242, nthreads=16)
    print(f"--- {n} x {length} bases at {err:.0%} under {pen2}, max_error {me}", flush=True)
    al = wfagpu.DeviceAligner(0); batch = al.upload(buf, meta)
    for cigar in (False, True):
        tag = "cigar" if cigar else "score"
        exact = leg(f"exact [{tag}]", batch, al, me, cigar)
        if not exact_only:
            ad = leg(f"wf-adaptive {heur} [{tag}]", batch, al, me, cigar, wfadaptive=heur)
            assert (ad >= exact).all()
            print(f"pairs above the optimum: {int((ad > exact).sum())} of {n} ({(ad > exact).mean():.1%}), mean excess {float((ad - exact).mean()):.1f}", flush=True)
    al.close()
