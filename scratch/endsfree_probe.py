"""What ends-free alignment costs: 1 kbp reads at 5 % error, the text padded by 100 random bases on each side, under the span
(0,0,200,200), with CIGARs and score-only; the unpadded pairs under a span of zeros (the ends-free kernels doing the end-to-end job);
and the baseline, the end-to-end kernels on the unpadded pairs held to the careful loop (tuning.careful_only: the same score loop, so
the difference is the termination scan and the wider start), with and without score budgets from a sample (a span switches them off).
A library without the span entry point (the parent commit) runs the baseline legs only.
   scratch/endsfree_probe.py [pairs] [repeats]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wfa-gpu_amd", "bindings")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, wfagpu
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
pen, me = (2, 3, 1), 300
have_span = hasattr(wfagpu.load(), "wfagpu_amd_align_device_span")
buf, meta = wfagpu.generate_pairs(n, 1000, 0.05, seed=4242, nthreads=16)
rng = np.random.default_rng(7)
acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
padded = [(p, acgt[rng.integers(0, 4, 100)].tobytes() + t + acgt[rng.integers(0, 4, 100)].tobytes()) for p, t in wfagpu.pairs_from_layout(buf, meta)]
pbuf, pmeta = wfagpu.layout_pairs(padded)
so = os.path.join(ROOT, "wfa-gpu_amd", "libwfagpu.so")
print(f"libwfagpu.so {os.path.getsize(so)} bytes; span entry point: {have_span}", flush=True)


def leg(name, b, m, cigar, span=None, **tuning):
    al = wfagpu.DeviceAligner(0, **tuning); batch = al.upload(b, m)
    kw = {"span": span} if span is not None else {}
    torch.cuda.synchronize(); t0 = time.perf_counter()
    al.align(batch, pen, max_error=me, compute_cigar=cigar, fetch=False, **kw)
    torch.cuda.synchronize(); cold = time.perf_counter() - t0
    al.hint_same_stream(True)
    al.align(batch, pen, max_error=me, compute_cigar=cigar, fetch=False, **kw)
    runs = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        al.align(batch, pen, max_error=me, compute_cigar=cigar, fetch=False, **kw)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        st = al.stats()
        runs.append((dt, st.main_launch_ms, st.main_launch_tier, st.cells, st.align_ms, st.trace_ms, st.auto_budget, st.pairs_retried))
    for dt, main, tier, cells, a_ms, t_ms, budget, retried in runs:
        print(f"{name}: {n / dt / 1e6:.3f} M alignments/s, step {dt * 1e3:.3f} ms, main launch {main:.3f} ms (tier {tier}), align {a_ms:.3f} trace {t_ms:.3f} ms, "
              f"cells {cells}, budget {budget}, retried {retried}; first call of the context {cold * 1e3:.1f} ms", flush=True)
    al.close()


for cigar in (True, False):
    tag = "cigar" if cigar else "score"
    leg(f"baseline end-to-end careful_only [{tag}]", buf, meta, cigar, careful_only=1)
    leg(f"baseline end-to-end careful_only no_auto_budget [{tag}]", buf, meta, cigar, careful_only=1, no_auto_budget=1)
    if have_span:
        leg(f"span zero, unpadded [{tag}]", buf, meta, cigar, span=(0, 0, 0, 0))
        leg(f"span (0,0,200,200), text padded 100+100 [{tag}]", pbuf, pmeta, cigar, span=(0, 0, 200, 200))
