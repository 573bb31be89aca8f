"""What two-piece gap-affine alignment costs: 1 kbp reads at 5 % error under (4,6,2,24,1), against the same pairs under gap-affine
(4,6,2) held to the careful loop (tuning.careful_only: the like-for-like baseline -- the two-piece kernels have no lean loop) and under
gap-affine as shipped; score-only and with CIGARs.  Prints the tier of the main launch and the LDS of a workgroup (one ring).
A library without the two-piece entry point (the parent commit) runs the gap-affine legs only.
   scratch/affine2p_probe.py [pairs] [repeats]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wfa-gpu_amd", "bindings")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, wfagpu
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
pen, pen2, me = (4, 6, 2), (4, 6, 2, 24, 1), 600
have_2p = hasattr(wfagpu.load(), "wfagpu_amd_align_device_2p")
buf, meta = wfagpu.generate_pairs(n, 1000, 0.05, seed=4242, nthreads=16)
print(f"{n} pairs of 1 kbp at 5 %; two-piece entry point: {have_2p}", flush=True)


def leg(name, cigar, affine2p=None, **tuning):
    al = wfagpu.DeviceAligner(0, **tuning); batch = al.upload(buf, meta)
    kw = {"affine2p": affine2p} if affine2p is not None else {}
    torch.cuda.synchronize(); t0 = time.perf_counter()
    al.align(batch, pen, max_error=me, compute_cigar=cigar, fetch=False, **kw)
    torch.cuda.synchronize(); cold = time.perf_counter() - t0
    al.hint_same_stream(True)
    al.align(batch, pen, max_error=me, compute_cigar=cigar, fetch=False, **kw)
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        al.align(batch, pen, max_error=me, compute_cigar=cigar, fetch=False, **kw)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        st = al.stats()
        print(f"{name}: step {dt * 1e3:.3f} ms, main launch {st.main_launch_ms:.3f} ms (tier {st.main_launch_tier}, LDS {st.lds_bytes_tier0} bytes, "
              f"{st.blocks_per_cu_tier0} workgroups per CU), align {st.align_ms:.3f} trace {st.trace_ms:.3f} ms, cells {st.cells}, passes {st.sub_batches}, "
              f"budget {st.auto_budget}, retried {st.pairs_retried}; first call of the context {cold * 1e3:.1f} ms", flush=True)
    al.close()


for cigar in (False, True):
    tag = "cigar" if cigar else "score"
    if have_2p:
        leg(f"two pieces (4,6,2,24,1) [{tag}]", cigar, affine2p=pen2)
    leg(f"gap-affine (4,6,2) careful_only no_auto_budget [{tag}]", cigar, careful_only=1, no_auto_budget=1)
    leg(f"gap-affine (4,6,2) careful_only [{tag}]", cigar, careful_only=1)
    leg(f"gap-affine (4,6,2) as shipped [{tag}]", cigar)
