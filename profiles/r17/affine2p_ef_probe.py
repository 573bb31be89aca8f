"""What the span costs over end-to-end two-piece alignment: 1 kbp reads at 5 % error under (4,6,2,24,1), each read against its mutated
copy end to end (wfagpu_amd_align_device_2p) and against the copy inside a 1.1 kbp window -- 50 random bases in front and behind -- under
the span (0,0,50,50) (wfagpu_amd_align_device_2p_span); score-only and with CIGARs, same session, same reads.
   profiles/r17/affine2p_ef_probe.py [pairs] [repeats]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "wfa-gpu_amd", "bindings")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, wfagpu
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
pen2, span, me = (4, 6, 2, 24, 1), (0, 0, 50, 50), 600
buf, meta = wfagpu.generate_pairs(n, 1000, 0.05, seed=4242, nthreads=16)
raw = buf.tobytes()
pad = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(17).integers(0, 4, size=(n, 100))]
pairs = [(raw[m["pattern_offset"]:m["pattern_offset"] + m["pattern_len"]],
          pad[i, :50].tobytes() + raw[m["text_offset"]:m["text_offset"] + m["text_len"]] + pad[i, 50:].tobytes()) for i, m in enumerate(meta)]
wbuf, wmeta = wfagpu.layout_pairs(pairs)
print(f"{n} reads of 1 kbp at 5 % under {pen2}; windows of {int(wmeta['text_len'].mean())} bases under {span}", flush=True)


def leg(name, cigar, b, m, **kw):
    al = wfagpu.DeviceAligner(0); batch = al.upload(b, m)
    for i in range(reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        al.align(batch, None, max_error=me, compute_cigar=cigar, fetch=False, affine2p=pen2, **kw)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        st = al.stats()
        if i:
            print(f"{name}: step {dt * 1e3:.3f} ms, wavefront kernels {st.align_ms:.3f} ms, backtrace {st.trace_ms:.3f} ms (main launch tier {st.main_launch_tier}, "
                  f"{st.blocks_per_cu_tier0} workgroups per CU), cells {st.cells}, passes {st.sub_batches}, retried {st.pairs_retried}", flush=True)
    al.close()


for cigar in (False, True):
    tag = "cigar" if cigar else "score"
    leg(f"end to end [{tag}]", cigar, buf, meta)
    leg(f"window, span {span} [{tag}]", cigar, wbuf, wmeta, span=span)
