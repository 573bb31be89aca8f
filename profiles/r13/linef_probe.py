"""Edit under the span (0,0,50,50): the new kernels against the emulation a caller had (gap-affine (1,0,1) under the same span on the
gap-affine ends-free kernels).  100k pairs of a 150 bp read in a 250 bp window and of a 1 kbp read in a 1.1 kbp window, ~5 % error,
score-only and with CIGARs; stage timers of DeviceAligner.stats(), the two alternated, medians of 9 after 2 warm-up calls each."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "wfa-gpu_amd", "bindings"))
import wfagpu  # noqa: E402

N, SPAN, REPS = 100_000, (0, 0, 50, 50), 9
out = {}
al = wfagpu.DeviceAligner(0)
for read, budget in ((150, 60), (1000, 200)):
    buf, meta = wfagpu.generate_pairs(N, read, 0.05, seed=20261021 + read)
    pairs = wfagpu.pairs_from_layout(buf, meta)
    rng = np.random.default_rng(read)
    flank = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(N, 100))]
    pairs = [(p, flank[i, :50].tobytes() + t + flank[i, 50:].tobytes()) for i, (p, t) in enumerate(pairs)]
    buf, meta = wfagpu.layout_pairs(pairs)
    batch = al.upload(buf, meta)
    for cigar in (False, True):
        runs = {"linef": dict(linear=("edit",)), "emulation": {}}
        res, times = {}, {k: [] for k in runs}
        for rep in range(2 + REPS):
            for name, kw in runs.items():
                t0 = time.perf_counter()
                s, c = al.align(batch, None if kw else (1, 0, 1), max_error=budget, compute_cigar=cigar, span=SPAN, **kw)
                wall = (time.perf_counter() - t0) * 1e3
                st = al.stats()
                res[name] = (s, c)
                if rep >= 2:
                    times[name].append((st.align_ms, st.trace_ms, st.total_ms, wall, st.pairs_retried, list(st.pairs_tier)))
        same_scores = bool(np.array_equal(res["linef"][0], res["emulation"][0]))
        same_cigars = (res["linef"][1] == res["emulation"][1]) if cigar else None
        key = f"read{read}_{'cigar' if cigar else 'score'}"
        out[key] = {"same_scores": same_scores, "same_cigars": same_cigars, "max_score": int(res["linef"][0].max()), "failed": int((res["linef"][0] < 0).sum())}
        for name in runs:
            a = np.array([t[:4] for t in times[name]], dtype=np.float64)
            out[key][name] = {"align_ms_median": float(np.median(a[:, 0])), "align_ms_min": float(a[:, 0].min()), "align_ms_max": float(a[:, 0].max()),
                              "trace_ms_median": float(np.median(a[:, 1])), "total_ms_median": float(np.median(a[:, 2])),
                              "wall_ms_median": float(np.median(a[:, 3])), "pairs_retried": times[name][-1][4], "pairs_tier": times[name][-1][5]}
        print(key, json.dumps(out[key]), flush=True)
al.close()
with open(os.path.join(HERE, "linef_probe.json"), "w") as f:
    json.dump(out, f, indent=1)
