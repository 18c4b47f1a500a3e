#!/usr/bin/env python3
"""
Time of CommonModeFilterLO (cm2_cmode_apply, cm2_cmode_fit) at 1e8 detector samples: ns = 1e7 with 10
detectors and ns = 1e5 with 1000, one group, 10 % of the samples flagged at random (and, for ten detectors, none: with
ten templates only a sample with no flag at all is fitted), for K = 1 (ones) and K = 3, 6, 10 (the monomials of degree
<= 1, 2, 3 of random positions); beside it a plain device copy that moves the 32 bytes per sample the apply must move
(v and the flags read twice, out written once: the copy reads 16 B and writes 16 B per sample), the fit alone and the
time of the constructor (the class of every unit, one synchronise).

    python profiles/scripts/cmode_filter_time.py [out.json]     # the GPU step under its own `timeout`
    python profiles/scripts/cmode_filter_time.py --step gpu out.json

One process; per shape 3 warm-up calls of every variant and of the copy, then 20 rounds in which every variant is
called once (variants alternated), each timed by a host clock around the call and a device synchronise; median, min,
max in ms.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SHAPES = ((10_000_000, 10, 0.10), (100_000, 1000, 0.10), (10_000_000, 10, 0.0))       # ns, ndet, flagged
TEMPLATES = ((1, 0), (3, 1), (6, 2), (10, 3))                                         # K, order
WARMUP, ROUNDS = 3, 20
BYTES_PER_SAMPLE = 32                       # 2 x (8 B of v + 4 B of flags) read, 8 B of out written
COPY = "copy moving 32 B per sample"


def step_gpu(out_path):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import CommonModeFilterLO, focalplane_modes
    res = {"warmup": WARMUP, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0),
           "bytes_per_sample": BYTES_PER_SAMPLE, "shapes": {}}
    for ns, ndet, flagged in SHAPES:
        n = ns * ndet
        g = torch.Generator(device="cuda").manual_seed(ns + ndet)
        pix = torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int32)
        if flagged:
            pix[torch.rand(n, generator=g, device="cuda") < flagged] = -1
        v = torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
        out = D.empty(n)
        cf = D.empty(TEMPLATES[-1][0] * ns)
        src = torch.zeros(n * BYTES_PER_SAMPLE // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        xy = np.random.default_rng(ndet).uniform(-1.0, 1.0, (ndet, 2))
        fns = {COPY: lambda: dst.copy_(src)}
        create, info = {}, {}
        for K, order in TEMPLATES:
            modes = focalplane_modes(xy, order)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            F = CommonModeFilterLO(pix, ndet, modes=modes)
            torch.cuda.synchronize()
            create[K] = 1e3 * (time.perf_counter() - t0)
            info[K] = F.filter_info()
            fns["apply, K = %d" % K] = lambda F=F: _hip.call("cm2_cmode_apply", F._handle.h, D.ptr(v), D.ptr(out),
                                                             D.stream())
            fns["fit only, K = %d" % K] = lambda F=F: _hip.call("cm2_cmode_fit", F._handle.h, D.ptr(v), D.ptr(cf),
                                                                D.stream())
        for _ in range(WARMUP):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0))
        key = "ns %d x ndet %d, %d %% flagged" % (ns, ndet, round(100 * flagged))
        r = res["shapes"][key] = {"create_ms": {str(K): round(create[K], 3) for K, _ in TEMPLATES},
                                  "info": {str(K): info[K] for K, _ in TEMPLATES}, "calls": {}}
        copy_med = statistics.median(ms[COPY])
        for k, t in ms.items():
            med = statistics.median(t)
            r["calls"][k] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                             "ratio_to_copy": round(med / copy_med, 3),
                             "samples_per_s": round(n / (med * 1e-3), 1),
                             "GB_per_s_at_32_B": round(n * BYTES_PER_SAMPLE / (med * 1e-3) / 1e9, 1)}
        del fns, pix, v, out, cf, src, dst, F
        torch.cuda.empty_cache()
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def main():
    if "--step" in sys.argv:
        return step_gpu(sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cmode_filter_timing.json")
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "gpu", out]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
