#!/usr/bin/env python3
"""
Time of HWPSSFilterLO (cm2_hwpss_apply) at 1e8 detector samples: ns = 1e7 with 10 detectors and
ns = 1e8 with one, chunks of 2.5e6 samples, 10 % of the samples flagged, for 1, 4 and 8 harmonics; beside it a plain
device copy that moves the 36 bytes per sample the apply must move (v and the flags read twice, out written once:
the copy reads 18 B and writes 18 B per sample), the fit alone (sums and solve, without the subtract pass) and the
time of the constructor (tables, Gram sums, factorisation, one synchronise).

    python profiles/scripts/hwpss_filter_time.py [out.json]     # the GPU step under its own `timeout`
    python profiles/scripts/hwpss_filter_time.py --step gpu out.json

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
SHAPES = ((10_000_000, 10), (100_000_000, 1))
HARMS = (1, 4, 8)
CHUNK = 2_500_000
WARMUP, ROUNDS = 3, 20
BYTES_PER_SAMPLE = 36                       # 2 x (8 B of v + 4 B of flags) read, 8 B of out written


def step_gpu(out_path):
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import HWPSSFilterLO
    res = {"chunk": CHUNK, "warmup": WARMUP, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0),
           "bytes_per_sample": BYTES_PER_SAMPLE, "shapes": {}}
    for ns, ndet in SHAPES:
        n = ns * ndet
        g = torch.Generator(device="cuda").manual_seed(ns + ndet)
        chi = torch.arange(ns, device="cuda", dtype=torch.float64) * 0.13 + 1.0e4
        pix = torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int32)
        pix[torch.rand(n, generator=g, device="cuda") < 0.10] = -1
        v = torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
        out = D.empty(n)
        src = torch.zeros(n * BYTES_PER_SAMPLE // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        fns = {"copy moving 36 B per sample": lambda: dst.copy_(src)}
        create, info = {}, {}
        for H in HARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            F = HWPSSFilterLO(chi, pix, ndet=ndet, nharm=H, chunks=CHUNK)
            torch.cuda.synchronize()
            create[H] = 1e3 * (time.perf_counter() - t0)
            info[H] = F.filter_info()
            cf = D.empty(ndet * info[H]["nchunks"] * (2 * H + 1))
            fns["apply, H = %d" % H] = lambda F=F: _hip.call("cm2_hwpss_apply", F._handle.h, D.ptr(v), D.ptr(out),
                                                             D.stream())
            fns["fit only, H = %d" % H] = lambda F=F, cf=cf: _hip.call("cm2_hwpss_fit", F._handle.h, D.ptr(v),
                                                                       D.ptr(cf), D.stream())
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
        r = res["shapes"]["ns %d x ndet %d" % (ns, ndet)] = {"create_ms": {str(H): round(create[H], 3) for H in HARMS},
                                                             "info": {str(H): info[H] for H in HARMS}, "calls": {}}
        copy_med = statistics.median(ms["copy moving 36 B per sample"])
        for k, t in ms.items():
            med = statistics.median(t)
            r["calls"][k] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                             "ratio_to_copy": round(med / copy_med, 3),
                             "samples_per_s": round(n / (med * 1e-3), 1),
                             "GB_per_s_at_36_B": round(n * BYTES_PER_SAMPLE / (med * 1e-3) / 1e9, 1)}
        del fns, chi, pix, v, out, src, dst, F, cf
        torch.cuda.empty_cache()
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def main():
    if "--step" in sys.argv:
        return step_gpu(sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hwpss_filter_timing.json")
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "gpu", out]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
