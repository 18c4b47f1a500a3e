#!/usr/bin/env python3
"""
Time of TemplateFilterLO (cm2_template_apply) at 1e8 detector samples: ns = 1e6 with 100 detectors
(chunks of 2.5e5 samples) and ns = 1e7 with 10 (chunks of 2.5e6), 10 % of the samples flagged, for K = 1, 4, 9 and 16
(the constant and K - 1 templates); in the same process and alternated with it: the fit alone (sums and solve,
without the subtract pass), HWPSSFilterLO(nharm=4) on the same flags (K = 9, the yardstick: its code is not touched
here) and a plain device copy that moves the 36 bytes per sample an apply must move of the stream itself (v and the
flags read twice, out written once: the copy reads 18 B and writes 18 B per sample).  The time of each constructor
(copy and centring of the table, counts, Gram sums row by row, factorisation, one synchronise) is taken once.

    python profiles/scripts/template_filter_time.py [out.json]     # the GPU step under its own `timeout`
    python profiles/scripts/template_filter_time.py --step gpu out.json

One process; per shape 3 warm-up calls of every variant and of the copy, then 20 rounds in which every variant is
called once (variants alternated), each timed by a host clock around the call and a device synchronise; median, min,
max in ms.  "table_bytes" is what the design reads of the table per detector sample and pass, 8 (K - 1) / Dt.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SHAPES = ((1_000_000, 100, 250_000), (10_000_000, 10, 2_500_000))
KS = (1, 4, 9, 16)
NHARM = 4
WARMUP, ROUNDS = 3, 20
BYTES_PER_SAMPLE = 36                       # 2 x (8 B of v + 4 B of flags) read, 8 B of out written
COPY = "copy moving 36 B per sample"


def det_tile(K):
    return 4 if K <= 2 else 2               # cm2_template_policy.h


def step_gpu(out_path):
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import HWPSSFilterLO, TemplateFilterLO
    res = {"warmup": WARMUP, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0),
           "bytes_per_sample": BYTES_PER_SAMPLE, "shapes": {}}
    for ns, ndet, chunk in SHAPES:
        n = ns * ndet
        g = torch.Generator(device="cuda").manual_seed(ns + ndet)
        chi = torch.arange(ns, device="cuda", dtype=torch.float64) * 0.13 + 1.0e4
        tab = torch.randn((max(KS) - 1, ns), generator=g, device="cuda", dtype=torch.float64)
        tab[0] = 0.1 + 1.0e-5 * torch.linspace(-1.0, 1.0, ns, device="cuda", dtype=torch.float64)
        pix = torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int32)
        pix[torch.rand(n, generator=g, device="cuda") < 0.10] = -1
        v = torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
        out = D.empty(n)
        src = torch.zeros(n * BYTES_PER_SAMPLE // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        fns = {COPY: lambda: dst.copy_(src)}
        create, info, keep = {}, {}, []

        def add(name, F, entry, K):
            cf = D.empty(ndet * F.nchunks * K)
            keep.extend([F, cf])
            fns["apply, " + name] = lambda: _hip.call(entry + "_apply", F._handle.h, D.ptr(v), D.ptr(out), D.stream())
            fns["fit only, " + name] = lambda: _hip.call(entry + "_fit", F._handle.h, D.ptr(v), D.ptr(cf), D.stream())

        def timed(make):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            F = make()
            torch.cuda.synchronize()
            return F, 1e3 * (time.perf_counter() - t0)

        for K in KS:
            F, create["template K = %d" % K] = timed(lambda: TemplateFilterLO(tab[:K - 1], pix, ndet=ndet, chunks=chunk))
            info["template K = %d" % K] = F.filter_info()
            add("template K = %d" % K, F, "cm2_template", K)
        F, create["hwpss H = %d" % NHARM] = timed(lambda: HWPSSFilterLO(chi, pix, ndet=ndet, nharm=NHARM, chunks=chunk))
        info["hwpss H = %d" % NHARM] = F.filter_info()
        add("hwpss H = %d" % NHARM, F, "cm2_hwpss", 2 * NHARM + 1)
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
        r = res["shapes"]["ns %d x ndet %d, chunks of %d" % (ns, ndet, chunk)] = {
            "create_ms": {k: round(t, 3) for k, t in create.items()}, "info": info,
            "table_bytes": {"template K = %d" % K: round(8.0 * (K - 1) / det_tile(K), 2) for K in KS}, "calls": {}}
        copy_med = statistics.median(ms[COPY])
        for k, t in ms.items():
            med = statistics.median(t)
            r["calls"][k] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                             "ratio_to_copy": round(med / copy_med, 3),
                             "samples_per_s": round(n / (med * 1e-3), 1),
                             "GB_per_s_at_36_B": round(n * BYTES_PER_SAMPLE / (med * 1e-3) / 1e9, 1)}
        del fns, keep, F, chi, tab, pix, v, out, src, dst
        torch.cuda.empty_cache()
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def main():
    if "--step" in sys.argv:
        return step_gpu(sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "template_filter_timing.json")
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "gpu", out]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
