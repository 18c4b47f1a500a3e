#!/usr/bin/env python3
"""
The ground-bin sums G^T v at 1e8 samples ("Reproducible ground-bin sums"): the default route
(cm2_ground_bin_sums, racing fp64 atomics) against the order-independent integer sums (cm2_ground_sums_apply) on the
LDS route (1) and the global route (2) at 2000 bins, and the default's pixel-major P^T fall-back against route 2 at
9000 bins.  The labels are a triangle wave over the bins, as an azimuth scan makes them.

    python profiles/scripts/ground_exact_timing.py [out.json]      # both steps, each under its own `timeout`,
                                                                   # stopping at the first one that fails
    python profiles/scripts/ground_exact_timing.py --step time out.json
    python profiles/scripts/ground_exact_timing.py --step trace

step `time`:   one process; per bin count 5 warm-up calls of every variant, then 20 rounds in which every variant is
               called once between two HIP events of its own (variants alternated); median, min and max in ms.
step `trace`:  `rocprofv3 --kernel-trace --stats` around 10 calls of each route at 2000 bins (no counters in that
               run): the split of one call over its kernels, read from the stats file into the JSON.
"""
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NT = 100_000_000
WARMUP, ROUNDS = 5, 20


def inputs(torch, nbins):
    t = torch.arange(NT, device="cuda", dtype=torch.int64)
    az = ((t % (2 * (nbins - 1))) - (nbins - 1)).abs().to(torch.int32)
    del t
    g = torch.Generator(device="cuda").manual_seed(nbins)
    return az, torch.randn(NT, generator=g, device="cuda", dtype=torch.float64)


def variants(nbins, az, v):
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import GroundFilterLO
    from cosmomap2_amd.interfaces import linearoperators as L
    h = L._GroundSums(nbins)
    sums = D.empty(nbins)
    out = {}
    if nbins <= GroundFilterLO.LDS_BINS:
        out["default cm2_ground_bin_sums"] = lambda: _hip.call("cm2_ground_bin_sums", NT, nbins, D.ptr(az), D.ptr(v),
                                                               D.ptr(sums), D.stream())
    else:
        Fg = GroundFilterLO(az)
        out["default P^T fall-back"] = lambda: Fg._bin_sums(v)
    for route in ((1, 2) if nbins <= h.info()["lds_bins"] else (2,)):
        out["exact route %d" % route] = lambda route=route: _hip.call(
            "cm2_ground_sums_apply", h.h, NT, D.ptr(az), D.ptr(v), route, D.ptr(sums), D.stream())
    return out, h


def step_time(out_path):
    import torch
    torch.cuda.set_device(0)
    res = {"nt": NT, "warmup": WARMUP, "rounds": ROUNDS, "bins": {}}
    for nbins in (2000, 9000):
        az, v = inputs(torch, nbins)
        fns, keep = variants(nbins, az, v)
        for _ in range(WARMUP):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        events = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                events[k].append((e0, e1))
        torch.cuda.synchronize()
        r = res["bins"][str(nbins)] = {}
        for k, ev in events.items():
            ms = [a.elapsed_time(b) for a, b in ev]
            r[k] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                    "max_ms": round(max(ms), 4)}
        del fns, keep, az, v
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def step_trace():
    import torch
    torch.cuda.set_device(0)
    az, v = inputs(torch, 2000)
    fns, keep = variants(2000, az, v)
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()


def kernel_stats(trace_dir):
    """{kernel: {calls, mean_us}} of the binning kernels from rocprofv3's kernel_stats.csv"""
    import csv
    rows = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Name", "").replace("(anonymous namespace)::", "").replace("cm2::", "")
            if name.startswith(("k_gsum_", "k_ground_bin")):
                rows[name.split("(")[0]] = {"calls": int(r.get("Calls", 0)),
                                            "mean_us": round(float(r.get("AverageNs", 0)) / 1e3, 1)}
    return rows


def main():
    if "--step" in sys.argv:
        step = sys.argv[sys.argv.index("--step") + 1]
        return step_time(sys.argv[-1]) if step == "time" else step_trace()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ground_exact_timing.json")
    trace_dir = os.path.splitext(out)[0] + "_trace"
    me = os.path.abspath(__file__)
    steps = [["timeout", "-k", "10", "300", sys.executable, me, "--step", "time", out],
             ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir,
              "--output-format", "csv", "--", sys.executable, me, "--step", "trace"]]
    for cmd in steps:
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            print("step failed with status %d, stopping: %s" % (rc, " ".join(cmd)), file=sys.stderr)
            return rc
    res = json.load(open(out))
    res["rocprofv3_kernel_stats_of_10_calls_per_route_at_2000_bins"] = kernel_stats(trace_dir)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["rocprofv3_kernel_stats_of_10_calls_per_route_at_2000_bins"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
