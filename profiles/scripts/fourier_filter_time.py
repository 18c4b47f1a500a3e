#!/usr/bin/env python3
"""
Time of the Fourier filter (cm2_fourier_apply) at 1e8 samples, as 10 noise blocks of 1e7 and as 100 of
1e6, for (a) deconvolution of a time constant of 5 samples with a 4th-order low-pass at 0.2 fs and (b) a real 2nd-order
high-pass at 1e-4 fs; detrend "ends", pad 1024.  Beside every figure, from the same process: a device copy of 16 B per
sample (8 read, 8 written: what a filter must move at the least), and the same result composed from torch operations:
subtract the line, pad, torch.fft.rfft over [nblocks, L], multiply by a precomputed H, irfft, slice, add H(0) line.

    python profiles/scripts/fourier_filter_time.py [out.json]     # each GPU step under its own `timeout`
    python profiles/scripts/fourier_filter_time.py --step gpu out.json
    python profiles/scripts/fourier_filter_time.py --step once out.json     # two calls per setting, for a kernel trace

Per setting 1 warm-up call of every variant, then 5 rounds in which every variant is called once (variants
alternated), each timed by a host clock around the call and a device synchronise; median, min, max in ms.  The
per-kernel split comes from one `rocprofv3 --kernel-trace --stats` run of `--step once`, a run of its own.  Writes
the tables of profiles/fourier_filter.md to <out>.md.
"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NT = 100_000_000
LAYOUTS = (10, 100)
FS = 100.0
FILTERS = {"deconvolve + low-pass": dict(tau=5.0 / FS, lowpass=(0.2 * FS, 4)),
           "high-pass (real H)": dict(highpass=(1e-4 * FS, 2))}
WARMUP, ROUNDS = 1, 5
END_MEAN, PAD = 32, 1024


def torch_composition(torch, x, nb, n, L, H):
    v = x.view(nb, n)
    a, b = v[:, :END_MEAN].mean(1, keepdim=True), v[:, -END_MEAN:].mean(1, keepdim=True)
    line = a + (b - a) * (torch.arange(n, device=x.device, dtype=torch.float64) / (n - 1))
    rows = torch.nn.functional.pad(v - line, (0, L - n))
    y = torch.fft.irfft(torch.fft.rfft(rows, dim=1) * H, n=L, dim=1)
    return (y[:, :n] + H[0].real * line).reshape(-1)


def make(nb, kw, work):
    from cosmomap2_amd.utilities import FourierFilter
    return FourierFilter(NT // nb, FS, detrend="ends", end_mean=END_MEAN, pad=PAD, max_work_bytes=work, **kw)


def settings(torch):
    """(layout, filter name, FourierFilter, handle, info) with the default work cap, or 4 GB where a row needs more"""
    from cosmomap2_amd import _hip
    for nb in LAYOUTS:
        for name, kw in FILTERS.items():
            ff, work = make(nb, kw, None), 512 << 20
            try:
                info = ff.info(NT)
            except _hip.HipError as e:
                if e.status != _hip.ERR_ARGUMENT:
                    raise
                ff, work = make(nb, kw, 4 << 30), 4 << 30
                info = ff.info(NT)
            yield nb, name, ff, ff._handle(NT, None).h, info, work


def step_once(_):
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as Dv
    x = torch.randn(NT, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda", dtype=torch.float64)
    out = Dv.empty(NT)
    for nb, name, ff, h, info, work in settings(torch):
        for _ in range(2):
            _hip.call("cm2_fourier_apply", h, Dv.ptr(x), Dv.ptr(out), Dv.stream())
        torch.cuda.synchronize()
        del ff
    print("once: done")


def step_gpu(out_path):
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as Dv
    res = {"warmup": WARMUP, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "nt": NT, "settings": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.cumsum(torch.randn(NT, generator=g, device="cuda", dtype=torch.float64), 0) * 1e-3 + \
        torch.randn(NT, generator=g, device="cuda", dtype=torch.float64)
    out, src, dst = Dv.empty(NT), Dv.empty(NT), Dv.empty(NT)
    for nb, name, ff, h, info, work in settings(torch):
        n, L = NT // nb, info["lengths"][0]
        H = torch.from_numpy(ff.response(0, NT)).to("cuda")   # one tau for all blocks: one row of H serves them all
        fns = {
            "copy": lambda: dst.copy_(src),
            "cm2_fourier_apply": lambda: _hip.call("cm2_fourier_apply", h, Dv.ptr(x), Dv.ptr(out), Dv.stream()),
            "torch": lambda: torch_composition(torch, x, nb, n, L, H),
        }
        o = {"nblocks": nb, "n": n, "L": L, "filter": name, "info": info, "max_work_bytes": work, "calls": {}}
        try:
            ref = fns["torch"]()
            fns["cm2_fourier_apply"]()
            torch.cuda.synchronize()
            o["max_abs_difference"] = float((ref - out).abs().max())
            o["max_abs_output"] = float(out.abs().max())
            del ref
        except Exception as e:                                 # the composition is a yardstick: say why it is missing
            o["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            del fns["torch"]
        torch.cuda.empty_cache()
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
        copy_med = statistics.median(ms["copy"])
        for k, v in ms.items():
            med = statistics.median(v)
            o["calls"][k] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                             "ratio_to_copy": round(med / copy_med, 2), "samples_per_s": round(NT / (med * 1e-3), 1)}
        res["settings"].append(o)
        del fns, H, ff
        torch.cuda.empty_cache()
    json.dump(res, open(out_path, "w"), indent=1)
    lines = ["| blocks | n | L | rows a batch | filter | `cm2_fourier_apply` ms: median (min–max) | copy of 16 B/sample, ms | "
             "× the copy | torch composition ms: median (min–max) | call / composition | max abs difference |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for o in res["settings"]:
        c = o["calls"]
        k = c["cm2_fourier_apply"]
        if "torch" in c:
            t = "%.2f (%.2f–%.2f)" % (c["torch"]["median_ms"], c["torch"]["min_ms"], c["torch"]["max_ms"])
            r = "%.2f" % (k["median_ms"] / c["torch"]["median_ms"])
        else:
            t, r = "failed", "-"
        lines.append("| %d | %d | %d | %d | %s | %.2f (%.2f–%.2f) | %.2f | %.2f | %s | %s | %.2g |" % (
            o["nblocks"], o["n"], o["L"], o["info"]["batches"][0], o["filter"], k["median_ms"], k["min_ms"], k["max_ms"],
            c["copy"]["median_ms"], k["ratio_to_copy"], t, r, o.get("max_abs_difference", float("nan"))))
    open(os.path.splitext(out_path)[0] + ".md", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def kernel_split(trace_dir, out_path):
    """the per-kernel table of the trace run: every kernel with 0.5 % or more of the time"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    if not rows:
        return "no kernel statistics were written under %s" % trace_dir
    lines = ["| kernel | calls | total ms | average ms | % |", "|---|---|---|---|---|"]
    for r in sorted(rows, key=lambda r: -float(r.get("TotalDurationNs", 0))):
        if float(r.get("Percentage", 0)) >= 0.5:
            lines.append("| `%s` | %s | %.2f | %.3f | %.1f |" % (
                r.get("Name", "?")[:90], r.get("Calls", "?"), float(r.get("TotalDurationNs", 0)) / 1e6,
                float(r.get("AverageNs", 0)) / 1e6, float(r.get("Percentage", 0))))
    open(os.path.splitext(out_path)[0] + "_kernels.md", "w").write("\n".join(lines) + "\n")
    return "\n".join(lines)


def main():
    if "--step" in sys.argv:
        return {"gpu": step_gpu, "once": step_once}[sys.argv[sys.argv.index("--step") + 1]](sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fourier_filter_timing.json")
    me = os.path.abspath(__file__)
    cmd = ["timeout", "-k", "10", "420", sys.executable, me, "--step", "gpu", out]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
        return rc
    trace_dir = os.path.splitext(out)[0] + "_trace"
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d",
           trace_dir, "--", sys.executable, me, "--step", "once", out]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
        return rc
    print(kernel_split(trace_dir, out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
