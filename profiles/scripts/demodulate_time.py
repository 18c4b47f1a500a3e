#!/usr/bin/env python3
"""
Time of the demodulator (cm2_demod_run) at 1e8 samples in 10 noise blocks, for D = 4, 8, 16, 64 with
the default taps (L = 16 D + 1), with and without a carrier: unit white noise plus a carrier of 0.13 cycles per sample,
3 % of the samples flagged at random (int32 flags) and nothing flagged (the same array without a negative entry: the
units then take W = Wfull).  Beside every figure, from the same run: a device copy that moves as many bytes as the
call reads and writes (a copy of n bytes reads n and writes n, so n is half the call's traffic),
and the same result composed from torch operations (mask, the two products, a strided fp64 conv1d per channel over the
blocks, the weight test and the divisions; where conv1d refuses fp64, unfold and a matrix-vector product).

    python profiles/scripts/demodulate_time.py [out.json]     # the GPU step under its own `timeout`
    python profiles/scripts/demodulate_time.py --step gpu out.json

One process; per setting 2 warm-up calls of every variant, then 10 rounds (3 for the torch composition) in which every
variant is called once (variants alternated), each timed by a host clock around the call and a device synchronise;
median, min, max in ms.  Also writes the summary table of profiles/demodulate.md to <out>.md.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NT, NBLOCKS = 100_000_000, 10
FACTORS = (4, 8, 16, 64)
WARMUP, ROUNDS, TORCH_ROUNDS = 2, 10, 3
MIN_WEIGHT = 0.5


def torch_composition(torch, d, pix, cosv, sinv, taps, D, wfull):
    """(T, Q, U, classes) of the definition from torch operations; the sums in whatever order conv1d adds them"""
    L = taps.numel()
    c = (L - 1) // 2
    use = (pix >= 0) & torch.isfinite(d)
    x = torch.where(use, d, torch.zeros_like(d))
    chans = [x] if cosv is None else [x, x * torch.where(use, cosv, torch.zeros_like(d)),
                                      x * torch.where(use, sinv, torch.zeros_like(d))]
    chans.append(use.to(torch.float64))

    def fir(v, w):
        v = v.view(NBLOCKS, 1, -1)
        try:
            return torch.nn.functional.conv1d(v, w.view(1, 1, L), stride=D, padding=c).reshape(-1), "conv1d"
        except RuntimeError:
            return (torch.nn.functional.pad(v, (c, c)).unfold(-1, L, D) @ w).reshape(-1), "unfold"
    sums, how = zip(*[fir(v, taps) for v in chans])
    W = sums[-1]
    ok = W >= MIN_WEIGHT * wfull
    safe = torch.where(ok, W, torch.ones_like(W))
    out = [torch.where(ok, s / safe, torch.zeros_like(s)) for s in sums[:-1]]
    included = fir(chans[-1], torch.ones_like(taps))[0]            # the count of included terms: the classes
    cls = torch.where(included == L, 0, torch.where(ok, 1, 2)).to(torch.uint8)
    if cosv is not None:
        out[1], out[2] = 2.0 * out[1], 2.0 * out[2]
    return out, cls, how[0]


def step_gpu(out_path):
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as Dv
    from cosmomap2_amd.utilities import Demodulator
    res = {"warmup": WARMUP, "rounds": ROUNDS, "torch_rounds": TORCH_ROUNDS, "device": torch.cuda.get_device_name(0),
           "nt": NT, "nblocks": NBLOCKS, "settings": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    ph = 2.0 * 3.141592653589793 * 0.13 * torch.arange(NT, device="cuda", dtype=torch.float64)
    cosv, sinv = torch.cos(ph), torch.sin(ph)
    del ph
    d = torch.randn(NT, generator=g, device="cuda", dtype=torch.float64) + 1.0 + 0.1 * cosv - 0.05 * sinv
    clean = torch.randint(0, 1000, (NT,), generator=g, device="cuda", dtype=torch.int32)
    flagged = clean.clone()
    flagged[torch.rand(NT, generator=g, device="cuda") < 0.03] = -1
    st = Dv.stream
    for D, (flags, pix) in ((D, f) for D in FACTORS for f in (("3 % at random", flagged), ("none", clean))):
        dm = Demodulator(NT // NBLOCKS, D)
        info = dm.info(NT)
        H = dm._handle(NT, None).h
        M, L = info["M"], info["ntaps"]
        taps = Dv.f64(dm.taps)
        T, Q, U = Dv.empty(M), Dv.empty(M), Dv.empty(M)
        cls, counts = Dv.empty(M, torch.uint8), Dv.empty(3 * NBLOCKS, torch.int64)
        for carrier in (True, False):
            co, si = (cosv, sinv) if carrier else (None, None)
            read = NT * (8 + 4 + (16 if carrier else 0))
            written = M * ((24 if carrier else 8) + 1)
            half = (read + written) // 2
            src, dst = Dv.empty(half, torch.uint8), Dv.empty(half, torch.uint8)
            fns = {
                "copy": lambda: dst.copy_(src),
                "cm2_demod_run": lambda: _hip.call("cm2_demod_run", H, Dv.ptr(d), Dv.ptr(co), Dv.ptr(si), Dv.ptr(pix), 0,
                                                   MIN_WEIGHT, Dv.ptr(T), Dv.ptr(Q if carrier else None),
                                                   Dv.ptr(U if carrier else None), Dv.ptr(cls), Dv.ptr(counts), st()),
                "torch": lambda: torch_composition(torch, d, pix, co, si, taps, D, dm.wfull),
            }
            o = {"factor": D, "ntaps": L, "carrier": carrier, "flagged": flags, "info": info, "bytes_read": read,
                 "bytes_written": written, "fp64_ops_per_input_sample": round(L / D * (7 if carrier else 3), 1), "calls": {}}
            try:
                ref, ref_cls, how = fns["torch"]()
                fns["cm2_demod_run"]()
                torch.cuda.synchronize()
                o["torch_route"] = how
                o["max_abs_difference"] = [float((a - b).abs().max()) for a, b in zip(ref, (T, Q, U) if carrier else (T,))]
                o["classes_equal"] = bool((ref_cls == cls).all())
                del ref, ref_cls
            except Exception as e:                                 # the composition is a yardstick: say why it is missing
                o["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
                del fns["torch"]
            torch.cuda.empty_cache()
            for _ in range(WARMUP):
                for fn in fns.values():
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in fns}
            for r in range(ROUNDS):
                for k, fn in fns.items():
                    if k == "torch" and r >= TORCH_ROUNDS:
                        continue
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ms[k].append(1e3 * (time.perf_counter() - t0))
            copy_med = statistics.median(ms["copy"])
            for k, v in ms.items():
                med = statistics.median(v)
                o["calls"][k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                                 "ratio_to_copy": round(med / copy_med, 3),
                                 "input_samples_per_s": round(NT / (med * 1e-3), 1)}
            med = o["calls"]["cm2_demod_run"]["median_ms"] * 1e-3
            o["TB_per_s"] = round((read + written) / med / 1e12, 3)
            o["fp64_Tops_per_s"] = round(NT * o["fp64_ops_per_input_sample"] / med / 1e12, 3)
            o["counts"] = Dv.to_host(counts).reshape(NBLOCKS, 3).sum(0).tolist()
            res["settings"].append(o)
            del src, dst, fns
            torch.cuda.empty_cache()
        del dm, T, Q, U, cls, counts
    json.dump(res, open(out_path, "w"), indent=1)
    lines = ["| D | L | carrier | flagged | `cm2_demod_run` ms: median (min–max) | copy of the same bytes, ms | × the copy | "
             "torch composition, ms | TB/s | fp64 Tops/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for o in res["settings"]:
        c = o["calls"]
        k = c["cm2_demod_run"]
        t = "%.1f (%s)" % (c["torch"]["median_ms"], o["torch_route"]) if "torch" in c else "failed"
        lines.append("| %d | %d | %s | %s | %.3f (%.3f–%.3f) | %.3f | %.2f | %s | %.2f | %.2f |" % (
            o["factor"], o["ntaps"], "yes" if o["carrier"] else "no", o["flagged"], k["median_ms"], k["min_ms"], k["max_ms"],
            c["copy"]["median_ms"], k["ratio_to_copy"], t, o["TB_per_s"], o["fp64_Tops_per_s"]))
    open(os.path.splitext(out_path)[0] + ".md", "w").write("\n".join(lines) + "\n")
    print(json.dumps(res))


def main():
    if "--step" in sys.argv:
        return step_gpu(sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "demodulate_timing.json")
    cmd = ["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--step", "gpu", out]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
