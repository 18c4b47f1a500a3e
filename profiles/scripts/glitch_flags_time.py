#!/usr/bin/env python3
"""
Time of the glitch flagger (cm2_glitch_residual, cm2_glitch_scale, cm2_glitch_classify) at 1e8 samples
in 10 noise blocks, for half-widths h = 8, 16, 32, 48, 64 (one per tier): unit white noise plus a slow drift, 3 % of the
samples flagged at random (int32 flags), 1000 glitches of +-20.  Beside the three calls one whole pass (residual, scale,
classify and the read-back of the counts, as GlitchFlagger.flag(iterations=1) runs it) and a device copy of nt doubles,
the yardstick of profiles/pointing_expand.md.

    python profiles/scripts/glitch_flags_time.py [out.json]     # the GPU step under its own `timeout`
    python profiles/scripts/glitch_flags_time.py --step gpu out.json

One process; per half-width 2 warm-up calls of every variant and of the copy, then 10 rounds in which every variant is
called once (variants alternated), each timed by a host clock around the call and a device synchronise; median, min,
max in ms.  Also writes the summary table of profiles/glitch_flags.md to <out>.md.
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
HALF_WIDTHS = (8, 16, 32, 48, 64)
WARMUP, ROUNDS = 2, 10
COPY = "copy of nt doubles"
RUN = 64                                    # kRun of cm2_glitch_policy.h
TIER_SLOTS = {8: 17, 16: 33, 32: 65, 48: 97, 64: 129}


def step_gpu(out_path):
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.utilities import GlitchFlagger
    res = {"warmup": WARMUP, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "nt": NT, "nblocks": NBLOCKS,
           "half_widths": {}}
    g = torch.Generator(device="cuda").manual_seed(1)
    d = torch.randn(NT, generator=g, device="cuda", dtype=torch.float64)
    d += 3.0 * torch.sin(torch.arange(NT, device="cuda", dtype=torch.float64) * (2.0 * 3.141592653589793 / 4000.0))
    where = torch.randint(0, NT, (1000,), generator=g, device="cuda")
    d[where] += 20.0 * (2.0 * torch.randint(0, 2, (1000,), generator=g, device="cuda").to(torch.float64) - 1.0)
    pix = torch.randint(0, 1000, (NT,), generator=g, device="cuda", dtype=torch.int32)
    pix[torch.rand(NT, generator=g, device="cuda") < 0.03] = -1
    r, dst = D.empty(NT), D.empty(NT)
    cls = D.empty(NT, torch.uint8)
    counts = D.empty(NBLOCKS * 5, torch.int64)
    st = D.stream
    for h in HALF_WIDTHS:
        gf = GlitchFlagger(NT // NBLOCKS, half_width=h)
        info = gf.info(NT)
        H = gf._handle(NT, None).h
        sigma = gf.scale(d, gf.residual(d, flags=pix), flags=pix)
        fns = {
            COPY: lambda: dst.copy_(d),
            "residual": lambda: _hip.call("cm2_glitch_residual", H, D.ptr(d), D.ptr(pix), 0, None, D.ptr(r), st()),
            "scale": lambda: _hip.call("cm2_glitch_scale", H, D.ptr(d), D.ptr(r), D.ptr(pix), 0, None, D.ptr(sigma),
                                       st()),
            "classify": lambda: _hip.call("cm2_glitch_classify", H, D.ptr(d), D.ptr(r), D.ptr(pix), 0, None,
                                          D.ptr(sigma), 5.0, 2, D.ptr(cls), D.ptr(counts), st()),
            "one whole pass": lambda: gf.flag(d, flags=pix, nsigma=5.0, grow=2, iterations=1),
        }
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
        copy_med = statistics.median(ms[COPY])
        out = res["half_widths"][str(h)] = {"info": info, "sigma": [float(s) for s in D.to_host(sigma)],
                                            "hits": int(D.to_host(counts).reshape(NBLOCKS, 5)[:, 3].sum()),
                                            "calls": {}}
        for k, t in ms.items():
            med = statistics.median(t)
            out["calls"][k] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                               "ratio_to_copy": round(med / copy_med, 3),
                               "samples_per_s": round(NT / (med * 1e-3), 1)}
        # the rates the arithmetic of DESIGN 8.10 is held against
        W, slots = 2 * h + 1, TIER_SLOTS[h]
        visits = slots * (1.0 + W / RUN)                   # slot visits per output
        in_lds = max(W - 96, 0) * (1.0 + W / RUN) if h > 48 else 0.0           # of them in LDS, 16 B each
        med = out["calls"]["residual"]["median_ms"] * 1e-3
        out["residual_rates"] = {"slot_visits_per_output": round(visits, 1),
                                 "slot_visits_per_s": round(NT * visits / med, 1),
                                 "lds_TB_per_s": round(NT * in_lds * 16 / med / 1e12, 2),
                                 "hbm_GB_per_s_at_20_B": round(NT * 20 / med / 1e9, 1)}
        med = out["calls"]["scale"]["median_ms"] * 1e-3
        out["scale_rates"] = {"hbm_GB_per_s_at_6_x_12_B": round(NT * 72 / med / 1e9, 1)}
        med = out["calls"]["classify"]["median_ms"] * 1e-3
        out["classify_rates"] = {"hbm_GB_per_s_at_21_B": round(NT * 21 / med / 1e9, 1)}
        del gf, fns
        torch.cuda.empty_cache()
    json.dump(res, open(out_path, "w"), indent=1)
    lines = ["| h (tier) | call | ms per call: median (min–max) | × the copy |", "|---|---|---|---|"]
    for h, o in res["half_widths"].items():
        for k, c in o["calls"].items():
            lines.append("| %s (%d) | %s | %.3f (%.3f–%.3f) | %.2f |" % (h, o["info"]["tier"], k, c["median_ms"],
                                                                        c["min_ms"], c["max_ms"], c["ratio_to_copy"]))
    open(os.path.splitext(out_path)[0] + ".md", "w").write("\n".join(lines) + "\n")
    print(json.dumps(res))


def main():
    if "--step" in sys.argv:
        return step_gpu(sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "glitch_flags_timing.json")
    cmd = ["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--step", "gpu", out]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
