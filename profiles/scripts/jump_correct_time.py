#!/usr/bin/env python3
"""
Time of the jump corrector (cm2_jump_stat, cm2_jump_scale, cm2_jump_find, cm2_jump_correct) at 1e8
samples in 10 noise blocks, for half-windows w = 16, 64, 256: unit white noise, 3 % of the samples flagged at random
(int32 flags), 60 steps of +-3 .. 20 at random positions.  Beside the four calls one whole pass (stat, scale, find,
correct and the read-backs, as JumpCorrector.run(iterations=1) runs it) and a device copy of nt doubles, the yardstick
of profiles/glitch_flags.md.

    python profiles/scripts/jump_correct_time.py [out.json]     # the GPU step under its own `timeout`
    python profiles/scripts/jump_correct_time.py --step gpu out.json

One process; per half-window 2 warm-up calls of every variant and of the copy, then 10 rounds in which every variant is
called once (variants alternated), each timed by a host clock around the call and a device synchronise; median, min,
max in ms.  Also writes the summary table of profiles/jump_correct.md to <out>.md.
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
HALF_WINDOWS = (16, 64, 256)
WARMUP, ROUNDS = 2, 10
COPY = "copy of nt doubles"
CAPACITY = 1 << 20
LDS_PEAK = 79e12                            # bytes per second, the figure of profiles/glitch_flags.md


def step_gpu(out_path):
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.utilities import JumpCorrector
    res = {"warmup": WARMUP, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "nt": NT, "nblocks": NBLOCKS,
           "half_windows": {}}
    g = torch.Generator(device="cuda").manual_seed(1)
    d = torch.randn(NT, generator=g, device="cuda", dtype=torch.float64)
    where = torch.randint(1000, NT // NBLOCKS - 1000, (60,), generator=g, device="cuda") + \
        (NT // NBLOCKS) * torch.arange(60, device="cuda").remainder(NBLOCKS)
    heights = (3.0 + 17.0 * torch.rand(60, generator=g, device="cuda", dtype=torch.float64)) * \
        (2.0 * torch.randint(0, 2, (60,), generator=g, device="cuda").to(torch.float64) - 1.0)
    for p, h in zip(where.tolist(), heights.tolist()):
        d[p:(p // (NT // NBLOCKS) + 1) * (NT // NBLOCKS)] += h
    pix = torch.randint(0, 1000, (NT,), generator=g, device="cuda", dtype=torch.int32)
    pix[torch.rand(NT, generator=g, device="cuda") < 0.03] = -1
    t, dst, out = D.empty(NT), D.empty(NT), D.empty(NT)
    noeval, cls = D.empty(NT, torch.uint8), D.empty(NT, torch.uint8)
    pos, hgt, off = D.empty(CAPACITY, torch.int64), D.empty(CAPACITY), D.empty(CAPACITY)
    nj, counts = D.empty(NBLOCKS + 1, torch.int64), D.empty(NBLOCKS * 3, torch.int64)
    sigma = D.empty(NBLOCKS)
    st = D.stream
    for w in HALF_WINDOWS:
        jc = JumpCorrector(NT // NBLOCKS, half_window=w)
        info = jc.info(NT)
        H = jc._handle(NT, None).h
        mc = (w + 1) // 2
        fns = {
            COPY: lambda: dst.copy_(d),
            "stat": lambda: _hip.call("cm2_jump_stat", H, D.ptr(d), D.ptr(pix), 0, None, mc, D.ptr(t), D.ptr(noeval),
                                      st()),
            "scale": lambda: _hip.call("cm2_jump_scale", H, D.ptr(t), D.ptr(noeval), D.ptr(sigma), st()),
            "find": lambda: _hip.call("cm2_jump_find", H, D.ptr(t), D.ptr(noeval), D.ptr(sigma), 6.0, CAPACITY,
                                      D.ptr(pos), D.ptr(hgt), D.ptr(off), D.ptr(nj), st()),
            "correct": lambda: _hip.call("cm2_jump_correct", H, D.ptr(d), None, D.ptr(pos), D.ptr(off), D.ptr(nj),
                                         CAPACITY, 4, D.ptr(out), D.ptr(cls), D.ptr(counts), st()),
            "one whole pass": lambda: jc.run(d, flags=pix, nsigma=6.0, radius=4, iterations=1),
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
        found = D.to_host(nj)
        o = res["half_windows"][str(w)] = {"info": info, "sigma": [float(s) for s in D.to_host(sigma)],
                                           "jumps_found": int(found[-1]), "jumps_injected": 60, "calls": {}}
        for k, v in ms.items():
            med = statistics.median(v)
            o["calls"][k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                             "ratio_to_copy": round(med / copy_med, 3), "samples_per_s": round(NT / (med * 1e-3), 1)}
        # the two floors of k_jump_stat that DESIGN 8.11 holds it against
        med = o["calls"]["stat"]["median_ms"] * 1e-3
        hbm_floor = 22.0 / 16.0 * copy_med * 1e-3          # 13 B read, 9 B written per sample at the copy's rate
        lds_floor = NT * w * 8 / LDS_PEAK
        o["stat_rates"] = {"hbm_floor_ms": round(1e3 * hbm_floor, 3), "lds_floor_ms": round(1e3 * lds_floor, 3),
                           "ratio_to_larger_floor": round(med / max(hbm_floor, lds_floor), 2),
                           "lds_TB_per_s": round(NT * w * 8 / med / 1e12, 2),
                           "additions_per_s": round(NT * w / med, 1)}
        del jc, fns
        torch.cuda.empty_cache()
    json.dump(res, open(out_path, "w"), indent=1)
    lines = ["| w | call | ms per call: median (min–max) | × the copy |", "|---|---|---|---|"]
    for w, o in res["half_windows"].items():
        for k, c in o["calls"].items():
            lines.append("| %s | %s | %.3f (%.3f–%.3f) | %.2f |" % (w, k, c["median_ms"], c["min_ms"], c["max_ms"],
                                                                   c["ratio_to_copy"]))
    open(os.path.splitext(out_path)[0] + ".md", "w").write("\n".join(lines) + "\n")
    print(json.dumps(res))


def main():
    if "--step" in sys.argv:
        return step_gpu(sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "jump_correct_timing.json")
    cmd = ["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--step", "gpu", out]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
