#!/usr/bin/env python3
"""
Time of expand_pointing (cm2_pointing_expand) at 1e8 detector samples: ns = 1e7 with 10 detectors and
ns = 1e8 with one, nside 256, RING and NESTED, with and without a plate angle; beside it a plain device copy of the
20 bytes per detector sample the kernel stores (20 B read and 20 B written), and the NumPy vec2pix of
healpix_fits.py on 1e6 directions on the host.

    python profiles/scripts/pointing_expand_time.py [out.json]     # both steps, each under its own `timeout`,
                                                                   # stopping at the first one that fails
    python profiles/scripts/pointing_expand_time.py --step gpu out.json
    python profiles/scripts/pointing_expand_time.py --step host out.json

step `gpu`:  one process; per shape 3 warm-up calls of every variant and of the copy, then 20 rounds in which every
             variant is called once (variants alternated), each timed by a host clock around the call and a device
             synchronise (the call itself waits once, for the check of the detector table); median, min, max in ms.
step `host`: vec2pix on 1e6 seeded unit vectors, median of 5.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NSIDE = 256
SHAPES = ((10_000_000, 10), (100_000_000, 1))
WARMUP, ROUNDS = 3, 20
BYTES_PER_SAMPLE = 20                       # int32 pixel, two doubles


def step_gpu(out_path):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import device as D
    from cosmomap2_amd.utilities import expand_pointing
    res = {"nside": NSIDE, "warmup": WARMUP, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for ns, ndet in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(ns + ndet)
        bore = torch.randn((ns, 4), generator=g, device="cuda", dtype=torch.float64)
        bore /= bore.norm(dim=1, keepdim=True)
        det = np.random.default_rng(ndet).standard_normal((ndet, 4))
        det = D.f64(det / np.sqrt((det * det).sum(axis=1))[:, None])
        chi = torch.arange(ns, device="cuda", dtype=torch.float64) * (2 * np.pi * 2.0 / 100.0)
        n = ns * ndet
        out = (D.empty(n, torch.int32), D.empty(n), D.empty(n))
        src = torch.zeros(n * BYTES_PER_SAMPLE, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        fns = {"copy of 20 B per detector sample": lambda: dst.copy_(src)}
        stored = {"copy of 20 B per detector sample": BYTES_PER_SAMPLE}      # bytes written per detector sample
        for nest in (False, True):
            for hwp in (None, chi):
                name = "%s, %s" % ("NESTED" if nest else "RING", "plate angle" if hwp is not None else "no plate")
                fns[name] = lambda nest=nest, hwp=hwp: expand_pointing(bore, det, NSIDE, nest=nest, hwp=hwp, out=out)
                stored[name] = BYTES_PER_SAMPLE
        fns["RING, pixels only (pol=1)"] = lambda: expand_pointing(bore, det, NSIDE, pol=1, out=(out[0], None, None))
        stored["RING, pixels only (pol=1)"] = 4
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
        r = res["shapes"]["ns %d x ndet %d" % (ns, ndet)] = {}
        for k, v in ms.items():
            med = statistics.median(v)
            r[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                    "detector_samples_per_s": round(n / (med * 1e-3), 1),
                    "stored_bytes_per_sample": stored[k],
                    "stored_GB_per_s": round(n * stored[k] / (med * 1e-3) / 1e9, 1)}
        del fns, bore, chi, out, src, dst
        torch.cuda.empty_cache()
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def step_host(out_path):
    import numpy as np
    from cosmomap2_amd.utilities.healpix_fits import vec2pix
    v = np.random.default_rng(5).standard_normal((3, 1_000_000))
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        vec2pix(NSIDE, v[0], v[1], v[2])
        times.append(time.perf_counter() - t0)
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    med = statistics.median(times)
    res["host_numpy_vec2pix"] = {"directions": v.shape[1], "median_s": round(med, 4),
                                 "directions_per_s": round(v.shape[1] / med, 1),
                                 "scaled_to_1e8_s": round(med * 100, 2)}
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res["host_numpy_vec2pix"]))


def main():
    if "--step" in sys.argv:
        step = sys.argv[sys.argv.index("--step") + 1]
        return step_gpu(sys.argv[-1]) if step == "gpu" else step_host(sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pointing_expand_timing.json")
    me = os.path.abspath(__file__)
    for cmd in (["timeout", "-k", "10", "400", sys.executable, me, "--step", "gpu", out],
                ["timeout", "-k", "10", "120", sys.executable, me, "--step", "host", out]):
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            print("step failed with status %d, stopping: %s" % (rc, " ".join(cmd)), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
