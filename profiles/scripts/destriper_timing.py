#!/usr/bin/env python3
"""
The destriper's normal operator at C4 size: nside 256, IQU, 1e8 samples, 100 blocks, 10 % of
the samples flagged in runs of 500 every 5000, baseline_length 100 and 10000.

    python profiles/scripts/destriper_timing.py [out.json]       # every step below, each under its own `timeout`,
                                                                 # stopping at the first one that fails
    python profiles/scripts/destriper_timing.py --step time out.json     # one step, in this process
    python profiles/scripts/destriper_timing.py --step trace             # the kernels of 10 applications, for rocprofv3

step `time`:   per baseline length: one A application against the plain P.T*N*P of the same pointing (C4's Toeplitz
               band), alternated 5 times in one process (20 applications each per turn); the two window kernels
               against the plan's plain windowed permutations, alternated likewise; the stages of the chain alone; the
               iteration count of solve_destriped at rtol = 1e-6.
step `trace`:  `rocprofv3 --kernel-trace --stats` around 10 applications per baseline length (no counters in that
               run); the per-kernel split is read from the stats file into the JSON.
"""
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
RUN, EVERY = 500, 5000
LENGTHS = (100, 10000)


def setup():
    import torch
    import bench
    from cosmomap2_amd.interfaces import SparseLO, BlockLO, BlockDiagonalPreconditionerLO
    from cosmomap2_amd.interfaces import linearoperators as L
    from cosmomap2_amd.utilities import ProcessTimeSamples
    cfg = bench.CONFIGS["c4"]
    nt, nb, lam, npix = cfg["nt"], cfg["nb"], cfg["lam"], 12 * cfg["nside"] ** 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    inp = bench.synth_inputs(torch, dev, npix, nt, nb, lam, rank=0)
    pix = inp["pix"]
    pix[(torch.arange(nt, device=dev) % EVERY) < RUN] = -1
    N = BlockLO(nt // nb, inp["bands"], offdiag=True, method=3)
    ces = ProcessTimeSamples(pix, npix, pol=3, phi=inp.pop("phi"))
    n = ces.get_new_pixel[0]
    P = SparseLO(n, nt, pix, pol=3, angle_processed=ces)
    Mbd = BlockDiagonalPreconditionerLO(ces, n, pol=3)
    L.set_pointing_mode("tiled")
    return dict(torch=torch, nt=nt, nb=nb, P=P, N=N, Mbd=Mbd, d=inp["d"], A=P.T * N * P)


def ms(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def step_time(out_path):
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import OffsetsLO, DestriperNormalLO, solve_destriped
    s = setup()
    torch, A, P = s["torch"], s["A"], s["P"]
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand(A.shape[0], generator=g, device="cuda", dtype=torch.float64)
    res = {"nt": s["nt"], "nmap": int(A.shape[0]), "baseline_lengths": {}}
    for Lb in LENGTHS:
        F = OffsetsLO(P, s["nt"] // s["nb"], Lb)
        op = DestriperNormalLO(P, F, s["Mbd"])
        a = torch.rand(F.na, generator=g, device="cuda", dtype=torch.float64)
        for _ in range(20):
            op * a
            A * x
        torch.cuda.synchronize()
        r = {"na": F.na, "empty_baselines": int((F.nvalid == 0).sum()), "A_ms": [], "plain_PtNP_ms": []}
        for _ in range(5):
            r["A_ms"].append(round(ms(torch, lambda: op * a, 20), 4))
            r["plain_PtNP_ms"].append(round(ms(torch, lambda: A * x, 20), 4))
        T = op._tiles()
        tb, st, ptr, h = op._tb, D.stream, D.ptr, F._f.h
        t1, out = D.empty(s["nt"]), D.empty(F.na)
        m1, m2 = op._m1, op._m2
        call = _hip.call
        stages = {
            "k_offsets_to_tiles": lambda: call("cm2_offsets_to_tiles", h, T.h, ptr(a), 1, ptr(tb), st()),
            "k_perm_windows<false>": lambda: call("cm2_tod_time_to_tiles", T.h, ptr(t1), ptr(tb), st()),
            "k_Pt_tiles_fixed": lambda: call("cm2_Pt_tiles_apply", T.h, ptr(tb), ptr(m1), st()),
            "k_bdprecond": lambda: op._precond_map(m1, m2),
            "k_P_tiles": lambda: call("cm2_P_tiles_apply", T.h, ptr(m2), ptr(tb), st()),
            "k_offsets_from_tiles": lambda: call("cm2_offsets_from_tiles", h, T.h, ptr(tb), 1, ptr(out), st()),
            "k_perm_windows<true>": lambda: call("cm2_tod_tiles_to_time", T.h, ptr(tb), ptr(t1), st()),
            "k_offsets_sum": lambda: call("cm2_offsets_sum", h, ptr(t1), 1, ptr(out), st()),
            "k_offsets_expand": lambda: call("cm2_offsets_expand", h, ptr(a), 1, ptr(t1), st()),
        }
        for fn in stages.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        r["stages_alone_ms"] = {k: [] for k in stages}
        for _ in range(5):
            for k, fn in stages.items():
                r["stages_alone_ms"][k].append(round(ms(torch, fn, 20), 4))
        chain = ("k_offsets_to_tiles", "k_Pt_tiles_fixed", "k_bdprecond", "k_P_tiles", "k_offsets_from_tiles")
        r["sum_of_stages_ms"] = round(sum(min(r["stages_alone_ms"][k]) for k in chain), 4)
        m, aa, info, sop = solve_destriped(P, s["nt"] // s["nb"], Lb, s["d"], s["Mbd"], rtol=1e-6)
        r["solve_destriped"] = {"iterations": sop.iterations, "info": info}
        res["baseline_lengths"][str(Lb)] = r
        del op, F, sop, m, aa, t1
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def step_trace():
    from cosmomap2_amd.interfaces import OffsetsLO, DestriperNormalLO
    s = setup()
    torch, P = s["torch"], s["P"]
    for Lb in LENGTHS:
        F = OffsetsLO(P, s["nt"] // s["nb"], Lb)
        op = DestriperNormalLO(P, F, s["Mbd"])
        a = torch.rand(F.na, device="cuda", dtype=torch.float64)
        for _ in range(10):
            op * a
        torch.cuda.synchronize()


def kernel_stats(trace_dir):
    """{kernel: {calls, mean_us}} of the chain's kernels from rocprofv3's kernel_stats.csv (both baseline lengths
    together: 20 applications)."""
    import csv
    rows = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Name", "")
            if any(k in name for k in ("k_offsets_", "k_P_tiles", "k_Pt_tiles", "k_parts_combine", "k_bdprecond")):
                rows[name.split("(")[0][-60:]] = {"calls": int(r.get("Calls", 0)),
                                                  "mean_us": round(float(r.get("AverageNs", 0)) / 1e3, 1)}
    return rows


def main():
    if "--step" in sys.argv:
        step = sys.argv[sys.argv.index("--step") + 1]
        return step_time(sys.argv[-1]) if step == "time" else step_trace()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "destriper_timing.json")
    trace_dir = os.path.splitext(out)[0] + "_trace"
    me = os.path.abspath(__file__)
    steps = [["timeout", "-k", "10", "420", sys.executable, me, "--step", "time", out],
             ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir,
              "--output-format", "csv", "--", sys.executable, me, "--step", "trace"]]
    for cmd in steps:
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            print("step failed with status %d, stopping: %s" % (rc, " ".join(cmd)), file=sys.stderr)
            return rc
    res = json.load(open(out))
    res["rocprofv3_kernel_stats_of_20_applications"] = kernel_stats(trace_dir)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["rocprofv3_kernel_stats_of_20_applications"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
