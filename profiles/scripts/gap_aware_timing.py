#!/usr/bin/env python3
"""
The gap-aware normal operator at C4 size: nside 256, IQU, 1e8 samples, 100 blocks,
lambda = 2048, 10 % of the samples flagged in runs of 500 every 5000.

    python profiles/scripts/gap_aware_timing.py [out.json]       # every step below, each under its own `timeout`,
                                                                 # stopping at the first one that fails
    python profiles/scripts/gap_aware_timing.py --step time out.json     # one step, in this process
    python profiles/scripts/gap_aware_timing.py --step trace             # the kernels of 10 applications, for rocprofv3

step `time`:   one A_e application against the plain P.T*N*P of the same pointing, alternated 5 times in one process
               (20 applications each per turn); the two new permutation kernels against the plan's plain windowed
               permutations, alternated likewise; the stages of the chain alone; the iteration counts of
               solve_gls_with_gaps and of the plain solve at rtol = 1e-6.
step `trace`:  `rocprofv3 --kernel-trace --stats` around 10 applications (no counters in that run); the per-kernel
               split is read from the stats file into the JSON.
"""
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
RUN, EVERY = 500, 5000


def setup():
    import numpy as np                                               # noqa: F401
    import torch
    import bench
    from cosmomap2_amd.interfaces import (SparseLO, BlockLO, BlockDiagonalPreconditionerLO, GapAwareNormalLO)
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
    return dict(torch=torch, L=L, nt=nt, P=P, N=N, Mbd=Mbd, d=inp["d"], A=P.T * N * P, op=GapAwareNormalLO(P, N))


def ms(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def step_time(out_path):
    from cosmomap2_amd import _hip, cg, device as D
    from cosmomap2_amd.interfaces import solve_gls_with_gaps
    s = setup()
    torch, op, A, P, N = s["torch"], s["op"], s["A"], s["P"], s["N"]
    g = torch.Generator(device="cuda").manual_seed(7)
    z = torch.rand(op.nmap + op.ng, generator=g, device="cuda", dtype=torch.float64)
    x = z[:op.nmap].clone()
    for _ in range(20):
        op * z
        A * x
    torch.cuda.synchronize()
    res = {"nt": s["nt"], "ng": op.ng, "nmap": op.nmap, "A_e_ms": [], "plain_PtNP_ms": []}
    for _ in range(5):
        res["A_e_ms"].append(round(ms(torch, lambda: op * z, 20), 4))
        res["plain_PtNP_ms"].append(round(ms(torch, lambda: A * x, 20), 4))
    # the stages alone, and the new kernels against the plain windowed permutations of the same plan
    T = op._tiles()
    t1, t2 = op._time_scratch()
    tb, st, ptr, gh = op._tb, D.stream, D.ptr, op._gaps.h
    comp = z[op.nmap:]
    call = _hip.call
    stages = {
        "k_P_tiles": lambda: call("cm2_P_tiles_apply", T.h, ptr(z), ptr(tb), st()),
        "k_gap_perm_windows<true>": lambda: call("cm2_gaps_tiles_to_time", gh, T.h, ptr(tb), ptr(comp), ptr(t1), st()),
        "k_perm_windows<true>": lambda: call("cm2_tod_tiles_to_time", T.h, ptr(tb), ptr(t1), st()),
        "N^-1 on the time order": lambda: call("cm2_noise_apply", N._noise.h, ptr(t1), ptr(t2), st()),
        "k_gap_perm_windows<false>": lambda: call("cm2_gaps_time_to_tiles", gh, T.h, ptr(t2), ptr(tb), ptr(comp), st()),
        "k_perm_windows<false>": lambda: call("cm2_tod_time_to_tiles", T.h, ptr(t2), ptr(tb), st()),
        "k_Pt_tiles_fixed": lambda: call("cm2_Pt_tiles_apply", T.h, ptr(tb), ptr(x), st()),
    }
    comp = comp.clone()
    for fn in stages.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res["stages_alone_ms"] = {k: [] for k in stages}
    for _ in range(5):
        for k, fn in stages.items():
            res["stages_alone_ms"][k].append(round(ms(torch, fn, 20), 4))
    chain = ("k_P_tiles", "k_gap_perm_windows<true>", "N^-1 on the time order", "k_gap_perm_windows<false>",
             "k_Pt_tiles_fixed")
    res["sum_of_stages_ms"] = round(sum(min(res["stages_alone_ms"][k]) for k in chain), 4)
    # iteration counts at rtol = 1e-6
    its = []
    m, info, sop = solve_gls_with_gaps(P, N, s["d"], M=s["Mbd"], rtol=1e-6)
    res["solve_gls_with_gaps"] = {"iterations": sop.iterations, "info": info}
    xs, info = cg(A, P.T * N * s["d"], M=s["Mbd"], rtol=1e-6, callback=lambda xk: its.append(1))
    res["plain_solve"] = {"iterations": len(its), "info": info}
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def step_trace():
    s = setup()
    torch, op = s["torch"], s["op"]
    z = torch.rand(op.nmap + op.ng, device="cuda", dtype=torch.float64)
    for _ in range(10):
        op * z
    torch.cuda.synchronize()


def kernel_stats(trace_dir):
    """{kernel: {calls, mean_us}} of the chain's kernels from rocprofv3's kernel_stats.csv."""
    import csv
    rows = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Name", "")
            if any(k in name for k in ("k_gap_perm_windows", "k_os_real", "k_P_tiles", "k_Pt_tiles", "k_parts_combine")):
                rows[name.split("(")[0][-60:]] = {"calls": int(r.get("Calls", 0)),
                                                  "mean_us": round(float(r.get("AverageNs", 0)) / 1e3, 1)}
    return rows


def main():
    if "--step" in sys.argv:
        step = sys.argv[sys.argv.index("--step") + 1]
        return step_time(sys.argv[-1]) if step == "time" else step_trace()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gap_aware_timing.json")
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
    res["rocprofv3_kernel_stats_of_10_applications"] = kernel_stats(trace_dir)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["rocprofv3_kernel_stats_of_10_applications"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
