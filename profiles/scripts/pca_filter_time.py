#!/usr/bin/env python3
"""
Time of PCAFilterLO (cm2_pca_cov, cm2_pca_apply) at 1e8 detector samples: ns = 1e7 with 10 detectors
in one group, ns = 1e5 with 1000 detectors in one group and in ten groups of 100, each with one chunk and with ten,
10 % of the samples flagged at random.

For the covariance: its time; a device copy of the bytes it reads at least once (8 B of d and 4 B of flags per
sample); its multiply-add count (n (n + 1) / 2 per sample and group: the lower triangle) divided by the rate of a bare
loop of independent v_mfma_f64_16x16x4_f64 measured here (MFMA_SRC below: 4 waves a workgroup, 16 accumulators a wave,
operands in registers); and, for comparison only, a masked copy plus torch.mm(X, X.T) per unit (rocBLAS: the full
square, an nt-sized temporary, no stated order).  For the apply at K = 1, 3, 10: its time beside CommonModeFilterLO
at the same shape and K, in the same run.

    python profiles/scripts/pca_filter_time.py [out.json]       # every GPU step under its own `timeout`, chained
    python profiles/scripts/pca_filter_time.py --build          # compile the MFMA loop only (no GPU needed)
    python profiles/scripts/pca_filter_time.py --step N out.json

One process per shape; 3 warm-up calls of every variant, then 20 rounds in which every variant is called once
(variants alternated), each timed by a host clock around the call and a device synchronise; median, min, max in ms.
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
SHAPES = ((10_000_000, 10, 1), (100_000, 1000, 1), (100_000, 1000, 10))               # ns, ndet, groups
CHUNKS = (1, 10)
KS = (1, 3, 10)
FLAGGED = 0.10
WARMUP, ROUNDS = 3, 20
MFMA_LIB = os.path.join(HERE, "build", "libmfma_f64_rate.so")
MFMA_ITERS, MFMA_BLOCKS = 4096, 256 * 8

MFMA_SRC = r"""
#include <hip/hip_runtime.h>
typedef double double4_t __attribute__((ext_vector_type(4)));
// every wave: iters rounds of 16 independent v_mfma_f64_16x16x4_f64 (16 x 16 x 4 multiply-adds each)
__global__ __launch_bounds__(256) void k_rate(int iters, double *out)
{
    double4_t acc[16];
    for (int j = 0; j < 16; ++j) acc[j] = (double4_t){0.0, 0.0, 0.0, 0.0};
    double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
    }
    double s = 0.0;
    for (int j = 0; j < 16; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
    if (s == 12345.678) out[0] = s;                          // keeps the loop alive, never true
}
extern "C" int mfma_rate_launch(int blocks, int iters, double *out, void *stream)
{
    k_rate<<<blocks, 256, 0, (hipStream_t)stream>>>(iters, out);
    return (int)hipGetLastError();
}
"""


def build_mfma():
    os.makedirs(os.path.dirname(MFMA_LIB), exist_ok=True)
    src = MFMA_LIB[:-3] + ".hip"
    if os.path.exists(MFMA_LIB) and os.path.exists(src) and open(src).read() == MFMA_SRC:
        return MFMA_LIB
    open(src, "w").write(MFMA_SRC)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", src, "-o", MFMA_LIB])
    return MFMA_LIB


def timed(fns, torch):
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
    return {k: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
            for k, t in ms.items()}


def step_gpu(which, out_path):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import CommonModeFilterLO, PCAFilterLO
    ns, ndet, groups = SHAPES[which]
    n = ns * ndet
    res = {"shape": {"ns": ns, "ndet": ndet, "groups": groups}, "warmup": WARMUP, "rounds": ROUNDS,
           "device": torch.cuda.get_device_name(0), "flagged": FLAGGED}
    # the bare MFMA loop
    lib = ctypes.CDLL(build_mfma())
    lib.mfma_rate_launch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    sink = D.empty(1)
    t = timed({"mfma": lambda: lib.mfma_rate_launch(MFMA_BLOCKS, MFMA_ITERS, D.ptr(sink), D.stream())}, torch)["mfma"]
    madds = MFMA_BLOCKS * 4 * MFMA_ITERS * 16 * (16 * 16 * 4)
    rate = madds / (t["median_ms"] * 1e-3)
    res["mfma_loop"] = dict(t, multiply_adds=madds, multiply_adds_per_s=rate, TFLOPs=round(2 * rate / 1e12, 2))
    g = torch.Generator(device="cuda").manual_seed(ns + ndet + groups)
    pix = torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int32)
    pix[torch.rand(n, generator=g, device="cuda") < FLAGGED] = -1
    v = torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
    out = D.empty(n)
    src = torch.zeros(n * 12, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    gsize = ndet // groups
    res["chunks"] = {}
    for nchunks in CHUNKS:
        clen = ns // nchunks
        F = PCAFilterLO(pix, ndet, nmodes=1, groups=gsize, chunks=clen)
        cov = D.empty(F.filter_info()["cov_doubles"])
        X, keep = v.view(ndet, ns), (pix >= 0).view(ndet, ns)

        def blas():
            Xm = torch.where(keep, X, torch.zeros((), dtype=X.dtype, device=X.device))      # the nt-sized temporary
            return [torch.mm(Xm[a:a + gsize, c:c + clen], Xm[a:a + gsize, c:c + clen].T)
                    for c in range(0, ns, clen) for a in range(0, ndet, gsize)]

        fns = {"cov": lambda: _hip.call("cm2_pca_cov", F._handle.h, D.ptr(v), D.ptr(pix), D.ptr(cov), D.stream()),
               "copy of 12 B per sample": lambda: dst.copy_(src),
               "masked copy + torch.mm per unit": blas}
        r = timed(fns, torch)
        lower = groups * gsize * (gsize + 1) // 2 * ns
        r["cov"].update(multiply_adds_lower_triangle=lower,
                        mfma_floor_ms=round(1e3 * lower / rate, 4),
                        copy_floor_ms=r["copy of 12 B per sample"]["median_ms"],
                        work_doubles=F.filter_info()["work_doubles"], work_items=F.filter_info()["work_items"])
        entry = res["chunks"][str(nchunks)] = {"cov": r, "apply": {}}
        rng = np.random.default_rng(nchunks)
        for K in KS:
            if gsize < K + 1:                                # refused: K modes need K + 1 detectors in every group
                entry["apply"][str(K)] = None
                continue
            modes = rng.standard_normal((nchunks, ndet, K))
            Fk = PCAFilterLO(pix, ndet, groups=gsize, chunks=clen, modes=modes)
            Fc = CommonModeFilterLO(pix, ndet, modes=modes[0], groups=gsize)
            entry["apply"][str(K)] = timed({
                "pca": lambda: _hip.call("cm2_pca_apply", Fk._handle.h, D.ptr(v), D.ptr(out), D.stream()),
                "cmode": lambda: _hip.call("cm2_cmode_apply", Fc._handle.h, D.ptr(v), D.ptr(out), D.stream())}, torch)
            del Fk, Fc
        del F, cov
        torch.cuda.empty_cache()
    allres = json.load(open(out_path)) if os.path.exists(out_path) and which else {}
    allres["ns %d x ndet %d, %d group(s)" % (ns, ndet, groups)] = res
    json.dump(allres, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def main():
    if "--build" in sys.argv:
        print(build_mfma())
        return 0
    if "--step" in sys.argv:
        return step_gpu(int(sys.argv[sys.argv.index("--step") + 1]), sys.argv[-1])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pca_filter_timing.json")
    for which in range(len(SHAPES)):                         # chained: a failed step ends the run
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--step", str(which), out]
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
