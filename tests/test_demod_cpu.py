"""
The demodulator without a GPU: the NumPy restatement of _demod_ref.py against an independent brute force, the
conditions the shared cases must meet, the detection quality of the definition itself, the default taps,
cm2_demod_policy.h compiled with the host compiler and checked against Python, the header's prototypes and constants,
the exported names and every argument check of the Python layer.
"""
import ctypes
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _demod_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
ENTRY_POINTS = {"create": 8, "destroy": 1, "info": 2, "run": 13, "pick": 6}
EPS = 2.0 ** -53


# ------------------------------------------------- the restatement against a brute force ----
ONE_SIGN = ["sizes_D1_L1", "sizes_D2_L1", "sizes_D8_L1", "sizes_D64_L1", "sizes_D3_L7", "sizes_D7_L15", "sizes_D8_L17",
            "weight_edge", "min_weight_1", "subnormals", "chain_order"]


def brute(c):
    """Every output on its own from exact window sums (math.fsum): (T, Q, U, W, included, bound on |T - T_ref|, on
    |Q - Q_ref|, on |U - U_ref|), the bound (L + 2) 2^-53 sum|h_k x_i| / W of the issue that asked for this stage.
    The restatement's chain of n terms makes n products and n - 1 additions, each within 2^-53 of a quantity no
    larger than sum|h x| to first order, the carrier product and the division one more each: L + 2 roundings at the
    most.  W's own chain adds up to L - 1 more, each relative to W itself as long as the included taps have one sign
    (no cancellation), which only the cases listed in ONE_SIGN are: with taps of both signs the error of W is relative
    to sum|h_k|, not to W, and this bound does not hold."""
    use, e = R.usable(c.d, c.flags), R.edges(c.sizes)
    L = c.h.size
    half = (L - 1) // 2
    rows = []
    for b0, b1 in zip(e[:-1], e[1:]):
        n = int(b1 - b0)
        for j in range(-(-n // c.D)):
            tT, tQ, tU, tW = [], [], [], []
            for k in range(L):
                i = j * c.D - half + k
                if 0 <= i < n and use[b0 + i]:
                    x, h = float(c.d[b0 + i]), float(c.h[k])
                    tT.append(h * x)
                    tQ.append(h * (x * float(c.cosv[b0 + i])))
                    tU.append(h * (x * float(c.sinv[b0 + i])))
                    tW.append(h)
            W = math.fsum(tW)
            scale = (L + 2) * EPS / W if W > 0 else 0.0
            rows.append((math.fsum(tT), math.fsum(tQ), math.fsum(tU), W, len(tW),
                         scale * math.fsum(map(abs, tT)), 2 * scale * math.fsum(map(abs, tQ)),
                         2 * scale * math.fsum(map(abs, tU))))
    return [np.array(col) for col in zip(*rows)]


@pytest.mark.parametrize("name", ONE_SIGN)
def test_restatement_against_brute_force(name):
    c, want = R.case(name), R.expected(name)
    assert (c.h > 0).all()                                                    # every tap of one sign
    sT, sQ, sU, W, n, bT, bQ, bU = brute(c)
    assert np.array_equal(n, want.n)
    thr = c.min_weight * want.wfull
    ok = W >= thr
    # the weight test decides alike unless W sits within its rounding of the threshold (weight_edge sits on it, exactly)
    clear = np.abs(W - thr) > c.h.size * EPS * np.abs(W)
    assert np.array_equal((want.cls != R.REJECTED)[clear], ok[clear])
    assert np.array_equal(want.cls == R.FULL, n == c.h.size)
    keep = want.cls != R.REJECTED
    with np.errstate(invalid="ignore", divide="ignore"):
        for got, s, bound in ((want.T, sT, bT), (want.Q, 2 * sQ, bQ), (want.U, 2 * sU, bU)):
            err = np.abs(got[keep] - s[keep] / W[keep])
            assert (err <= bound[keep]).all(), (name, np.flatnonzero(err > bound[keep])[:10])
            assert not got[~keep].any()
    assert want.counts.sum() == want.M == len(n)


def test_pick_restatement():
    sizes, D = [10, 1, 17], 4
    pix = np.arange(28, dtype=np.int32)
    pix[[4, 27]] = -5
    cls = np.array([0, 1, 2, 0, 0, 1, 2, 0, 0], dtype=np.uint8)
    assert R.out_sizes(sizes, D) == [3, 1, 5]
    assert R.pick(pix, cls, sizes, D, 2).tolist() == [0, -1, -1, 10, 11, 15, -1, 23, -1]
    assert R.pick(pix, cls, sizes, D, 1).tolist() == [0, -1, -1, 10, 11, -1, -1, 23, -1]


# ------------------------------------------------------- conditions on the shared cases ----
def test_size_cases_are_the_ones_the_issue_lists():
    assert set(R.CASES) == set(R.cases()) and len(set(R.CASES)) == len(R.CASES)
    shapes = set(R.SIZE_SHAPES)
    assert {D for D, _ in shapes} >= {1, 2, 8, 64}
    for D in (1, 2, 8, 64):
        assert {(D, 1), (D, 3), (D, 2 * D + 1), (D, 1025)} <= shapes
    for D, L in R.SIZE_SHAPES:
        c, want = R.case("sizes_D%d_L%d" % (D, L)), R.expected("sizes_D%d_L%d" % (D, L))
        half, unit = (L - 1) // 2, R.unit_len(D)
        for s in (1, half, half + 1, D - 1, D, D + 1, unit - 1, unit, unit + 1, unit + half):
            assert s < 1 or s in c.sizes, (D, L, s)
        assert c.h.size == L and unit % D == 0 and unit <= 2048 < unit + D
        assert any(s % D == 1 for s in c.sizes) or D == 1                     # a last output centred on the last sample
        assert any(s > unit and s % unit % D for s in c.sizes) or D == 1      # outputs across a unit edge, D not dividing
        assert want.M == sum(-(-s // D) for s in c.sizes) and c.flags.dtype == np.int32
        assert R.PARTIAL in want.cls or L == 1
        full = R.expected(c.name, True, "none")                               # without flags every interior output is full
        assert (full.cls == R.FULL).sum() == sum(max(0, (s - 1 - half) // D - -(-half // D) + 1) for s in c.sizes)
    assert R.rounds(1) == R.ROUNDS == 8 and R.rounds(8) == 1 and R.rounds(3) == 3 and R.rounds(7) == 2


def test_special_cases_are_what_they_say():
    c, want = R.case("flag_run"), R.expected("flag_run")
    assert c.h.size == 9 and (want.cls[126:132] == R.REJECTED).all() and not want.T[126:132].any()
    assert not want.Q[126:132].any() and not want.U[126:132].any()
    assert want.cls[299] == R.PARTIAL and want.cls[300] == R.PARTIAL and want.cls[298] == want.cls[301] == R.FULL
    assert (want.cls[748:750] == R.REJECTED).all() and (want.cls[750:752] == R.REJECTED).all()    # both sides of the edge
    want = R.expected("weight_edge")
    assert want.wfull == 3.0 and want.W[[25, 50, 75]].tolist() == [1.5, 1.25, 1.5]
    assert want.cls[[25, 50, 75]].tolist() == [R.PARTIAL, R.REJECTED, R.PARTIAL] and want.T[50] == 0.0 and want.T[25] != 0
    c, want = R.case("min_weight_1"), R.expected("min_weight_1")
    assert c.min_weight == 1.0 and c.flags.dtype == np.uint8 and set(want.cls) == {R.FULL, R.REJECTED}
    assert (want.cls == R.REJECTED).sum() == 5 and (want.n[want.cls == R.REJECTED] < 7).all()
    want = R.expected("negative_lobes")
    assert want.W[[50, 100, 150]].tolist() == [-1.0, 0.0, 3.0] and want.wfull == 1.0
    assert want.cls[[50, 100, 150]].tolist() == [R.REJECTED, R.REJECTED, R.PARTIAL]
    c, want = R.case("nonfinite"), R.expected("nonfinite")
    e, unit = R.edges(c.sizes), R.unit_len(c.D)
    where = [0, e[1] - 1, e[1], e[2] - 1, e[2], e[3] - 1, unit - 1, unit, unit + 1, e[1] + unit, e[1] + 2 * unit - 1]
    assert not np.isfinite(c.d[where]).any() and np.isfinite(want.T).all() and np.isfinite(want.U).all()
    assert np.isnan(c.cosv[300]) and np.isnan(c.sinv[301]) and c.flags[300] < 0 and c.flags[301] < 0
    assert np.isnan(want.Q).sum() == 3 and np.isnan(want.Q[299:302]).all()    # the NaN carrier under a usable sample
    want = R.expected("huge_pairs")
    assert np.isinf(want.T[99:103]).all() and np.isfinite(want.T[298:306]).all() and want.T[302] == 0.2
    c, want = R.case("subnormals"), R.expected("subnormals")
    assert (np.abs(c.d) < 2.3e-308).all() and want.T.any() and (np.abs(want.T) < 2.3e-308).all() and want.Q.any()
    c, want = R.case("shortcut"), R.expected("shortcut")
    unit, per = R.unit_len(c.D), R.per_unit(c.D)
    use = R.usable(c.d, c.flags)
    half = (c.h.size - 1) // 2
    assert use[unit - half:2 * unit - c.D + half + 1].all() and (want.cls[per:2 * per] == R.FULL).all()
    for g in (0, 2, 3):                                                       # the neighbours stage one unusable sample
        assert (~use[max(0, g * unit - half):(g + 1) * unit - c.D + half + 1]).sum() == 1
    assert want.counts.tolist() == [[1008, 17, 0]]


def test_the_stated_chain_order_is_the_only_one_that_gives_the_expected_bits():
    want = R.expected("chain_order")
    assert R.TWO53 + 1.0 == R.TWO53
    # the window 99 .. 101 holds 2^53, 1, -2^53: ascending 0, descending 1
    assert (0.0 + R.TWO53 + 1.0) + -R.TWO53 == 0.0 and (0.0 + -R.TWO53 + 1.0) + R.TWO53 == 1.0
    assert want.T[100] == 0.0 and want.Q[100] == 0.0
    # the window 149 .. 151 holds -2^53, 2^53, 1: ascending 1, descending 0
    assert want.T[150] == 1.0 / 3.0 and (0.0 + 1.0 + R.TWO53) + -R.TWO53 == 0.0
    assert want.Q[150] == 2.0 * (1.0 / 3.0)


# ------------------------------------------------------------------ detection quality ----
@pytest.mark.parametrize("D,fm", R.QUALITY)
def test_the_definition_recovers_constant_stokes_parameters(D, fm):
    I, Q, U = R.QUALITY_IQU
    h = R.default_taps(D)
    half = (h.size - 1) // 2
    d, co, si = R.quality_stream(fm)
    got = R.run(d, [R.QUALITY_N], D, h, None, co, si, 0.5)
    bT, bQ = R.quality_bounds(h, fm)
    j = np.arange(got.M)
    inside = (j * D - half >= 0) & (j * D + half < R.QUALITY_N)
    assert np.array_equal(inside, got.cls == R.FULL) and inside.sum() > 100
    eT, eQ, eU = (np.abs(x - v) for x, v in ((got.T, I), (got.Q, Q), (got.U, U)))
    print("D %d f_m %.2f: |T - I| <= %.3g (bound %.3g), |Q^ - Q| <= %.3g, |U^ - U| <= %.3g (bound %.3g); partial outputs "
          "up to %.3g, %.3g" % (D, fm, eT[inside].max(), bT, eQ[inside].max(), eU[inside].max(), bQ,
                                eT[~inside].max(), max(eQ[~inside].max(), eU[~inside].max())))
    assert (eT[inside] <= bT).all() and (eQ[inside] <= bQ).all() and (eU[inside] <= bQ).all()
    # a truncated window breaks these bounds although W is close to Wfull: why the class partial exists
    partial = got.cls == R.PARTIAL
    assert partial.any() and (got.W[partial] >= 0.5 * got.wfull).all()
    assert (eT[partial] > bT).any() and ((eQ[partial] > bQ) | (eU[partial] > bQ)).any()


# -------------------------------------------------------------------------------- taps ----
@pytest.mark.parametrize("D", [1, 2, 3, 4, 8, 16, 64])
def test_default_taps(D):
    from cosmomap2_amd.utilities import lowpass_taps
    h = lowpass_taps(D)
    assert h.dtype == np.float64 and h.size == 16 * D + 1 and np.array_equal(R.bits(h), R.bits(R.default_taps(D)))
    assert np.array_equal(h, h[::-1])                                         # symmetric, bit for bit
    assert abs(math.fsum(h) - 1.0) <= 2.0 ** -52                              # 1 to one ulp
    # the stopband: beyond the slow streams' Nyquist frequency |H| stays below the worst sidelobe of the window itself
    half = (h.size - 1) // 2
    k = np.arange(h.size) - half
    w = 0.54 + 0.46 * np.cos(np.pi * k / (half + 1))
    f = np.linspace(0.0, 0.5, 40001)
    E = np.exp(-2j * np.pi * np.outer(f, k))
    Wf, Hf = np.abs(E @ w) / w.sum(), np.abs(E @ h)
    first_null = int(np.argmax(np.diff(Wf) > 0))
    side = Wf[first_null:].max()
    assert 0.005 < side < 0.02 and Hf[f >= 0.5 / D].max() < side
    assert abs(Hf[0] - 1.0) < 1e-12 and (Hf[f <= 0.2 / D] > 0.99).all()       # and passes its band
    # other lengths and cut-offs
    g = lowpass_taps(D, 2 * D + 1, 0.25 / D)
    assert g.size == 2 * D + 1 and np.array_equal(g, g[::-1]) and abs(math.fsum(g) - 1.0) <= 2.0 ** -52
    assert lowpass_taps(D, 1).tolist() == [1.0]


# ------------------------------------------------------------------ names and header ----
def test_names_are_exported_and_the_header_declares_the_entry_points():
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, build as B, kernel_resources as KR
    M = importlib.import_module("cosmomap2_amd.utilities.demodulate")    # (the package's demodulate is the function)
    for name in ("Demodulator", "demodulate", "decimate", "lowpass_taps"):
        assert callable(getattr(U, name)) and name in M.__all__
    assert U.DEMOD_CLASSES == ("full", "partial", "rejected") == R.CLASSES
    for name in ("decimate", "demodulate", "pick", "out_blocksize", "info"):
        assert callable(getattr(U.Demodulator, name))
    hdr = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint cm2_demod_%s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_hip.PROTOTYPES["cm2_demod_" + name]), name
        assert "cm2_demod_" + name in _hip.RESTARTABLE                        # no entry point works in place
    assert re.search(r"#define CM2_DEMOD_MAX_FACTOR 64\b", hdr) and R.MAX_FACTOR == M.MAX_FACTOR == 64
    assert re.search(r"#define CM2_DEMOD_MAX_TAPS 1025\b", hdr) and R.MAX_TAPS == M.MAX_TAPS == 1025
    for code, name in enumerate(("FULL", "PARTIAL", "REJECTED")):
        assert re.search(r"#define CM2_DEMOD_%s %d\b" % (name, code), hdr)
        assert getattr(R, name) == getattr(M, name) == code
    assert hdr.index("---- f2f:") < hdr.index("---- f2g:") < hdr.index("---- f2h:") < hdr.index("---- f3:")
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert "cm2_demod_" + name in integ, name
    for k in ("k_demod_fir<true, 0>", "k_demod_pick"):
        assert any(re.search(p, k) for p in KR.NO_SPILL), k
    assert "cm2_demod.hip" not in B.FMA_OK
    src = open(os.path.join(CSRC, "cm2_demod.hip")).read()
    body = src.split('#include "cm2_common.h"')[1]
    assert set(re.findall(r"\batomic\w*\s*\(\s*&?\s*([\w.>-]+)", body)) == {"tally", "o.counts"}   # integer tallies only
    assert re.search(r"unsigned int tally", body) and re.search(r"unsigned long long \*counts", body)
    assert "__shfl" not in body and "mfma" not in body and "fma(" not in body


def test_the_built_kernels_use_no_scratch():
    from cosmomap2_amd import build as B, kernel_resources as KR
    B.build(verbose=False)
    own = {r["kernel"]: r for r in KR.load_all() if r["unit"] == "cm2_demod" and r["kernel"].startswith("k_demod_")}
    table = open(os.path.join(ROOT, "profiles", "kernel_resources.md")).read()
    want = ["k_demod_fir<%s, %d>" % (c, k) for c in ("false", "true") for k in (0, 1)] + ["k_demod_pick"]
    assert sorted(own) == sorted(want)
    for k in want:
        assert own[k].get("scratch_bytes_per_lane", 0) == 0 and own[k].get("vgpr_spill", 0) == 0, own[k]
        assert "`%s`" % k in table, k
    # two workgroups of 256 threads a CU are two waves a SIMD: the registers must leave room for them
    assert all(own[k]["vgpr"] <= 256 and own[k]["occupancy"] >= 2 for k in want)


def test_null_arguments_are_refused_without_a_gpu():
    from cosmomap2_amd import _hip
    lib = _hip.load()
    assert lib.cm2_demod_destroy(None) == 0
    for name in ENTRY_POINTS:
        if name == "destroy":
            continue
        args = [0 if a in (ctypes.c_int, ctypes.c_int64) else 0.0 if a is ctypes.c_double else None
                for a in _hip.PROTOTYPES["cm2_demod_" + name]]
        assert getattr(lib, "cm2_demod_" + name)(*args) == _hip.ERR_ARGUMENT, name
        assert b"cm2_demod_" + name.encode() in lib.cm2_last_error(), (name, lib.cm2_last_error())
    h = ctypes.c_void_p()

    def create(nt, sizes, D, taps):
        sz = (ctypes.c_int64 * len(sizes))(*sizes)
        tp = (ctypes.c_double * max(1, len(taps)))(*taps)
        return lib.cm2_demod_create(ctypes.byref(h), nt, sz, len(sizes), D, tp, len(taps), None), lib.cm2_last_error()

    ok = [0.25, 0.5, 0.25]
    for args, word in (((100, [100], 0, ok), b"factor"), ((100, [100], 65, ok), b"factor"),
                       ((2 ** 32 - 1, [2 ** 32 - 1], 4, ok), b"32-bit"), ((100, [60, 30], 4, ok), b"add up"),
                       ((100, [100, 0], 4, ok), b"add up"), ((0, [1], 4, ok), b"nt="),
                       ((100, [100], 4, [0.5, 0.5]), b"odd"), ((100, [100], 4, []), b"odd"),
                       ((100, [100], 4, [1.0] * 1027), b"odd"), ((100, [100], 4, [1.0, float("nan"), 1.0]), b"finite"),
                       ((100, [100], 4, [1.0, float("inf"), 1.0]), b"finite"),
                       ((100, [100], 4, [1.0, -2.0, 1.0]), b"sum"), ((100, [100], 4, [1e308, 1e308, 1e308]), b"sum"),
                       ((100, [100], 4, [1.0, -1.0, 0.0]), b"sum")):
        rc, msg = create(*args)
        assert rc == _hip.ERR_ARGUMENT and b"cm2_demod_create" in msg and word in msg, (args[:3], rc, msg)
        assert not h.value


# ----------------------------------------------------- the policy header, on a CPU ----
DRIVER = r"""
#include "cm2_demod_policy.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace cm2::demod;
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "constants")) {
        printf("%d %d %d %d %d %d %lld %lld\n", kMaxFactor, kMaxTaps, kThreads, kMaxUnit, kRounds, kCounts,
               (long long)kLdsLimit, (long long)kMaxBlocks);
        printf("%d %d %d\n", (int)kFull, (int)kPartial, (int)kRejected);
        for (int D = 1; D <= kMaxFactor; ++D)
            printf("%d %d %d %lld %lld %lld %lld\n", outputs_per_unit(D), unit_len(D), rounds(D),
                   (long long)lds_bytes(D, 1, true), (long long)lds_bytes(D, 1, false),
                   (long long)lds_bytes(D, kMaxTaps, true), (long long)lds_bytes(D, kMaxTaps, false));
        return 0;
    }
    if (!strcmp(argv[1], "lds")) {                // lds D L
        const int D = atoi(argv[2]), L = atoi(argv[3]);
        printf("%lld %lld %d %d\n", (long long)lds_bytes(D, L, true), (long long)lds_bytes(D, L, false),
               staged(outputs_per_unit(D), D, L), slots(staged(outputs_per_unit(D), D, L)));
        return 0;
    }
    if (!strcmp(argv[1], "slot")) {               // slot n: the slots of the values 0 .. n - 1, all different
        const int n = atoi(argv[2]);
        int last = -1, ok = 1;
        for (int v = 0; v < n; ++v) {
            ok = ok && slot(v) > last && slot(v) < slots(n);
            last = slot(v);
        }
        printf("%d %d\n", ok, slots(n));
        return 0;
    }
    if (!strcmp(argv[1], "checks")) {             // checks have_flags kind min_weight drop_from included L weight_ok
        printf("%d %d %d\n", (int)check_run(atoi(argv[2]) != 0, atoi(argv[3]), atof(argv[4])),
               (int)check_pick(atoi(argv[5])), class_of(atoi(argv[6]), atoi(argv[7]), atoi(argv[8]) != 0));
        return 0;
    }
    // create|status nt D ntaps tap s0 s1 ...   (every tap has the value tap, but tap "mixed": 1, -1, 0 ...; no
    // sizes: a null pointer; ntaps < 0: a null pointer for the taps)
    // ones n D                                  n blocks of one sample
    std::vector<int64_t> s;
    for (int i = 6; i < argc; ++i) s.push_back(atoll(argv[i]));
    int ntaps = 1;
    std::vector<double> taps(1, 1.0);
    if (!strcmp(argv[1], "ones")) {
        s.assign((size_t)atoll(argv[2]), 1);
    } else {
        ntaps = atoi(argv[4]);
        taps.assign((size_t)(ntaps > 0 ? ntaps : 1), strcmp(argv[5], "mixed") ? atof(argv[5]) : 0.0);
        if (!strcmp(argv[5], "mixed") && ntaps >= 2) {
            taps[0] = 1.0;
            taps[1] = -1.0;
        }
    }
    Launch l;
    const Status st = check_create(&l, atoll(argv[2]), s.empty() ? nullptr : s.data(), (int64_t)s.size(), atoi(argv[3]),
                                   ntaps < 0 ? nullptr : taps.data(), ntaps);
    printf("%d\n", (int)st);
    if (st != kOk || strcmp(argv[1], "create")) return 0;
    printf("%lld %lld %lld %lld %d %d %d %d %d %d %lld %lld %.17g\n", (long long)l.nt, (long long)l.nblocks,
           (long long)l.units, (long long)l.M, l.D, l.L, l.c, l.unit, l.per_unit, l.rounds, (long long)l.lds_carrier,
           (long long)l.lds_plain, l.wfull);
    std::vector<int64_t> off(s.size() + 1, 0), us(s.size() + 1, 0), os(s.size() + 1, 0);
    for (size_t b = 0; b < s.size(); ++b) {
        off[b + 1] = off[b] + s[b];
        us[b + 1] = us[b] + units_of(s[b], l.unit);
        os[b + 1] = os[b] + outputs_of(s[b], l.D);
    }
    for (int64_t g = 0; g < l.units; ++g) {
        const Span sp = unit_span(off.data(), us.data(), l.nblocks, l.unit, g);
        printf("u %lld %lld %lld %lld %lld\n", (long long)sp.block, (long long)sp.first, (long long)sp.end,
               (long long)outputs_of(sp.end - sp.first, l.D),
               (long long)(os[sp.block] + (sp.first - off[sp.block]) / l.D));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("demod_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [ln.split() for ln in p.stdout.splitlines()]


def test_policy_constants_and_lds(driver):
    out = _run(driver, "constants")
    assert [int(x) for x in out[0]] == [64, 1025, R.THREADS, R.MAX_UNIT, R.ROUNDS, 3, 80 * 1024, 1 << 18]
    assert [int(x) for x in out[1]] == [R.FULL, R.PARTIAL, R.REJECTED]
    worst = 0
    for D in range(1, 65):
        per, unit, rounds, c1, p1, cmax, pmax = [int(x) for x in out[1 + D]]
        assert (per, unit, rounds) == (R.per_unit(D), R.unit_len(D), R.rounds(D))
        assert unit % D == 0 and unit <= 2048 < unit + D and (rounds - 1) * 256 < per <= rounds * 256 <= 8 * 256
        assert (c1, p1, cmax, pmax) == (R.lds_bytes(D, 1), R.lds_bytes(D, 1, False), R.lds_bytes(D, 1025),
                                        R.lds_bytes(D, 1025, False))
        n = (per - 1) * D + 1025
        assert cmax >= 25 * (n + (n - 1) // 32) and cmax % 8 == 0 and n <= 3072
        worst = max(worst, cmax)
    # every (D, L) corner: two workgroups with a carrier fit the 160 KB of a CU
    assert worst == R.lds_bytes(1, 1025) == 79176 and 2 * worst <= 160 * 1024
    for D, L in ((1, 1), (1, 1025), (64, 1), (64, 1025), (8, 129), (63, 1025), (33, 3)):
        lc, lp, staged, slots = [int(x) for x in _run(driver, "lds", D, L)[0]]
        assert staged == (R.per_unit(D) - 1) * D + L and slots == R.slots(staged)
        assert (lc, lp) == (R.lds_bytes(D, L), R.lds_bytes(D, L, False)) and lp >= 9 * slots and lc >= 25 * slots
    assert R.lds_bytes(64, 1025) == 77576
    for n in (1, 31, 32, 33, 3009, 3072):
        assert _run(driver, "slot", n)[0] == ["1", str(R.slots(n))]


SIZE_SETS = [[1], [1, 2, 63, 64, 65, 131], [2047, 2048, 2049, 1, 4097], [2046, 2047, 4093, 6140], [7] * 40, [100000]]


@pytest.mark.parametrize("sizes", SIZE_SETS)
@pytest.mark.parametrize("D", [1, 3, 8, 64])
def test_units_cover_every_sample_and_every_output_exactly_once(driver, sizes, D):
    nt, L = sum(sizes), 2 * D + 1
    out = _run(driver, "create", nt, D, L, 0.5, *sizes)
    assert out[0] == ["0"]
    unit = R.unit_len(D)
    units = sum(-(-s // unit) for s in sizes)
    M = sum(R.out_sizes(sizes, D))
    head = out[1]
    assert [int(x) for x in head[:12]] == [nt, len(sizes), units, M, D, L, D, unit, R.per_unit(D), R.rounds(D),
                                           R.lds_bytes(D, L), R.lds_bytes(D, L, False)]
    assert float(head[12]) == R.tap_sum([0.5] * L)
    e = R.edges(sizes)
    oe = R.edges(R.out_sizes(sizes, D))
    spans = [[int(x) for x in ln[1:]] for ln in out[2:] if ln[0] == "u"]
    assert len(spans) == units
    seen, seen_out = np.zeros(nt, dtype=np.int64), np.zeros(M, dtype=np.int64)
    for b, first, end, nout, out0 in spans:
        assert e[b] <= first < end <= e[b + 1] and end - first <= unit                    # never crosses a block
        assert (first - e[b]) % unit == 0 and (end - first == unit or end == e[b + 1])
        assert nout == -(-(end - first) // D) <= R.per_unit(D)
        assert oe[b] <= out0 and out0 + nout <= oe[b + 1] and out0 - oe[b] == (first - e[b]) // D
        seen[first:end] += 1
        seen_out[out0:out0 + nout] += 1
        # the centres of the unit's outputs are its own samples, and its windows stay within the staged range
        centres = first + D * np.arange(nout)
        assert (centres < end).all() and (nout - 1) * D + L <= (R.per_unit(D) - 1) * D + L
    assert (seen == 1).all() and (seen_out == 1).all()


def test_policy_status_codes(driver):
    def create(nt, D, ntaps, tap, *sizes):
        return int(_run(driver, "status", nt, D, ntaps, tap, *sizes)[0][0])
    assert create(100, 4, 3, 0.5, 60, 40) == 0
    assert create(0, 4, 3, 0.5, 1) == 1 and create(100, 4, 3, 0.5) == 1 and create(-5, 4, 3, 0.5, 1) == 1   # kBadSize
    assert create(100, 4, 3, 0.5, 60, 30) == 2 and create(100, 4, 3, 0.5, 60, 50) == 2                     # kBadBlocks
    assert create(100, 4, 3, 0.5, 100, 0) == 2 and create(2, 4, 3, 0.5, 1, 1, 1) == 2
    assert create(100, 0, 3, 0.5, 100) == 11 and create(100, 65, 3, 0.5, 100) == 11                        # kBadFactor
    assert create(100, -1, 3, 0.5, 100) == 11 and create(100, 1, 3, 0.5, 100) == 0 and create(100, 64, 3, 0.5, 100) == 0
    assert create(2 ** 32 - 1, 4, 3, 0.5, 2 ** 32 - 1) == 4 and create(2 ** 32 - 2, 4, 3, 0.5, 2 ** 32 - 2) == 0
    assert _run(driver, "ones", (1 << 18) + 1, 4)[0] == ["5"] and _run(driver, "ones", 1 << 18, 4)[0] == ["0"]
    assert create(100, 4, 0, 0.5, 100) == 12 and create(100, 4, 2, 0.5, 100) == 12                         # kBadTaps
    assert create(100, 4, 1027, 0.5, 100) == 12 and create(100, 4, -1, 0.5, 100) == 12
    assert create(100, 4, 1, 0.5, 100) == 0 and create(100, 4, 1025, 0.5, 100) == 0
    assert create(100, 4, 3, "nan", 100) == 13 and create(100, 4, 3, "inf", 100) == 13                     # kBadTapValue
    assert create(100, 4, 3, "-inf", 100) == 13
    assert create(100, 4, 3, 0.0, 100) == 14 and create(100, 4, 3, -1.0, 100) == 14                        # kBadTapSum
    assert create(100, 4, 3, 1e308, 100) == 14 and create(100, 4, 3, "mixed", 100) == 14
    assert create(100, 4, 3, 5e-324, 100) == 0
    # two faults at once: the sizes given, then the factor, the 32-bit limit, the blocks, then the taps
    assert create(0, 0, 2, 0.5, 1) == 1 and create(2 ** 32 - 1, 0, 2, 0.5, 2 ** 32 - 1) == 11
    assert create(2 ** 32 - 1, 4, 2, 0.5, 2 ** 32 - 1) == 4 and create(100, 4, 2, 0.5, 60, 30) == 2
    assert create(100, 4, 2, "nan", 100) == 12 and create(100, 4, 3, "nan", 100) == 13

    def checks(have=0, kind=0, min_weight=0.5, drop_from=2, included=3, L=3, ok=1):
        return [int(x) for x in _run(driver, "checks", have, kind, min_weight, drop_from, included, L, ok)[0]]
    assert checks()[:2] == [0, 0] and checks(min_weight=1.0)[0] == 0 and checks(min_weight=1e-300)[0] == 0
    for bad in (0.0, -0.5, 1.0000000000000002, "nan", "inf"):
        assert checks(min_weight=bad)[0] == 15                                                             # kBadMinWeight
    assert checks(have=1, kind=2)[0] == 8 and checks(have=1, kind=-1)[0] == 8                              # kBadFlagKind
    assert checks(have=1, kind=1)[0] == 0 and checks(have=0, kind=7)[0] == 0
    assert checks(drop_from=1)[1] == 0 and checks(drop_from=2)[1] == 0
    assert checks(drop_from=0)[1] == 16 and checks(drop_from=3)[1] == 16                                   # kBadDropFrom
    assert checks(included=3, L=3, ok=1)[2] == R.FULL and checks(included=2, L=3, ok=1)[2] == R.PARTIAL
    assert checks(included=2, L=3, ok=0)[2] == R.REJECTED and checks(included=0, L=3, ok=0)[2] == R.REJECTED


# ------------------------------------------------------ the Python layer's checks ----
def test_arguments_are_refused_before_the_gpu_is_needed():
    import torch
    from cosmomap2_amd import _hip
    from cosmomap2_amd.utilities import Demodulator, decimate, demodulate, lowpass_taps
    d = np.zeros(100)
    pix = np.zeros(100, dtype=np.int32)
    co, si = np.ones(100), np.zeros(100)
    for kw in (dict(factor=0), dict(factor=65), dict(factor=2.5), dict(factor=True), dict(factor=4, taps=[0.5, 0.5]),
               dict(factor=4, taps=[]), dict(factor=4, taps=np.ones(1027)), dict(factor=4, taps=np.ones((3, 3))),
               dict(factor=4, taps=[1.0, float("nan"), 1.0]), dict(factor=4, taps=[1.0, -2.0, 1.0]),
               dict(factor=4, taps=[1e308] * 3), dict(factor=4, taps="abc"), dict(factor=4, min_weight=0.0),
               dict(factor=4, min_weight=1.5), dict(factor=4, min_weight=float("nan")), dict(factor=4, min_weight="x")):
        with pytest.raises(ValueError) as e:
            Demodulator(10, **kw)
        assert str(e.value), kw
    for bs in (0, -3, 2.5, [], [10, 0], [10, -1], [2.5]):
        with pytest.raises(ValueError):
            Demodulator(bs, 4)
    for args in ((0,), (65,), (2.5,), (4, 4), (4, 0), (4, 1027), (4, 2.0), (4, 9, 0.0), (4, 9, 0.6), (4, 9, "x"),
                 (4, 9, float("nan"))):
        with pytest.raises(ValueError):
            lowpass_taps(*args)
    dm = Demodulator(50, 4)
    assert dm.taps.size == 65 and dm.min_weight == 0.5 and dm.out_blocksize(100) == [13, 13]
    assert Demodulator([60, 41], 8, taps=[1.0]).out_blocksize(101) == [8, 6]
    for bad in (dict(flags=pix[:50]), dict(flags=np.zeros(100)), dict(flags=np.zeros((10, 10), dtype=np.int32))):
        with pytest.raises(ValueError):
            dm.decimate(d, **bad)
        with pytest.raises(ValueError):
            dm.demodulate(d, (co, si), **bad)
        with pytest.raises(ValueError):
            decimate(d, 50, 4, **bad)
    for bad_d in (np.zeros(95), np.zeros((10, 10)), np.zeros(0), np.zeros(100, dtype=complex),
                  torch.zeros(100, dtype=torch.float32), torch.zeros(100, dtype=torch.float64)):   # (a host tensor)
        with pytest.raises(ValueError):
            dm.decimate(bad_d)
    for bad_c in (None, co, (co,), (co, si, si), (co[:99], si), (co, np.zeros((10, 10))), (co, si.astype(complex)),
                  (torch.zeros(100, dtype=torch.float64), si), (co, torch.zeros(100, dtype=torch.float32))):
        with pytest.raises(ValueError):
            dm.demodulate(d, bad_c)
        with pytest.raises(ValueError):
            demodulate(d, 50, 4, bad_c)
    with pytest.raises(ValueError):
        Demodulator([60, 30], 4).decimate(d)                     # the sizes do not add up to the stream
    cls = np.zeros(26, dtype=np.uint8)
    for call in (lambda: dm.pick(pix, cls, drop_from=0), lambda: dm.pick(pix, cls, drop_from=3),
                 lambda: dm.pick(pix, cls, drop_from=1.5), lambda: dm.pick(pix, cls[:25]),
                 lambda: dm.pick(pix, cls.astype(np.int32)), lambda: dm.pick(pix.astype(np.float64), cls),
                 lambda: dm.pick(pix[:95], cls), lambda: dm.pick(pix.reshape(10, 10), cls),
                 lambda: dm.pick(np.full(100, 2 ** 40), cls), lambda: dm.pick(torch.zeros(100, dtype=torch.int64), cls),
                 lambda: dm.out_blocksize(95), lambda: dm.info(95), lambda: dm.out_blocksize(2.5)):
        with pytest.raises(ValueError):
            call()
    if not torch.cuda.is_available():
        for call in (lambda: dm.decimate(d, flags=pix), lambda: dm.demodulate(d, (co, si)), lambda: dm.info(100),
                     lambda: dm.pick(pix, cls), lambda: decimate(d, 50, 4), lambda: demodulate(d, 50, 4, (co, si))):
            with pytest.raises(_hip.HipError):
                call()
