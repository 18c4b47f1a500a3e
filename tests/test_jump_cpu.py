"""
The jump corrector without a GPU: the NumPy restatement of _jump_ref.py against an independent brute force on the
shared cases, the conditions the shared cases must meet, the detection quality of the definition itself,
cm2_jump_policy.h compiled with the host compiler and checked against Python, the header's prototypes and constants,
the exported names and every argument check of the Python layer.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _jump_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
ENTRY_POINTS = {"create": 6, "destroy": 1, "info": 2, "stat": 9, "scale": 5, "find": 11, "correct": 12}
EPS = 2.0 ** -53


# ------------------------------------------------- the restatement against a brute force ----
def brute_statistic(c):
    """exact window sums (math.fsum), their means and difference in long arithmetic: (t, noeval, bound on |t - t_ref|)
    The restatement's sum of n terms is within (n - 1) eps sum|d| of the exact one (each of its n - 1 roundings is at
    most eps times a partial sum, and no partial sum exceeds sum|d| to first order), fsum within eps of it; a division
    and the subtraction add one rounding each: the bound is w eps (sum|d_L| / nL + sum|d_R| / nR) with w + 2 in place of
    w - 1 for the last three roundings and the second order."""
    use, e = R.usable(c.d, c.flags, c.prev), R.edges(c.sizes)
    nt, w = c.d.size, c.w
    t, noeval, bound = np.zeros(nt), np.ones(nt, dtype=np.uint8), np.zeros(nt)
    for b0, b1 in zip(e[:-1], e[1:]):
        for i in range(b0 + w, b1 - w + 1):
            left = [float(x) for x in c.d[i - w:i][use[i - w:i]]]
            right = [float(x) for x in c.d[i:i + w][use[i:i + w]]]
            if len(left) < c.min_count or len(right) < c.min_count:
                continue
            t[i] = math.fsum(right) / len(right) - math.fsum(left) / len(left)
            bound[i] = (w + 2) * EPS * (math.fsum(map(abs, left)) / len(left) + math.fsum(map(abs, right)) / len(right))
            noeval[i] = 0
    return t, noeval, bound


def brute_scale(t, noeval, sizes):
    e = R.edges(sizes)
    out = np.full(len(sizes), np.inf)
    for b in range(len(sizes)):
        a = np.abs(t[e[b]:e[b + 1]])[noeval[e[b]:e[b + 1]] == 0]
        if a.size >= 3:
            k = (a.size - 1) // 2
            out[b] = 1.4826 * np.partition(a, k)[k]
    return out


def brute_find(t, noeval, sizes, w, sigma, nsigma):
    """rules 5 and 6 vectorised: the jumps are the candidates that win against every evaluable rival within w"""
    blk = np.repeat(np.arange(len(sizes)), sizes)
    a = np.where(noeval == 0, np.abs(t), -1.0)
    cand = np.flatnonzero((noeval == 0) & (a > nsigma * np.asarray(sigma, dtype=np.float64)[blk]))
    ev = np.flatnonzero(noeval == 0)
    keep = []
    for p in cand:
        j = ev[(np.abs(ev - p) <= w) & (ev != p) & (blk[ev] == blk[p])]
        if not ((a[j] > a[p]) | ((a[j] == a[p]) & (j < p))).any():
            keep.append(p)
    return np.array(keep, dtype=np.int64)


def brute_classes(nt, sizes, pos, prev, radius):
    """rule 9 vectorised"""
    blk, idx = np.repeat(np.arange(len(sizes)), sizes), np.arange(nt)
    at = np.isin(idx, pos)
    near = np.zeros(nt, dtype=bool)
    for p in pos:
        near |= (np.abs(idx - p) <= radius) & (idx != p) & (blk == blk[p])
    cls = np.where(at, R.AT, np.where(near, R.NEAR, R.CLEAN)).astype(np.uint8)
    return cls if prev is None else np.where(prev != 0, prev, cls).astype(np.uint8)


FINITE_STREAMS = [n for n in R.STREAM_CASES if n not in ("nonfinite", "huge_pairs", "sizes_w256")]


@pytest.mark.parametrize("name", FINITE_STREAMS)
def test_restatement_against_brute_force(name):
    c, want = R.stream_case(name), R.stream_expected(name)
    t, noeval, bound = brute_statistic(c)
    assert np.array_equal(noeval, want.noeval)
    assert (np.abs(t - want.t) <= bound).all(), np.flatnonzero(np.abs(t - want.t) > bound)[:10]
    assert not want.t[want.noeval == 1].any()
    assert np.array_equal(R.bits(want.sigma), R.bits(brute_scale(want.t, want.noeval, c.sizes)))
    assert np.array_equal(want.pos, brute_find(want.t, want.noeval, c.sizes, c.w, want.sigma_used, c.nsigma))
    assert np.array_equal(want.cls, brute_classes(c.d.size, c.sizes, want.pos, c.prev, c.radius))
    assert np.array_equal(want.heights, want.t[want.pos]) and want.njumps.sum() == want.pos.size


@pytest.mark.parametrize("name", R.PEAK_CASES)
def test_peak_restatement_against_the_vectorised_form(name):
    c, want = R.peak_case(name), R.peak_expected(name)
    sigma = [c.sigma] * len(c.sizes)
    assert np.array_equal(want.pos, brute_find(c.t, c.noeval, c.sizes, c.w, sigma, c.nsigma))
    assert np.array_equal(want.cls, brute_classes(c.d.size, c.sizes, want.pos, want.prev, c.radius))
    e = R.edges(c.sizes)
    assert want.njumps.tolist() == [int(((want.pos >= a) & (want.pos < b)).sum()) for a, b in zip(e[:-1], e[1:])]
    # the corrected stream: d minus the sum so far of the block's heights (exact for these heights, fsum otherwise)
    blk = np.repeat(np.arange(len(c.sizes)), c.sizes)
    for i in (0, c.d.size // 2, c.d.size - 1) + tuple(int(p) for p in want.pos[:4]):
        mine = want.heights[(want.pos <= i) & (blk[want.pos] == blk[i])]
        if name not in ("offsets_order", "offsets_overflow"):
            assert want.d_out[i] == pytest.approx(c.d[i] - math.fsum(mine), rel=1e-12, abs=1e-12), i
    prev_n = 0 if want.prev is None else int((want.prev != 0).sum())
    assert want.counts.sum() == c.d.size - prev_n


def test_scale_restatement_against_partition():
    t, noeval, sizes = R.scale_cases()
    sigma, eb = R.scale(t, noeval, sizes)
    assert np.array_equal(R.bits(sigma), R.bits(brute_scale(t, noeval, sizes)))
    assert eb[:6].tolist() == [0, 2, 3, 4, 10, 10] and 3000 < eb[6] < 4000
    assert np.isinf(sigma[:2]).all() and np.isfinite(sigma[2:]).all() and sigma[4] == 1.4826 * 0.75 and sigma[5] == 0.0
    # definition 4 of f2e with d = r = t, the noeval bytes as flags and h = 1 is the same number
    import _glitch_ref as G
    same, mb = G.scale(t, t, sizes, 1, noeval)
    assert np.array_equal(R.bits(sigma), R.bits(same)) and np.array_equal(mb, eb)


# ------------------------------------------------------- conditions on the shared cases ----
def test_stream_cases_are_the_ones_the_issue_lists():
    assert R.W_EDGES == (1, 2, 64, 256) and set(R.STREAM_CASES) == set(R.stream_cases())
    for w in R.W_EDGES:
        c, want = R.stream_case("sizes_w%d" % w), R.stream_expected("sizes_w%d" % w)
        assert c.sizes == [1, 2 * w - 1, 2 * w, 2 * w + 1, 2047, 2048, 2049, 2048 + w] and c.w == w
        assert want.eb[0] == want.eb[1] == 0 and want.eb[2] <= 1 and want.eb[3] <= 2    # 2w-1: nothing, 2w: one position
        assert (want.njumps[4:] >= 1).all() and np.isinf(want.sigma[:4]).all()
        assert {R.AT, R.CLEAN} <= set(want.cls)
    assert R.stream_case("sizes_w1").radius == 0 and R.stream_case("sizes_w256").radius == 256
    # a jump w and w + 1 from the block edges: the first and last evaluable positions, and their neighbours
    c, want = R.stream_case("edge_jumps"), R.stream_expected("edge_jumps")
    assert want.pos.tolist() == [8, 300 + 9, 600 + 292, 900 + 291] and want.heights.tolist() == [5.0, 6.0, 7.0, 8.0]
    assert want.noeval[7] == 1 and want.noeval[8] == 0 and want.noeval[600 + 292] == 0 and want.noeval[600 + 293] == 1
    assert not want.d_out[:1200].any() and (want.d_out[1200:] == 1.0).all()           # the steps are gone exactly
    assert want.cls[0] == R.NEAR and want.cls[299] == R.CLEAN and want.cls[300] == R.NEAR and want.cls[899] == R.NEAR \
        and want.cls[900] == R.CLEAN                                                   # no NEAR across a block
    # min_count: 4 usable samples on the left are one too few, 5 are enough
    for name in ("min_count_int32", "min_count_bytes", "min_count_uint8", "min_count_prev", "min_count_flags_and_prev"):
        c, want = R.stream_case(name), R.stream_expected(name)
        use = R.usable(c.d, c.flags, c.prev)
        assert c.min_count == 5 and use[92:100].sum() == 4 and use[292:300].sum() == 5
        assert want.noeval[100] == 1 and want.noeval[300] == 0 and 300 in want.pos and 100 not in want.pos
        assert np.array_equal(want.t, R.stream_expected("min_count_int32").t)
    assert R.stream_case("min_count_bytes").flags.dtype == np.bool_
    assert R.stream_case("min_count_uint8").flags.dtype == np.uint8
    assert R.stream_case("min_count_prev").flags is None and R.stream_case("min_count_prev").prev.dtype == np.uint8
    # values
    c, want = R.stream_case("nonfinite"), R.stream_expected("nonfinite")
    assert not np.isfinite(c.d[[0, 499, 500, 832, 240, 251, 260]]).any() and np.isfinite(want.t).all()
    assert not np.isfinite(want.d_out[[0, 499, 500, 832, 240, 251, 260]]).any() and want.pos.size == 2
    c, want = R.stream_case("huge_pairs"), R.stream_expected("huge_pairs")
    assert want.noeval[90:100].all() and want.noeval[390:400].all()                    # the sums overflowed
    assert not want.noeval[590:600].any() and np.isfinite(want.t).all()                # this pair cancelled
    c, want = R.stream_case("subnormals"), R.stream_expected("subnormals")
    assert (np.abs(c.d) < 2.3e-308).all() and want.t.any() and (np.abs(want.t) < 2.3e-308).all()
    assert want.pos.tolist() == [250] and np.abs(want.d_out).max() < 1e-315
    want = R.stream_expected("constant")
    assert not want.sigma.any() and want.pos.size == 0 and not want.t.any()            # sigma 0, and still no jump
    want = R.stream_expected("scale_edges")
    assert want.eb.tolist() == [2, 3, 4] and np.isinf(want.sigma[0]) and np.isfinite(want.sigma[1:]).all()


def test_the_stated_sum_order_is_the_only_one_that_gives_the_expected_bits():
    c, want = R.stream_case("sum_order"), R.stream_expected("sum_order")
    assert R.TWO53 + 1.0 == R.TWO53 and (1.0 - R.TWO53) + R.TWO53 == 1.0
    # the window 100 .. 103 holds 2^53, 1, -2^53, 0: ascending 0, descending or pairwise 1
    assert ((R.TWO53 + 1.0) + -R.TWO53) + 0.0 == 0.0 and ((0.0 + -R.TWO53) + 1.0) + R.TWO53 == 1.0 \
        and (R.TWO53 + 1.0) + (-R.TWO53 + 0.0) == 0.0 and (R.TWO53 + -R.TWO53) + (1.0 + 0.0) == 1.0
    assert want.t[100] == 0.0 and want.t[104] == 0.0 and want.noeval[100] == 0
    # the window 200 .. 203 holds -2^53, 2^53, 1, 0: ascending 1, descending 0
    assert want.t[200] == 0.25 and want.t[204] == -0.25
    assert ((0.0 + 1.0) + R.TWO53) + -R.TWO53 == 0.0
    # the chain of the offsets
    want = R.peak_expected("offsets_order")
    assert want.heights.tolist() == [R.TWO53, 1.0, -R.TWO53, 1.0, -R.TWO53, R.TWO53]
    assert want.offsets.tolist() == [R.TWO53, R.TWO53, 0.0, 1.0, 1.0 - R.TWO53, 1.0]
    want = R.peak_expected("offsets_overflow")
    assert want.offsets[0] == 1.5e308 and np.isinf(want.offsets[1]) and np.isinf(want.offsets[2])


def test_peak_cases_are_what_they_say():
    assert set(R.PEAK_CASES) == set(R.peak_cases())
    want = R.peak_expected("threshold")
    assert want.pos.tolist() == [200, 300] and R.THR == 5.0 * 0.7                     # equality is no candidate
    w = 16
    want = R.peak_expected("ties")
    assert want.pos.tolist() == [100, 500, 900, 900 + w + 1, 1300 + w, 1700, 2100]
    want = R.peak_expected("ties_not_evaluable")
    assert want.pos.tolist() == [100, 300]                                            # a rival that is not evaluable is none
    want = R.peak_expected("tile_and_block_edges")
    assert want.pos.tolist() == [0, 2047, 2048 + w + 1, 4095, 4999, 5000, 7047, 7048, 9096]
    assert want.njumps.tolist() == [5, 2, 2]
    assert R.peak_expected("tile_edge_2048").pos.tolist() == [2048]
    assert R.peak_expected("tile_edge_2049").pos.tolist() == [2049]                   # 2049 - w, in the tile before, lost
    for radius in (0, 256):
        c, want = R.peak_case("radius_%d" % radius), R.peak_expected("radius_%d" % radius)
        assert want.pos.tolist() == [2047, 2100, 2199, 2200, 2350, 2500, 4400, 4547] and c.radius == radius
        assert want.cls[[2046, 2100, 2348, 4000]].tolist() == [3, 4, 2, 1]            # rule 9a first
        assert want.cls[2047] == want.cls[2199] == want.cls[2200] == R.AT
        if radius == 0:
            assert (want.cls == R.NEAR).sum() == 1                                    # the carried byte at 2348 only
        else:
            assert want.cls[2047 - 256] == R.NEAR and want.cls[2047 - 257] == R.CLEAN
            assert (want.cls[2201:2350] == R.NEAR).all() and (want.cls[2351:2500] == R.NEAR).all()   # all of block 1
            assert want.cls[2500 + 256] == R.NEAR and want.cls[2500 + 257] == R.CLEAN
            assert want.cls[4400 - 256] == R.NEAR and want.cls[4400 - 257] == R.CLEAN and want.cls[4546] == R.NEAR
    want = R.peak_expected("no_jump")
    assert want.pos.size == 0 and want.counts.tolist() == [[700, 0, 0], [3, 0, 0]]
    want = R.peak_expected("many")
    assert want.njumps.tolist() == [601, 20, 400] and want.pos.size == 1021


def test_iteration_case_needs_its_second_pass():
    c = R.iteration_case()
    each = c.info["each"]
    assert c.info["passes"] == 3 and [p.pos.size for p in each] == [1, 1, 0]
    assert abs(each[0].pos[0] - 700) <= 3 and abs(each[1].pos[0] - 716) <= 3 and each[1].pos[0] - each[0].pos[0] <= c.w
    assert each[0].cls[each[0].pos[0]] == R.AT and c.cls[each[0].pos[0]] == R.AT      # carried by rule 9a
    assert c.cls[each[1].pos[0]] == R.AT and abs(c.d_out[800:1500].mean() - c.d[:600].mean()) < 1.0
    assert abs(each[0].d_out[800:1500].mean() - c.d[:600].mean()) > 2.0                # one pass leaves a step
    print("iteration case: seed %d, positions %s, heights %s" % (c.seed, c.info["positions"], c.info["heights"]))


# ------------------------------------------------------------------ detection quality ----
def test_the_definition_finds_the_jumps_of_a_one_over_f_stream():
    q, e = R.quality_case(), R.quality_expected()
    pos, heights, sigma = e.info["positions"], e.info["heights"], e.info["sigma"][0]
    order = np.argsort(pos)
    pos, heights = pos[order], heights[order]
    assert q.where.size == 24 and len(q.sizes) == 4 and abs((q.pix < 0).mean() - 0.03) < 0.005
    assert sorted(set(np.abs(q.heights))) == [3.0, 5.0, 8.0, 20.0]
    e_ = R.edges(q.sizes)
    blk = np.searchsorted(e_, q.where, side="right") - 1
    assert (np.bincount(blk) == 6).all() and (np.diff(q.where)[np.diff(blk) == 0] >= 3 * q.w).all()
    assert (q.where - e_[blk] >= 3 * q.w).all() and (e_[blk + 1] - q.where >= 3 * q.w).all()
    clean, raw, fixed = (R.low_bin_power(x, q.sizes) for x in (q.clean, q.d, e.d_out))
    err = np.abs(heights - q.heights) / sigma[blk] if pos.size == 24 else np.array([np.inf])
    print("quality, seed %d: %d jumps found in %d passes, position error <= %d, height error <= %.2f sigma_b, sigma_b %s,"
          " low bins: corrected / clean %.2f, uncorrected / corrected %.0f"
          % (R.QUALITY_SEED, pos.size, e.info["passes"], np.abs(pos - q.where).max() if pos.size == 24 else -1,
             err.max(), np.round(sigma, 3).tolist(), fixed / clean, raw / fixed))
    assert pos.size == 24 and (np.abs(pos - q.where) <= 3).all()          # every jump within 3 samples, no other
    assert (err <= 6.0).all()                                             # within the detector's own threshold
    assert fixed <= 20.0 * clean and raw >= 100.0 * fixed


def test_the_end_to_end_case_meets_the_same_conditions():
    q, e = R.quality_case(glitches=40), R.end_to_end_expected()
    assert q.spikes.size == 40 and (q.pix[q.spikes] >= 0).all() and (e.gcls[q.spikes] == 3).all()
    pos = np.sort(e.info["positions"])
    assert pos.size == 24 and (np.abs(pos - q.where) <= 3).all()
    assert (e.cls[e.gcls != 0] == e.gcls[e.gcls != 0]).all() and (e.cls[pos] != 0).all()
    clean, raw, fixed = (R.low_bin_power(x, q.sizes) for x in (q.clean, q.d, e.d_out))
    assert fixed <= 20.0 * clean and raw >= 100.0 * fixed


# ------------------------------------------------------------------ names and header ----
def test_names_are_exported_and_the_header_declares_the_entry_points():
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, build as B, kernel_resources as KR
    from cosmomap2_amd.utilities import jumps as J
    for name in ("JumpCorrector", "correct_jumps"):
        assert callable(getattr(U, name)) and name in J.__all__
    assert U.JUMP_CLASSES == ("clean", "jump", "near") == R.CLASSES
    for name in ("statistic", "scale", "find", "correct", "run"):
        assert callable(getattr(U.JumpCorrector, name))
    hdr = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint cm2_jump_%s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_hip.PROTOTYPES["cm2_jump_" + name]), name
        assert ("cm2_jump_" + name in _hip.RESTARTABLE) == (name != "correct"), name       # correct may run in place
    assert re.search(r"#define CM2_JUMP_MAX_WINDOW 256\b", hdr) and R.MAX_W == J.MAX_WINDOW == 256
    assert re.search(r"#define CM2_JUMP_MAX_RADIUS 256\b", hdr) and R.MAX_RADIUS == J.MAX_RADIUS == 256
    for code, name in enumerate(("CLEAN", "AT", "NEAR")):
        assert re.search(r"#define CM2_JUMP_%s %d\b" % (name, code), hdr)
        assert getattr(R, name) == getattr(J, name) == code
    assert hdr.index("---- f2e:") < hdr.index("---- f2f:") < hdr.index("---- f3:")
    for k in ("k_jump_stat", "k_jump_peaks", "k_jump_offsets", "k_jump_correct"):
        assert any(re.search(p, k) for p in KR.NO_SPILL), k
    assert "cm2_jump.hip" not in B.FMA_OK
    src = open(os.path.join(CSRC, "cm2_jump.hip")).read()
    atomics = set(re.findall(r"\batomic\w*\s*\(\s*&?\s*(\w+)", src))                      # integer tallies only
    assert atomics == {"tally", "njumps", "counts"}
    assert re.search(r"unsigned int tally", src) and re.search(r"unsigned long long \*__restrict__ njumps", src) \
        and re.search(r"unsigned long long \*__restrict__ counts", src)
    body = src.split('#include "cm2_common.h"')[1]
    assert re.findall(r"__shfl\w*\((\w+)", body) == ["incl"] and re.search(r"unsigned int incl", body)   # integers only
    assert "fmin" not in body and "fmax" not in body and "fma(" not in body
    assert "cm2_glitch_scale(" in body and "k_glitch" not in body                         # no second selection


def test_the_built_kernels_use_no_scratch():
    from cosmomap2_amd import build as B, kernel_resources as KR
    B.build(verbose=False)
    rows = {r["kernel"]: r for r in KR.load_all() if r["unit"] == "cm2_jump"}
    own = {k: v for k, v in rows.items() if k.startswith("k_jump_")}
    table = open(os.path.join(ROOT, "profiles", "kernel_resources.md")).read()
    want = ["k_jump_stat", "k_jump_peaks", "k_jump_offsets", "k_jump_correct"]
    assert sorted(own) == sorted(want)
    for k in want:
        assert own[k].get("scratch_bytes_per_lane", 0) == 0 and own[k].get("vgpr_spill", 0) == 0, own[k]
        assert "`%s`" % k in table, k
    # the nine sums of a thread are in registers (two each) and leave room for 8 waves a SIMD
    assert 2 * R.STARTS <= own["k_jump_stat"]["vgpr"] <= 64 and own["k_jump_stat"]["occupancy"] >= 8
    assert own["k_jump_peaks"]["lds_bytes"] >= (R.TILE + 2 * R.MAX_W) * 8


def test_null_arguments_are_refused_without_a_gpu():
    from cosmomap2_amd import _hip
    lib = _hip.load()
    assert lib.cm2_jump_destroy(None) == 0
    for name in ENTRY_POINTS:
        if name == "destroy":
            continue
        args = [0 if a in (ctypes.c_int, ctypes.c_int64) else 0.0 if a is ctypes.c_double else None
                for a in _hip.PROTOTYPES["cm2_jump_" + name]]
        assert getattr(lib, "cm2_jump_" + name)(*args) == _hip.ERR_ARGUMENT, name
        assert b"cm2_jump_" + name.encode() in lib.cm2_last_error(), (name, lib.cm2_last_error())
    h = ctypes.c_void_p()

    def create(nt, sizes, w):
        sz = (ctypes.c_int64 * len(sizes))(*sizes)
        return lib.cm2_jump_create(ctypes.byref(h), nt, sz, len(sizes), w, None), lib.cm2_last_error()

    for args, word in (((100, [100], 0), b"half_window"), ((100, [100], 257), b"half_window"),
                       ((2 ** 32 - 1, [2 ** 32 - 1], 4), b"32-bit"), ((100, [60, 30], 4), b"add up"),
                       ((100, [60, 50], 4), b"add up"), ((100, [100, 0], 4), b"add up"), ((0, [1], 4), b"nt=")):
        rc, msg = create(*args)
        assert rc == _hip.ERR_ARGUMENT and b"cm2_jump_create" in msg and word in msg, (args, rc, msg)
        assert not h.value


# ----------------------------------------------------- the policy header, on a CPU ----
DRIVER = r"""
#include "cm2_jump_policy.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace cm2::jump;
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "constants")) {
        printf("%d %d %d %d %d %d %d %lld %lld\n", kMaxWindow, kMaxRadius, kTile, kTileThreads, kCounts, kStarts,
               stat_starts(), (long long)kMaxBlocks, (long long)peaks_lds_bytes());
        printf("%d %d %d\n", (int)kClean, (int)kAt, (int)kNear);
        for (int w = 1; w <= kMaxWindow; ++w) printf("%d %lld\n", stat_values(w), (long long)stat_lds_bytes(w));
        return 0;
    }
    if (!strcmp(argv[1], "checks")) {             // checks w have_flags kind min_count nsigma capacity radius
        printf("%d %d %d\n", (int)check_stat(atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4]), atoi(argv[5])),
               (int)check_find(atof(argv[6]), atoll(argv[7])), (int)check_correct(atoi(argv[8]), atoll(argv[7])));
        return 0;
    }
    if (!strcmp(argv[1], "table")) {              // table x p0 p1 ...: entries < x, entries <= x
        std::vector<int64_t> p;
        for (int i = 3; i < argc; ++i) p.push_back(atoll(argv[i]));
        printf("%lld %lld\n", (long long)table_lower(p.data(), (int64_t)p.size(), atoll(argv[2])),
               (long long)table_upper(p.data(), (int64_t)p.size(), atoll(argv[2])));
        return 0;
    }
    // create nt w s0 s1 ...   (no sizes: a null pointer)
    // ones n w [nt]             n blocks of one sample, nt = n unless given
    std::vector<int64_t> s;
    for (int i = 4; i < argc; ++i) s.push_back(atoll(argv[i]));
    if (!strcmp(argv[1], "ones")) s.assign((size_t)atoll(argv[2]), 1);
    Launch l;
    const int64_t nt = atoll(argv[!strcmp(argv[1], "ones") && argc > 4 ? 4 : 2]);
    const Status st = check_create(&l, nt, s.empty() ? nullptr : s.data(), (int64_t)s.size(), atoi(argv[3]));
    printf("%d\n", (int)st);
    if (st != kOk || strcmp(argv[1], "create")) return 0;
    printf("%lld %lld %lld %d %lld\n", (long long)l.nt, (long long)l.nblocks, (long long)l.tiles, l.w,
           (long long)l.lds_bytes);
    std::vector<int64_t> off(s.size() + 1, 0), ts(s.size() + 1, 0);
    for (size_t b = 0; b < s.size(); ++b) {
        off[b + 1] = off[b] + s[b];
        ts[b + 1] = ts[b] + tiles_of(s[b]);
    }
    for (int64_t g = 0; g < l.tiles; ++g) {
        const Span sp = tile_span(off.data(), ts.data(), l.nblocks, g);
        printf("t %lld %lld %lld\n", (long long)sp.block, (long long)sp.first, (long long)sp.end);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("jump_policy")
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
    assert [int(x) for x in out[0]] == [256, 256, R.TILE, R.TILE_THREADS, 3, R.STARTS, R.STARTS * R.TILE_THREADS,
                                        1 << 18, (R.TILE + 512) * 8]
    assert [int(x) for x in out[1]] == [R.CLEAN, R.AT, R.NEAR]
    assert R.STARTS * R.TILE_THREADS >= R.TILE + R.MAX_W > (R.STARTS - 1) * R.TILE_THREADS      # a thread per start
    for w in range(1, 257):
        values, lds = [int(x) for x in out[1 + w]]
        # the last start of the last round reads w samples; the last position reads the count at q + 2 w
        assert values == R.STARTS * R.TILE_THREADS + w >= R.TILE + 2 * w and values < 65536
        assert lds == R.stat_lds_bytes(w) >= values * 8 + R.STARTS * R.TILE_THREADS * 8 + (values + 1) * 2
        assert lds <= 64 * 1024 and lds % 8 == 0
    assert R.stat_lds_bytes(256) == 44040 and 3 * R.stat_lds_bytes(256) <= 160 * 1024           # three a CU


SIZE_SETS = [[1], [1, 2, 63, 64, 65, 131], [2047, 2048, 2049, 1, 4097], [2048 + 256, 511, 512, 513], [7] * 40, [100000]]


@pytest.mark.parametrize("sizes", SIZE_SETS)
@pytest.mark.parametrize("w", [1, 64, 256])
def test_tiles_cover_every_position_exactly_once(driver, sizes, w):
    nt = sum(sizes)
    out = _run(driver, "create", nt, w, *sizes)
    assert out[0] == ["0"]
    tiles = sum(-(-s // R.TILE) for s in sizes)
    assert [int(x) for x in out[1]] == [nt, len(sizes), tiles, w, R.stat_lds_bytes(w)]
    e = R.edges(sizes)
    spans = [[int(x) for x in ln[1:]] for ln in out[2:] if ln[0] == "t"]
    assert len(spans) == tiles
    seen = np.zeros(nt, dtype=np.int64)
    for b, first, end in spans:
        assert e[b] <= first < end <= e[b + 1] and end - first <= R.TILE                  # never crosses a block
        assert (first - e[b]) % R.TILE == 0 and (end - first == R.TILE or end == e[b + 1])
        seen[first:end] += 1
    assert (seen == 1).all() and spans == sorted(spans, key=lambda s: s[1])


def test_policy_status_codes(driver):
    def create(nt, w, *sizes):
        return int(_run(driver, "status", nt, w, *sizes)[0][0])
    assert create(100, 4, 60, 40) == 0
    assert create(0, 4, 1) == 1 and create(100, 4) == 1 and create(-5, 4, 1) == 1                  # kBadSize
    assert create(100, 4, 60, 30) == 2 and create(100, 4, 60, 50) == 2 and create(100, 4, 100, 0) == 2
    assert create(100, 4, 101, -1) == 2 and create(2, 4, 1, 1, 1) == 2                             # kBadBlocks
    assert create(100, 0, 100) == 3 and create(100, 257, 100) == 3 and create(100, -1, 100) == 3   # kBadWindow
    assert create(100, 1, 100) == 0 and create(100, 256, 100) == 0
    assert create(2 ** 32 - 1, 4, 2 ** 32 - 1) == 4 and create(2 ** 32 - 2, 4, 2 ** 32 - 2) == 0   # kTooLarge
    assert _run(driver, "ones", (1 << 18) + 1, 4)[0] == ["5"] and _run(driver, "ones", 1 << 18, 4)[0] == ["0"]
    # two faults at once: size, then window, then the 32-bit limit, then the blocks, then their number
    assert create(2 ** 32 - 1, 0, 2 ** 32 - 1) == 3 and create(0, 0, 1) == 1
    assert _run(driver, "ones", (1 << 18) + 1, 4, (1 << 18) + 2)[0] == ["2"]

    def checks(w=8, have=0, kind=0, min_count=4, nsigma=6.0, capacity=10, radius=4):
        return [int(x) for x in _run(driver, "checks", w, have, kind, min_count, nsigma, capacity, radius)[0]]
    assert checks() == [0, 0, 0] and checks(min_count=1) == [0, 0, 0] and checks(min_count=8) == [0, 0, 0]
    assert checks(min_count=0)[0] == 9 and checks(min_count=9)[0] == 9                             # kBadMinCount
    assert checks(have=1, kind=2)[0] == 8 and checks(have=1, kind=-1)[0] == 8                      # kBadFlagKind
    assert checks(have=1, kind=1)[0] == 0 and checks(have=0, kind=7)[0] == 0
    for bad in (0.0, -1.0, "nan", "inf"):
        assert checks(nsigma=bad)[1] == 6                                                          # kBadNsigma
    assert checks(nsigma=1e-300)[1] == 0 and checks(nsigma=1e308)[1] == 0
    assert checks(capacity=0)[1:] == [10, 10] and checks(capacity=1)[1:] == [0, 0]                 # kBadCapacity
    assert checks(radius=-1)[2] == 7 and checks(radius=257)[2] == 7                                # kBadRadius
    assert checks(radius=0)[2] == 0 and checks(radius=256)[2] == 0


def test_policy_table_bisection(driver):
    pos = [3, 7, 7, 20, 4000000000]
    for x in (-1, 0, 3, 4, 7, 8, 20, 21, 4000000000, 4000000001):
        want = [sum(p < x for p in pos), sum(p <= x for p in pos)]
        assert [int(v) for v in _run(driver, "table", x, *pos)[0]] == want, x
    assert _run(driver, "table", 5)[0] == ["0", "0"]


# ------------------------------------------------------ the Python layer's checks ----
def test_arguments_are_refused_before_the_gpu_is_needed():
    import torch
    from cosmomap2_amd import _hip
    from cosmomap2_amd.utilities import JumpCorrector, correct_jumps
    d = np.zeros(100)
    pix = np.zeros(100, dtype=np.int32)
    cls = np.zeros(100, dtype=np.uint8)
    for kw in (dict(half_window=0), dict(half_window=257), dict(half_window=2.5), dict(half_window=True)):
        with pytest.raises(ValueError):
            JumpCorrector(10, **kw)
    for bs in (0, -3, 2.5, [], [10, 0], [10, -1], [2.5]):
        with pytest.raises(ValueError):
            JumpCorrector(bs)
    jc = JumpCorrector(50, half_window=4)
    for bad in (dict(nsigma=0), dict(nsigma=-1.0), dict(nsigma=float("nan")), dict(nsigma=float("inf")),
                dict(nsigma="x"), dict(radius=-1), dict(radius=257), dict(radius=1.5), dict(iterations=0),
                dict(iterations=9), dict(iterations=2.0), dict(sigma=[1.0, 2.0, 3.0]), dict(sigma=-1.0),
                dict(sigma=float("nan")), dict(sigma=np.ones((2, 1))), dict(flags=pix[:50]),
                dict(flags=np.zeros(100)), dict(flags=np.zeros((10, 10), dtype=np.int32)), dict(min_count=0),
                dict(min_count=5), dict(min_count=1.5), dict(capacity=0), dict(capacity=2.5), dict(classes=cls[:99]),
                dict(classes=cls.astype(np.int32)), dict(classes=cls.reshape(100, 1)), dict(out=np.zeros(99)),
                dict(out=np.zeros(100, dtype=np.float32)), dict(out=torch.zeros(100, dtype=torch.float64)),
                dict(out=[0.0] * 100)):
        with pytest.raises(ValueError) as e:
            jc.run(d, **bad)
        assert str(e.value), bad
        with pytest.raises(ValueError):
            correct_jumps(d, 50, half_window=4, **bad)
    for bad_d in (np.zeros(95), np.zeros((10, 10)), np.zeros(0), np.zeros(100, dtype=complex),
                  torch.zeros(100, dtype=torch.float32), torch.zeros(100, dtype=torch.float64)):   # (a host tensor)
        with pytest.raises(ValueError):
            jc.run(bad_d)
        with pytest.raises(ValueError):
            jc.statistic(bad_d)
    with pytest.raises(ValueError):
        JumpCorrector([60, 30], 4).run(d)                        # the sizes do not add up to the stream
    with pytest.raises(ValueError):
        jc.statistic(d, min_count=5)
    with pytest.raises(ValueError):
        jc.statistic(d, classes=cls[:99])
    for call in (lambda: jc.scale(d, cls), lambda: jc.find(d, cls, 1.0), lambda: jc.correct(d, (1, 2, 3)),
                 lambda: jc.correct(d, None, radius=300)):
        with pytest.raises(ValueError):                          # t and noeval are the tensors statistic() returned
            call()
    with pytest.raises(ValueError):
        jc.info(95)
    if not torch.cuda.is_available():
        for call in (lambda: jc.run(d, flags=pix, classes=cls), lambda: jc.statistic(d), lambda: jc.info(100),
                     lambda: correct_jumps(d, 50)):
            with pytest.raises(_hip.HipError):
                call()


# ------------------------------------------- which arrays of a call may share memory ----
DISJOINT_DRIVER = r"""
#include "cm2_stream_policy.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace cm2::stream;
// nout nin alias_out alias_in, then address and bytes of every output and of every input (address 0: NULL)
int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int nout = atoi(argv[1]), nin = atoi(argv[2]);
    if (argc != 5 + 2 * (nout + nin)) return 2;
    std::vector<Range> r;
    for (int i = 5; i < argc; i += 2)
        r.push_back(Range{reinterpret_cast<const void *>((uintptr_t)strtoull(argv[i], nullptr, 10)),
                          (uint64_t)strtoull(argv[i + 1], nullptr, 10)});
    printf("%d\n", (int)disjoint(r.data(), nout, r.data() + nout, nin, atoi(argv[3]), atoi(argv[4])));
    return 0;
}
"""


@pytest.fixture(scope="module")
def disjoint(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_policy")
    src = d / "disjoint.cpp"
    src.write_text(DISJOINT_DRIVER)
    exe = str(d / "disjoint")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])

    def run(outs, ins, alias=(-1, -1)):
        flat = [v for r in list(outs) + list(ins) for v in r]
        return int(_run(exe, len(outs), len(ins), alias[0], alias[1], *flat)[0][0])
    return run


def test_disjoint_outputs_and_inputs(disjoint):
    OK, ON_INPUT, ON_OUTPUT = 0, 1, 2
    A, B, C = 1 << 20, 1 << 21, 1 << 22
    assert disjoint([(A, 800)], [(B, 800), (C, 100)]) == OK
    # a NULL range overlaps nothing, whatever its length, as an input and as an output
    assert disjoint([(A, 800)], [(0, 1 << 40), (B, 8)]) == OK and disjoint([(0, 1 << 40), (A, 8)], [(A + 8, 8)]) == OK
    assert disjoint([(0, 1 << 40)], [(0, 1 << 40)]) == OK
    # adjacent: the last byte of one next to the first of the other, on either side
    assert disjoint([(A, 800)], [(A + 800, 800)]) == OK and disjoint([(A, 800)], [(A - 800, 800)]) == OK
    # one shared byte, on either side; a range inside the other; the same range
    assert disjoint([(A, 800)], [(A + 799, 800)]) == ON_INPUT and disjoint([(A, 800)], [(A - 799, 800)]) == ON_INPUT
    assert disjoint([(A, 800)], [(A + 8, 8)]) == ON_INPUT and disjoint([(A + 8, 8)], [(A, 800)]) == ON_INPUT
    assert disjoint([(A, 800)], [(A, 800)]) == ON_INPUT
    # every input is looked at, and every output
    assert disjoint([(A, 800)], [(B, 8), (C, 8), (A + 792, 8)]) == ON_INPUT
    assert disjoint([(B, 8), (A, 800)], [(C, 8), (A + 792, 8)]) == ON_INPUT
    # output against output: adjacent, one shared byte, the last pair of three
    assert disjoint([(A, 800), (A + 800, 100)], [(B, 8)]) == OK
    assert disjoint([(A, 800), (A + 799, 100)], [(B, 8)]) == ON_OUTPUT
    assert disjoint([(C, 8), (A, 800), (A + 799, 100)], []) == ON_OUTPUT
    # the first pair in the order of the outputs decides: output 0 meets output 1 before output 1 meets an input
    assert disjoint([(A, 800), (A + 8, 8)], [(A + 8, 8)]) == ON_INPUT
    assert disjoint([(A, 800), (B, 8)], [(B, 8)]) == ON_INPUT and disjoint([(A, 800), (A, 8)], [(B, 8)]) == ON_OUTPUT
    # the one pair that may alias: the same pointer only (cm2_jump_correct's d_out == d_in, 8-byte elements)
    assert disjoint([(A, 800), (B, 100)], [(A, 800), (C, 100)], alias=(0, 0)) == OK
    assert disjoint([(A, 800), (B, 100)], [(A + 8, 800), (C, 100)], alias=(0, 0)) == ON_INPUT
    assert disjoint([(A, 800), (B, 100)], [(A - 8, 800), (C, 100)], alias=(0, 0)) == ON_INPUT
    assert disjoint([(A, 800), (B, 100)], [(C, 100), (A, 800)], alias=(0, 0)) == ON_INPUT      # another input
    assert disjoint([(B, 100), (A, 800)], [(A, 800), (C, 100)], alias=(0, 0)) == ON_INPUT      # another output
    assert disjoint([(A, 800), (A, 100)], [(A, 800)], alias=(0, 0)) == ON_OUTPUT               # outputs never alias
