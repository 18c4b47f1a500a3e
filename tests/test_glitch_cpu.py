"""
The glitch flagger without a GPU: the NumPy restatement of _glitch_ref.py against an independent brute force on the
shared cases, the conditions the shared cases must meet, cm2_glitch_policy.h compiled with the host compiler and
checked against Python, the header's prototypes and constants, the exported names and every argument check of the
Python layer.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _glitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
ENTRY_POINTS = {"create": 6, "destroy": 1, "info": 2, "residual": 7, "scale": 8, "classify": 12, "apply_pix": 4}


# ------------------------------------------------- the restatement against a brute force ----
def brute_residual(c):
    """np.median per window (NumPy's own even-count mean replaced by the stated 0.5 a + 0.5 b)"""
    use, e, r = R.usable(c.d, c.flags, c.prev), R.edges(c.sizes), np.zeros(c.d.size)
    blk = np.repeat(np.arange(len(c.sizes)), c.sizes)
    idx = np.arange(c.d.size)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in np.flatnonzero(use):
            w = c.d[use & (blk == blk[i]) & (np.abs(idx - i) <= c.h)]
            if w.size & 1:
                med = np.median(w)
            else:
                part = np.partition(w, [w.size // 2 - 1, w.size // 2])
                med = 0.5 * part[w.size // 2 - 1] + 0.5 * part[w.size // 2]
            r[i] = c.d[i] - med
    assert e[-1] == c.d.size
    return r


def brute_scale(c, r):
    use, e, W = R.usable(c.d, c.flags, c.prev), R.edges(c.sizes), 2 * c.h + 1
    out = np.full(len(c.sizes), np.inf)
    for b in range(len(c.sizes)):
        a = np.abs(r[e[b]:e[b + 1]])[use[e[b]:e[b + 1]]]
        if a.size >= W:
            k = (a.size - 1) // 2
            out[b] = 1.4826 * np.partition(a, k)[k]
    return out


SMALL = [n for n in R.MEDIAN_CASES if not n.startswith("group_")]


@pytest.mark.parametrize("name", SMALL)
def test_restatement_against_brute_force(name):
    c, want = R.median_case(name), R.median_expected(name)
    r = brute_residual(c)
    assert np.array_equal(want.r == r, np.ones(r.size, dtype=bool))            # == : the sign of a zero is free
    assert np.array_equal(R.bits(want.sigma), R.bits(brute_scale(c, want.r)))
    assert not want.r[~R.usable(c.d, c.flags, c.prev)].any()


@pytest.mark.parametrize("name", R.SELECTION_CASES)
def test_selection_restatement_against_partition(name):
    c = R.selection_case(name)
    sigma, mb = R.scale(c.d, c.r, c.sizes, c.h, c.flags)
    assert np.array_equal(R.bits(sigma), R.bits(brute_scale(c, c.r)))
    assert np.array_equal(mb, [R.usable(c.d, c.flags)[a:b].sum() for a, b in zip(R.edges(c.sizes)[:-1],
                                                                               R.edges(c.sizes)[1:])])


def test_classes_against_a_vectorised_form():
    s = R.spike_case()
    for grow in (0, 1, 64):
        for sigma in (R.SIGMA_GIVEN, 0.0, np.inf):
            r = R.residual(s.d, s.sizes, s.h, s.flags)
            cls, counts = R.classify(s.d, r, s.sizes, [sigma] * 2, R.NSIGMA, grow, s.flags)
            use = R.usable(s.d, s.flags)
            blk = np.repeat(np.arange(2), s.sizes)
            hit = use & (np.abs(r) > R.NSIGMA * sigma)
            pos = np.flatnonzero(hit)
            near = np.array([((np.abs(pos - i) <= grow) & (pos != i) & (blk[pos] == blk[i])).any()
                             for i in range(s.d.size)])
            want = np.where(R.flagged(s.flags, s.d.size), R.INPUT,
                            np.where(~np.isfinite(s.d), R.NONFINITE, np.where(hit, R.HIT, np.where(near, R.NEAR, 0))))
            assert np.array_equal(cls, want)
            assert counts.sum(axis=1).tolist() == s.sizes


# ------------------------------------------------------- conditions on the shared cases ----
def test_median_cases_are_the_ones_the_issue_lists():
    assert R.H_EDGES == (1, 8, 9, 16, 17, 32, 33, 48, 49, 64)
    assert [R.tier_of(h) for h in R.H_EDGES] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    for h in R.H_EDGES:
        W = 2 * h + 1
        assert R.median_case("sizes_h%d" % h).sizes == [1, 2, h, h + 1, W - 1, W, W + 1, 63, 64, 65, 131]
    for h in (16, 49):
        c = R.median_case("group_h%d" % h)
        G = R.TIER_THREADS[R.tier_of(h)] * R.RUN
        assert c.sizes == [G, G - 1, G + 1, R.RUN] and G == 4096
    c = R.median_case("flags_runs")
    use = R.usable(c.d, c.flags)
    W = 2 * c.h + 1
    assert use[89] and not use[80:89].any() and not use[90:99].any()         # alone in its window
    assert R.median_expected("flags_runs").r[89] == 0.0
    assert not R.usable(R.median_case("flags_all").d, R.median_case("flags_all").flags).any()
    m = np.array([use[max(0, i - c.h):i + c.h + 1].sum() for i in range(100)])
    assert (m % 2 == 0).any() and (m % 2 == 1).any() and (m == W).any()
    c = R.median_case("three_integers")
    assert set(c.d) == {-1.0, 0.0, 1.0}
    c = R.median_case("huge_pairs")
    assert np.isfinite(R.median_expected("huge_pairs").r[100:140]).all()       # no overflow in the even median
    c = R.median_case("subnormals")
    assert (np.abs(c.d) < 2.3e-308).all() and c.d.any()
    c = R.median_case("nonfinite")
    assert not np.isfinite(c.d[[0, 199, 200, 276, 49, 75]]).any() and (c.flags[50:75] < 0).all()
    assert R.median_case("flags_bytes").flags.dtype == np.bool_ and R.median_case("flags_uint8").flags.dtype == np.uint8
    assert R.median_case("prev").prev.dtype == np.uint8 and set(R.median_case("prev").prev) == {0, 1, 2, 3, 4}


def test_selection_cases_are_what_they_say():
    c = R.selection_case("short_and_exact")
    sigma, mb = R.scale(c.d, c.r, c.sizes, c.h, c.flags)
    assert mb.tolist() == [6, 7, 8, 12, 0, 30] and 2 * c.h + 1 == 7
    assert np.isinf(sigma[[0, 4]]).all() and np.isfinite(sigma[[1, 2, 3, 5]]).all() and sigma[3] == 1.4826 * 0.75
    k = R.bits(np.abs(R.selection_case("lowest_digit").r))
    assert len(set(k >> np.uint64(11))) == 1 and len(set(k)) == 2048
    k = R.bits(R.selection_case("highest_digit").r)
    assert not (k & np.uint64((1 << 55) - 1)).any() and len(set(k >> np.uint64(55))) == 256
    for first in (True, False):
        keys, K = R._rank_edge_keys(first)
        for p in range(R.DIGITS):
            top = R.DIGIT_SHIFT[p] + R.DIGIT_BITS[p]
            same_prefix = keys[(keys >> np.uint64(top)) == (np.uint64(K) >> np.uint64(top))] if top < 64 else keys
            mine = same_prefix[(same_prefix >> np.uint64(R.DIGIT_SHIFT[p])) == (np.uint64(K) >> np.uint64(R.DIGIT_SHIFT[p]))]
            assert (mine.min() if first else mine.max()) == K and (p == R.DIGITS - 1 or mine.size > 1)
    assert len(R.selection_case("many_small_blocks").sizes) == 300
    assert R.selection_case("one_long_block").sizes == [20000] and 20000 > 9 * R.TILE
    assert set(R.SELECTION_CASES) == set(R.selection_cases())


def test_spikes_leave_the_residual_equal_to_the_data():
    s = R.spike_case()
    r = R.residual(s.d, s.sizes, s.h, s.flags)
    ok = np.isfinite(s.d) & (s.flags >= 0)
    assert np.array_equal(r[ok], s.d[ok]) and R.THR == 5.0 * 0.7
    cls, info = R.flag(s.d, s.sizes, s.h, s.flags, nsigma=R.NSIGMA, grow=1, iterations=1, sigma=R.SIGMA_GIVEN)
    assert cls[100] == cls[400] == R.CLEAN and cls[200] == cls[300] == R.HIT         # equality is no hit
    assert cls[2999] == R.HIT and cls[3000] == R.CLEAN and cls[2998] == R.NEAR       # no NEAR across the boundary
    assert cls[0] == R.HIT and cls[1] == R.NEAR and cls[-1] == R.HIT and cls[-2] == R.NEAR
    assert cls[R.TILE - 1] == R.HIT and cls[R.TILE] == R.NEAR and cls[R.TILE + 30] == R.HIT
    assert cls[999] == cls[1001] == R.INPUT and cls[1000] == R.HIT and cls[1500] == R.NONFINITE


def test_iteration_case_needs_its_second_pass():
    c = R.iteration_case()
    assert c.info["passes"] == 3 and c.info["hits_per_pass"][1] >= 1 and c.info["hits_per_pass"][2] == 0
    assert c.info["each"][0].sigma[0] > 1.2 * c.info["each"][1].sigma[0]              # the first MAD was inflated
    assert c.info["each"][0].cls[c.weak] == R.CLEAN and c.cls[c.weak] == R.HIT
    print("iteration case: seed %d, hits per pass %s, sigma per pass %s"
          % (c.seed, c.info["hits_per_pass"], [float(p.sigma[0]) for p in c.info["each"]]))


def test_end_to_end_case_meets_both_conditions_on_the_cpu():
    e = R.end_to_end()
    hits = np.flatnonzero(e.cls == R.HIT)
    elsewhere = np.setdiff1d(hits, e.where)
    print("end to end, seed %d: %d injected, %d found, %d other hits, sigma %s, passes %d"
          % (R.E2E_SEED, e.where.size, np.isin(e.where, hits).sum(), elsewhere.size,
             np.round(e.info["sigma"], 4).tolist(), e.info["passes"]))
    assert e.where.size == 40 and (e.pix[e.where] >= 0).all()
    assert np.isin(e.where, hits).all()                                    # 1. every injected position is a hit
    assert elsewhere.size <= 2                                             # 2. at most 2 hits elsewhere
    assert ((e.info["sigma"] > 0.9) & (e.info["sigma"] < 1.1)).all()
    assert abs((e.pix < 0).mean() - 0.03) < 0.005


# ------------------------------------------------------------------ names and header ----
def test_names_are_exported_and_the_header_declares_the_entry_points():
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, build as B, kernel_resources as KR
    from cosmomap2_amd.utilities import glitches as G
    for name in ("GlitchFlagger", "flag_glitches", "apply_flags"):
        assert callable(getattr(U, name)) and name in G.__all__
    assert U.GLITCH_CLASSES == ("clean", "input", "nonfinite", "hit", "near") == R.CLASSES
    hdr = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint cm2_glitch_%s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_hip.PROTOTYPES["cm2_glitch_" + name]), name
        assert ("cm2_glitch_" + name in _hip.RESTARTABLE) == (name != "apply_pix"), name
    assert re.search(r"#define CM2_GLITCH_MAD_TO_SIGMA 1\.4826\b", hdr) and R.MAD_TO_SIGMA == 1.4826
    assert re.search(r"#define CM2_GLITCH_MAX_HALF_WIDTH 64\b", hdr) and R.MAX_H == G.MAX_HALF_WIDTH == 64
    assert re.search(r"#define CM2_GLITCH_MAX_GROW 64\b", hdr) and R.MAX_GROW == G.MAX_GROW == 64
    assert G.MAX_ITERATIONS == R.MAX_ITER == 8
    for code, name in enumerate(("CLEAN", "INPUT", "NONFINITE", "HIT", "NEAR")):
        assert re.search(r"#define CM2_GLITCH_%s %d\b" % (name, code), hdr)
        assert getattr(R, name) == getattr(G, name) == code
    assert hdr.index("---- f2d:") < hdr.index("---- f2e:") < hdr.index("---- f3:")
    for k in ("k_glitch_median<33, 33, 64>", "k_glitch_median<129, 96, 64>", "k_glitch_hist", "k_glitch_pick",
              "k_glitch_classify", "k_glitch_apply_pix"):
        assert any(re.search(p, k) for p in KR.NO_SPILL), k
    assert "cm2_glitch.hip" not in B.FMA_OK
    src = open(os.path.join(CSRC, "cm2_glitch.hip")).read()
    atomics = set(re.findall(r"\batomic\w*\s*\(\s*&?\s*(\w+)", src))                # integer tallies only
    assert atomics == {"bins", "mine", "tally", "counts"}
    assert re.search(r"unsigned int bins\[", src) and re.search(r"unsigned int \*mine", src) \
        and re.search(r"unsigned int tally\[", src) and re.search(r"unsigned long long \*__restrict__ counts", src)
    body = src.split('#include "cm2_common.h"')[1]
    assert "shfl" not in body and "fmin" not in body and "fmax" not in body       # no cross-lane doubles; bits kept


def test_the_built_kernels_use_no_scratch():
    from cosmomap2_amd import build as B, kernel_resources as KR
    B.build(verbose=False)
    rows = {r["kernel"]: r for r in KR.load_all() if r["unit"] == "cm2_glitch"}
    table = open(os.path.join(ROOT, "profiles", "kernel_resources.md")).read()
    want = ["k_glitch_median<%d, %d, %d>" % (2 * R.TIER_MAX_H[t] + 1, R.REGISTER_SLOTS[t], R.TIER_THREADS[t])
            for t in range(5)] + ["k_glitch_hist", "k_glitch_pick", "k_glitch_classify", "k_glitch_apply_pix"]
    assert sorted(rows) == sorted(want)
    for k in want:
        assert rows[k].get("scratch_bytes_per_lane", 0) == 0 and rows[k].get("vgpr_spill", 0) == 0, rows[k]
        assert "`%s`" % k in table, k
    # the windows of tiers 0-2 are in registers: two per key at the least, and enough left for 3 waves a SIMD
    for t in range(3):
        assert 2 * (2 * R.TIER_MAX_H[t] + 1) <= rows[want[t]]["vgpr"] <= 168, rows[want[t]]
        assert rows[want[t]]["occupancy"] >= 3
    for t in (3, 4):
        assert 2 * R.REGISTER_SLOTS[t] <= rows[want[t]]["vgpr"] <= 256 and rows[want[t]]["occupancy"] >= 2


def test_null_arguments_are_refused_without_a_gpu():
    from cosmomap2_amd import _hip
    lib = _hip.load()
    assert lib.cm2_glitch_destroy(None) == 0
    for name in ENTRY_POINTS:
        if name == "destroy":
            continue
        args = [0 if a in (ctypes.c_int, ctypes.c_int64) else 0.0 if a is ctypes.c_double else None
                for a in _hip.PROTOTYPES["cm2_glitch_" + name]]
        assert getattr(lib, "cm2_glitch_" + name)(*args) == _hip.ERR_ARGUMENT, name
        assert b"cm2_glitch_" + name.encode() in lib.cm2_last_error(), (name, lib.cm2_last_error())
    h = ctypes.c_void_p()

    def create(nt, sizes, hw):
        sz = (ctypes.c_int64 * len(sizes))(*sizes)
        return lib.cm2_glitch_create(ctypes.byref(h), nt, sz, len(sizes), hw, None), lib.cm2_last_error()

    for args, word in (((100, [100], 0), b"half_width"), ((100, [100], 65), b"half_width"),
                       ((2 ** 32 - 1, [2 ** 32 - 1], 4), b"32-bit"), ((100, [60, 30], 4), b"add up"),
                       ((100, [60, 50], 4), b"add up"), ((100, [100, 0], 4), b"add up"), ((0, [1], 4), b"nt=")):
        rc, msg = create(*args)
        assert rc == _hip.ERR_ARGUMENT and b"cm2_glitch_create" in msg and word in msg, (args, rc, msg)
        assert not h.value
    pix, cls = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)         # never read: refused first
    assert lib.cm2_glitch_apply_pix(2 ** 32 - 1, cls, pix, None) == _hip.ERR_ARGUMENT
    assert lib.cm2_glitch_apply_pix(100, pix, pix, None) == _hip.ERR_ARGUMENT and b"overlap" in lib.cm2_last_error()


# ----------------------------------------------------- the policy header, on a CPU ----
DRIVER = r"""
#include "cm2_glitch_policy.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace cm2::glitch;
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "constants")) {
        printf("%d %d %d %d %d %d %d %d %d %d\n", kMaxHalfWidth, kMaxGrow, kRun, kTile, kTileThreads, kClasses, kDigits,
               kMaxBins, kTiers, kChunk);
        printf("%d %d %d %d %d\n", (int)kClean, (int)kInput, (int)kNonfinite, (int)kHit, (int)kNear);
        for (int p = 0; p < kDigits; ++p)
            printf("%d %d %d %llu\n", digit_bits(p), digit_shift(p), digit_bins(p), (unsigned long long)prefix_mask(p));
        for (int h = 1; h <= kMaxHalfWidth; ++h) {
            const int t = tier_of(h);
            printf("%d %d %d %d %d %d %lld %lld\n", t, tier_max_h(t), tier_slots(t), (int)tier_in_registers(t),
                   tier_threads(t), tier_key_registers(t), (long long)tier_lds_bytes(t, h),
                   (long long)stage_lds_bytes(t));
        }
        return 0;
    }
    if (!strcmp(argv[1], "classify")) {           // classify nsigma grow have_flags kind
        printf("%d %d\n", (int)check_classify(atof(argv[2]), atoi(argv[3])),
               (int)check_flag_kind(atoi(argv[4]) != 0, atoi(argv[5])));
        return 0;
    }
    // create nt h s0 s1 ...   (no sizes: a null pointer)
    // ones n h [nt]             n blocks of one sample, nt = n unless given
    std::vector<int64_t> s;
    for (int i = 4; i < argc; ++i) s.push_back(atoll(argv[i]));
    if (!strcmp(argv[1], "ones")) s.assign((size_t)atoll(argv[2]), 1);
    Launch l;
    const int64_t nt = atoll(argv[!strcmp(argv[1], "ones") && argc > 4 ? 4 : 2]);
    const Status st = check_create(&l, nt, s.empty() ? nullptr : s.data(), (int64_t)s.size(), atoi(argv[3]));
    printf("%d\n", (int)st);
    if (st != kOk || strcmp(argv[1], "create")) return 0;
    printf("%lld %lld %lld %lld %d %d %d %lld %lld %lld\n", (long long)l.nt, (long long)l.nblocks, (long long)l.runs,
           (long long)l.tiles, l.h, l.tier, l.threads, (long long)l.median_blocks, (long long)l.lds_bytes,
           (long long)l.hist_bytes);
    std::vector<int64_t> off(s.size() + 1, 0), rs(s.size() + 1, 0), ts(s.size() + 1, 0);
    for (size_t b = 0; b < s.size(); ++b) {
        off[b + 1] = off[b] + s[b];
        rs[b + 1] = rs[b] + runs_of(s[b]);
        ts[b + 1] = ts[b] + tiles_of(s[b]);
    }
    for (int64_t g = 0; g < l.runs; ++g) {
        const Span sp = run_span(off.data(), rs.data(), l.nblocks, g);
        printf("r %lld %lld %lld\n", (long long)sp.block, (long long)sp.first, (long long)sp.end);
    }
    for (int64_t w = 0; w < l.tiles; ++w) {
        const Span sp = tile_span(off.data(), ts.data(), l.nblocks, w);
        printf("t %lld %lld %lld\n", (long long)sp.block, (long long)sp.first, (long long)sp.end);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("glitch_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [ln.split() for ln in p.stdout.splitlines()]


def test_policy_constants_digits_and_tiers(driver):
    out = _run(driver, "constants")
    assert [int(x) for x in out[0]] == [64, 64, R.RUN, R.TILE, R.TILE_THREADS, 5, R.DIGITS, R.MAX_BINS, 5, R.CHUNK]
    assert R.RUN % R.CHUNK == 0 and 64 % R.CHUNK == 0
    assert [int(x) for x in out[1]] == [R.CLEAN, R.INPUT, R.NONFINITE, R.HIT, R.NEAR]
    covered = 0
    for p in range(R.DIGITS):
        nbits, shift, bins, mask = [int(x) for x in out[2 + p]]
        assert (nbits, shift) == (R.DIGIT_BITS[p], R.DIGIT_SHIFT[p]) and bins == 1 << nbits <= R.MAX_BINS
        assert bins % R.TILE_THREADS == 0                                  # k_glitch_pick: whole bins per thread
        digit = ((1 << nbits) - 1) << shift
        assert covered & digit == 0 and mask == covered                    # the prefix: exactly the digits before
        covered |= digit
    assert covered == (1 << 63) - 1                                        # 63 bits, each exactly once
    for h in range(1, 65):
        t, top, slots, regs, threads, kregs, lds, stage = [int(x) for x in out[2 + R.DIGITS + h - 1]]
        assert stage == threads * (3 * (R.CHUNK + 1) * 8 + 4 * 8)
        assert t == R.tier_of(h) and top == R.TIER_MAX_H[t] and h <= top and (t == 0 or h > R.TIER_MAX_H[t - 1])
        assert slots == 2 * top + 1 >= 2 * h + 1 and threads == R.TIER_THREADS[t]
        assert regs == (t < 4) and kregs == 2 * R.REGISTER_SLOTS[t]
        assert lds == (0 if regs else (2 * h + 1 - 96) * threads * 8) and lds + stage <= 160 * 1024 // 2   # two a CU


SIZE_SETS = [[1], [1, 2, 63, 64, 65, 131], [64, 64, 128], [2047, 2048, 2049, 1, 4097], [16384, 16383, 16385, 64],
             [7] * 40, [100000]]


@pytest.mark.parametrize("sizes", SIZE_SETS)
@pytest.mark.parametrize("h", [4, 40, 56])
def test_runs_and_tiles_cover_every_sample_exactly_once(driver, sizes, h):
    nt = sum(sizes)
    out = _run(driver, "create", nt, h, *sizes)
    assert out[0] == ["0"]
    runs = sum(-(-s // R.RUN) for s in sizes)
    tiles = sum(-(-s // R.TILE) for s in sizes)
    t = R.tier_of(h)
    assert [int(x) for x in out[1]] == [nt, len(sizes), runs, tiles, h, t, R.TIER_THREADS[t],
                                        -(-runs // R.TIER_THREADS[t]), 0 if t < 4 else (2 * h + 1 - 96) * 64 * 8,
                                        len(sizes) * 2048 * 4]
    e = R.edges(sizes)
    for tag, unit, n in (("r", R.RUN, runs), ("t", R.TILE, tiles)):
        spans = [[int(x) for x in ln[1:]] for ln in out[2:] if ln[0] == tag]
        assert len(spans) == n
        seen = np.zeros(nt, dtype=np.int64)
        for b, first, end in spans:
            assert e[b] <= first < end <= e[b + 1] and end - first <= unit           # never crosses a block
            assert (first - e[b]) % unit == 0 and (end - first == unit or end == e[b + 1])
            seen[first:end] += 1
        assert (seen == 1).all()
        assert spans == sorted(spans, key=lambda s: s[1])                              # in stream order


def test_policy_status_codes(driver):
    def create(nt, h, *sizes):
        return int(_run(driver, "status", nt, h, *sizes)[0][0])
    assert create(100, 4, 60, 40) == 0
    assert create(0, 4, 1) == 1 and create(100, 4) == 1 and create(-5, 4, 1) == 1                  # kBadSize
    assert create(100, 4, 60, 30) == 2 and create(100, 4, 60, 50) == 2 and create(100, 4, 100, 0) == 2
    assert create(100, 4, 101, -1) == 2 and create(2, 4, 1, 1, 1) == 2                             # kBadBlocks
    assert create(100, 0, 100) == 3 and create(100, 65, 100) == 3 and create(100, -1, 100) == 3    # kBadHalfWidth
    assert create(100, 1, 100) == 0 and create(100, 64, 100) == 0
    assert create(2 ** 32 - 1, 4, 2 ** 32 - 1) == 4 and create(2 ** 32 - 2, 4, 2 ** 32 - 2) == 0   # kTooLarge
    assert _run(driver, "ones", (1 << 18) + 1, 4)[0] == ["5"] and _run(driver, "ones", 1 << 18, 4)[0] == ["0"]   # kTooManyBlocks
    # two faults at once: size, then half-width, then the 32-bit limit, then the blocks, then their number
    assert create(2 ** 32 - 1, 0, 2 ** 32 - 1) == 3 and create(0, 0, 1) == 1
    assert _run(driver, "ones", (1 << 18) + 1, 4, (1 << 18) + 2)[0] == ["2"]

    def classify(nsigma, grow, have=0, kind=0):
        return [int(x) for x in _run(driver, "classify", nsigma, grow, have, kind)[0]]
    assert classify(5.0, 2) == [0, 0] and classify(1e-300, 0) == [0, 0] and classify(1e308, 64) == [0, 0]
    assert classify(0.0, 2)[0] == 6 and classify(-1.0, 2)[0] == 6 and classify("nan", 2)[0] == 6 \
        and classify("inf", 2)[0] == 6                                                             # kBadNsigma
    assert classify(5.0, -1)[0] == 7 and classify(5.0, 65)[0] == 7                                 # kBadGrow
    assert classify(5.0, 2, 1, 2)[1] == 8 and classify(5.0, 2, 1, -1)[1] == 8                      # kBadFlagKind
    assert classify(5.0, 2, 1, 0)[1] == 0 and classify(5.0, 2, 1, 1)[1] == 0 and classify(5.0, 2, 0, 7)[1] == 0


# ------------------------------------------------------ the Python layer's checks ----
def test_arguments_are_refused_before_the_gpu_is_needed():
    import torch
    from cosmomap2_amd import _hip
    from cosmomap2_amd.utilities import GlitchFlagger, apply_flags, flag_glitches
    d = np.zeros(100)
    pix = np.zeros(100, dtype=np.int32)
    for kw in (dict(half_width=0), dict(half_width=65), dict(half_width=2.5), dict(half_width=True)):
        with pytest.raises(ValueError):
            GlitchFlagger(10, **kw)
    for bs in (0, -3, 2.5, [], [10, 0], [10, -1], [2.5]):
        with pytest.raises(ValueError):
            GlitchFlagger(bs)
    gf = GlitchFlagger(10, half_width=4)
    for bad in (dict(nsigma=0), dict(nsigma=-1.0), dict(nsigma=float("nan")), dict(nsigma=float("inf")),
                dict(nsigma="x"), dict(grow=-1), dict(grow=65), dict(grow=1.5), dict(iterations=0),
                dict(iterations=9), dict(iterations=2.0), dict(sigma=[1.0, 2.0]), dict(sigma=-1.0),
                dict(sigma=float("nan")), dict(sigma=np.ones((10, 1))), dict(flags=pix[:50]),
                dict(flags=np.zeros(100)), dict(flags=np.zeros((10, 10), dtype=np.int32))):
        with pytest.raises(ValueError) as e:
            gf.flag(d, **bad)
        assert str(e.value), bad
        with pytest.raises(ValueError):
            flag_glitches(d, 10, half_width=4, **bad)
    for bad_d in (np.zeros(95), np.zeros((10, 10)), np.zeros(0), np.zeros(100, dtype=complex),
                  torch.zeros(100, dtype=torch.float32), torch.zeros(100, dtype=torch.float64)):   # (a host tensor)
        with pytest.raises(ValueError):
            gf.flag(bad_d)
        with pytest.raises(ValueError):
            gf.residual(bad_d)
    with pytest.raises(ValueError):
        GlitchFlagger([60, 30], 4).flag(d)                       # the sizes do not add up to the stream
    for prev in (np.zeros(100, dtype=np.int32), np.zeros(99, dtype=np.uint8), np.zeros((100, 1), dtype=np.uint8)):
        with pytest.raises(ValueError):
            gf.residual(d, prev=prev)
        with pytest.raises(ValueError):
            gf.scale(d, d, prev=prev)
    with pytest.raises(ValueError):
        gf.scale(d, np.zeros(99))
    cls = np.zeros(100, dtype=np.uint8)
    for p, c in ((pix, cls[:99]), (pix, cls.astype(np.int32)), (pix.astype(np.uint32), cls), (pix.reshape(10, 10), cls),
                 (pix[:0], cls[:0]), (np.full(100, 2 ** 40), cls), (torch.zeros(100, dtype=torch.int64), cls)):
        with pytest.raises(ValueError):
            apply_flags(p, c)
    if not torch.cuda.is_available():
        for call in (lambda: gf.flag(d, flags=pix), lambda: gf.residual(d), lambda: gf.scale(d, d),
                     lambda: apply_flags(pix, cls), lambda: gf.info(100)):
            with pytest.raises(_hip.HipError):
                call()
