"""
The references, restatements and bounds of tests/_noise_ref.py, checked without a GPU: a bound that the
float64 restatement could not meet would be too tight, a bound that a wrong kernel could meet would be
vacuous, and a reference that disagreed with the project's established oracle would be a second opinion
nobody asked for.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noise_ref as R  # noqa: E402
from conftest import rel_l2  # noqa: E402


def test_geometry_restated():
    """windows / fft_geometry / dir_tiles give the counts the cases were chosen for"""
    nwin = {name: len(R.windows(R.offsets(R.SIZES[name]))) for name in ("E1", "E2", "E3", "E8", "E9")}
    assert nwin == {"E1": 15, "E2": 7, "E3": 1, "E8": 8, "E9": 9}
    assert sum(R.SIZES["E1"]) == 86020 and sum(R.SIZES["E2"]) == 24579
    assert (R.N, R.W, R.HOP, R.RLEN) == (256 * 32, 2 * R.N, R.W - 2 * R.HALO, 512 * (32 - 8) // 2)
    # a window of every block: start, length, block limits
    w = R.windows(R.offsets(R.SIZES["E2"]))
    assert [(x.len, x.blk) for x in w] == [(1, 0), (2047, 1), (2048, 2), (2049, 3), (6145, 4), (12288, 5), (1, 5)]
    assert w[-1].start == w[-2].start + R.HOP and w[-1].hi == 24579 and w[-1].lo == w[-2].lo
    L, halo, hop, segs = R.fft_geometry(1, R.SIZES["F1"])          # the L < 2 halo + 2 branch
    assert (L, halo, hop, len(segs)) == (4, 0, 4, 3)
    L, halo, hop, segs = R.fft_geometry(2, R.SIZES["F2"])
    assert (L, halo, hop, len(segs)) == (256, 1, 254, 2 + 2 + 1)
    L, halo, hop, segs = R.fft_geometry(33, R.SIZES["F33"])
    assert (L, halo, hop) == (256, 32, 192)
    assert [s.len for s in segs] == [191, 192, 192, 1, 192, 192, 1, 50]     # hop - 1, hop, hop + 1, 2 hop + 1
    L, halo, hop, segs = R.fft_geometry(2049, R.SIZES["E2"])
    assert (L, halo, hop, len(segs)) == (16384, 2048, 12288, 7)
    assert R.fft_geometry(33, R.SIZES["F33"], 1024)[:3] == (1024, 32, 960)
    assert R.fft_geometry(33, R.SIZES["F33"], 65)[0] == 256                   # CM2_FFT_LEN too short: ignored
    t = R.dir_tiles(R.offsets(R.SIZES["E2"]))
    assert [n for _, n, _ in t] == [1, 2047, 2048, 2048, 1, 2048, 2048, 2048, 1] + [2048] * 6 + [1]
    # list formats of the tile cases: 100 tiles run-coded, 800 inverse, 2100 plain; sorted lists never inverse
    assert [R.choose_lists(0, False, n) for n in (1, 100, 767, 768, 800, 2048, 2049, 2100)] == [2, 2, 2, 3, 3, 3, 1, 1]
    assert [R.choose_lists(0, True, n) for n in (100, 800, 2100)] == [2, 2, 1]
    assert [R.choose_lists(w, False, 2100) for w in (1, 2, 3)] == [1, 1, 1]


def test_cases_are_what_they_claim():
    for lam in (1, 2, 32, 33, 300, 2048, 2049, 8578):
        R.make_bands(lam, 2)                                       # asserts the size of the last tap
    cs = R.case("E2", 33, "impulses", "first_last")
    off = R.offsets(cs.sizes)
    assert not cs.ok[off[:-1]].any() and not cs.ok[off[1:] - 1].any() and (cs.raw[~cs.ok] != 0).all()
    assert not cs.v[~cs.ok].any()
    cs = R.case("E9", 33, "normal", "window")
    B = R.window_scale(cs.sizes, cs.bands, cs.v, R.W, R.HALO, R.HOP)
    off = R.offsets(cs.sizes)
    assert not cs.ok[off[3]:off[4]].any() and cs.ok[off[5]:off[6]].all()
    assert not B[off[3]:off[4]].any() and not B[off[5]:off[6]].any() and B[off[4]] > 0     # two windows with B = 0
    cs = R.case("E2", 2049, "impulses", "window")
    assert not cs.ok[off_last(cs) + R.HOP:].any() and cs.ok[:off_last(cs) + R.HOP].all()
    imp = R.make_input("E1", "impulses")
    off = R.offsets(R.SIZES["E1"])
    pos = [int(np.flatnonzero(imp[off[b]:off[b + 1]])[0]) for b in range(len(R.SIZES["E1"]))]
    assert {R.HOP - 1, R.HOP, R.RLEN - 1, R.RLEN, 0} <= set(pos), pos
    ids = [t.id for t in R.TILE_CASES]
    assert len(ids) == len(set(ids)) == 20
    for ls in ("plain", "rc", "inv"):
        for fl in (False, True):
            lay = {(t.pointing, t.flags) for t in R.TILE_CASES if t.lists == ls and t.flat == fl}
            assert {("raster", "random7"), ("random", "window")} <= lay


def off_last(cs):
    return int(R.offsets(cs.sizes)[-2])


def test_reference_agrees_with_the_oracle(golden, oracle):
    """toeplitz_ref against the oracle's blocklo_mult on the golden vectors; direct_f64 bit-equal to it"""
    v = golden["toep_v"]
    for lam in (1, 2, 33):
        a, y = golden["toep_a%d" % lam], golden["toep_y%d" % lam]
        for sizes in ([200], [1, 2, 60, 137], [100, 100]):
            bands = [a * (1.0 + 0.5 * b) for b in range(len(sizes))]
            want = oracle.blocklo_mult(sizes, bands, True, v)
            if sizes == [200]:
                R.assert_bit_equal(want, y, "oracle against the golden vector")
            R.assert_bit_equal(R.direct_f64(sizes, bands, v), want, "direct_f64, lambda %d, sizes %r" % (lam, sizes))
            ref = R.toeplitz_ref(sizes, bands, v)
            S = R.toeplitz_ref(sizes, np.abs(bands), np.abs(v))
            assert R.excess(want, ref, S, 2 * lam + 1) <= 1.0
    a, vs = golden["toep_a9"], golden["toep_vshort"]
    R.assert_bit_equal(R.direct_f64([5], [a], vs), golden["toep_yshort"], "band longer than the block")
    R.assert_bit_equal(R.direct_f64([5], [a], vs), oracle.blocklo_mult([5], [a], True, vs), "the same, oracle")
    assert R.excess(golden["toep_yshort"], R.toeplitz_ref([5], [a], vs),
                    R.toeplitz_ref([5], [np.abs(a)], np.abs(vs)), 2 * 9 + 1) <= 1.0
    R.assert_bit_equal(R.diag_f64([2, 3], [2.0, 0.5], np.arange(5.0)), oracle.blocklo_mult([2, 3], [2.0, 0.5], False,
                                                                                          np.arange(5.0)), "diagonal")


@pytest.mark.parametrize("route", ["fused", "fft"])
def test_restatements_meet_their_bounds_and_constants_are_fresh(route):
    """Every restatement is within 1/8 of its bound on every shared case; WORST is what is measured now,
    rounded up to one decimal"""
    worst = R.measure_worst(route)
    print("%s: largest |restatement - ref| / (2^-53 B) per lambda: %s" % (route, {k: round(v, 2) for k, v in
                                                                                 sorted(worst.items())}))
    assert {k: R.round_up(v) for k, v in worst.items()} == R.WORST[route], "WORST is stale"
    for lam, w in worst.items():
        assert w / R.c_of(route, lam) <= 1.0 / 8.0, (route, lam, w, R.c_of(route, lam))


def test_kernel_passes_stay_inside_the_constants():
    """The kernel's own three passes, butterfly order, 32-entry table and twiddle recurrences, in NumPy float64:
    they equal NumPy's FFT to rounding, lose more than it does (the recurrences), and still meet every bound
    that was made from NumPy's FFT -- what is left of the headroom of 8 is for the FMA contraction."""
    rng = np.random.default_rng(0)
    z = rng.standard_normal(R.N) + 1j * rng.standard_normal(R.N)
    re, im = R.passes_forward(z.real.copy(), z.imag.copy())
    Z, want = R.passes_natural(re) + 1j * R.passes_natural(im), np.fft.fft(z)
    assert np.abs(Z - want).max() <= 64 * 2.0 ** -53 * np.abs(want).max()
    R.assert_bit_equal(R.passes_natural(R.passes_layout(want.real)), want.real, "layout and back")
    y = R.passes_inverse(re, im)
    assert np.abs((y[0] + 1j * y[1]) / R.N - z).max() <= 256 * 2.0 ** -53 * np.abs(z).max()
    worst = {}
    for key in R.fused_keys():
        cs = R.case(*key)
        e = R.share(R.os_f64(cs.sizes, cs.bands, cs.v, passes=True), cs, "fused")
        worst[cs.lam] = max(worst.get(cs.lam, 0.0), e)
    print("the kernel's passes in float64: largest share of the bound per lambda: %s"
          % {k: round(v, 3) for k, v in sorted(worst.items())})
    assert max(worst.values()) <= 1.0, worst


def test_direct_restatement_against_the_reference():
    """direct_f64 stays within (2 lambda + 1) 2^-53 sum |a| |v| of the reference on its cases, zeros stay zeros"""
    for name, lam in R.DIRECT_CASES:
        for inp in ("normal", "impulses"):
            cs = R.case(name, lam, inp)
            got = R.direct_f64(cs.sizes, cs.bands, cs.v)
            S = R.toeplitz_ref(cs.sizes, np.abs(cs.bands), np.abs(cs.v))
            assert R.excess(got, cs.ref, S, 2 * lam + 1) <= 1.0, (name, lam, inp)


ALL_MUTATIONS = dict(R.MUTATIONS, **R.SUBTLE)


def _mutate(name):
    route, key, kind = ALL_MUTATIONS[name]
    cs = R.case(*key)
    if route == "direct":
        return cs, kind, R.direct_f64(cs.sizes, cs.bands, cs.v), R.direct_f64(cs.sizes, cs.bands, cs.v, mut=name)
    return cs, kind, R.os_f64(cs.sizes, cs.bands, cs.v), R.os_f64(cs.sizes, cs.bands, cs.v, mut=name, raw=cs.raw)


# the smallest factor by which a value mutation exceeds the bound of its case (inf: an element that must be exactly
# zero is not, or a NaN is left), rounded DOWN to two digits; measured by the test below
FACTORS = {
    "dir_tile_halo": 1.3e11, "flag_leak": 1.5e13, "halo_short": 1.6e10, "last_tap_dropped": 3.3e11,
    "no_zero_boundary": 7.5e19, "nyquist_dropped": 2.5e8, "partner_same": 7.3e13, "prev_block_band": 1.9e13,
    "round_seam": 3.2e12, "drop_last_output": float("inf"), "window_skipped": float("inf"),
    "seam_1e11": 150.0, "tables_three_digits": 6.8,
}


def test_the_twelve_mutations_are_there():
    assert len(R.MUTATIONS) == 12 and not set(R.MUTATIONS) & set(R.SUBTLE)


@pytest.mark.parametrize("name", sorted(ALL_MUTATIONS))
def test_every_mutation_fails_its_check(name):
    cs, kind, good, bad = _mutate(name)
    route = ALL_MUTATIONS[name][0]
    old = rel_l2(bad, np.asarray(cs.ref, dtype=np.float64)) < 1e-12     # (a NaN compares False: noticed)
    if route == "direct":
        R.assert_bit_equal(good, R.direct_f64(cs.sizes, cs.bands, cs.v), name)
        assert (R.bits(bad) != R.bits(good)).any(), name + ": still bit-equal"
        factor = R.share(bad, cs, "fused") if kind == "value" else None
    else:
        assert R.share(good, cs, "fused") <= 1.0 / 8.0
        factor = R.share(bad, cs, "fused")
    if kind == "nan":
        assert np.isnan(bad).any(), name + ": no NaN is left"
    elif kind == "value":
        assert factor >= 100.0, "%s: only %.3g x the bound" % (name, factor)
    elif kind == "subtle":
        assert factor > 1.0 and old, "%s: %.3g x the bound, rel_l2 %s" % (name, factor, old)
    print("%s on %r: %s; rel_l2 < 1e-12 over the stream would %s" % (
        name, ALL_MUTATIONS[name][1], "x %.3g the bound" % factor if factor is not None else "bit-equality lost",
        "NOT have noticed" if old else "have noticed"))
    if name in FACTORS:
        assert factor >= FACTORS[name], "%s: the recorded factor %.3g is stale (now %.3g)" % (name, FACTORS[name], factor)


def test_fft_route_mutations():
    """the mutations that the rocFFT restatement has fail its check too"""
    cs = R.case("F33", 33, "normal")
    assert R.share(R.fft_f64(cs.sizes, cs.bands, cs.v), cs, "fft") <= 1.0 / 8.0
    for mut in ("no_zero_boundary", "prev_block_band", "last_tap_dropped", "drop_last_output", "window_skipped"):
        assert R.share(R.fft_f64(cs.sizes, cs.bands, cs.v, mut=mut), cs, "fft") >= 100.0, mut
