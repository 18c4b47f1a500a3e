"""
The references and bounds of tests/_vector_ref.py, checked without a GPU: a bound that the
float64 restatements and plain NumPy float64 products could not meet would be too tight, a bound
that a wrong kernel could meet would be vacuous.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vector_ref as R  # noqa: E402


def _pair(family, seed, n, ra=None, rb=None):
    if family == "a":
        sa = (n,) + ((ra,) if ra is not None else ())
        sb = (n,) + ((rb,) if rb is not None else ())
        return R.normals(seed, *sa), R.normals(seed + 1, *sb)
    return R.cancelling(seed, n, ra, rb)


def _m2_case(pol, r, npix, seed=5, shift=0):
    W = R.pixel_weights(seed, npix, shift)
    det, mask = R.det_mask_f64(pol, W)
    Z, AZ = R.normals(seed + 1, pol * npix, r), R.normals(seed + 2, pol * npix, r)
    y, res = R.normals(seed + 3, r), R.normals(seed + 4, pol * npix)
    return Z, AZ, y, res, W, det, mask


def test_cancelling_family_cancels():
    x, y = R.cancelling(3, 4097)
    ref, S = R.dot_ref(x, y)
    assert abs(ref[0]) < 1e-7 * S[0]
    A, B = R.cancelling(4, 1001, 3, 2)
    ref, S = R.gemm_tn_ref(A, B)
    assert (np.abs(ref) < 1e-6 * S).all()


def test_pixel_weights_mask_pattern():
    for pol in (1, 2, 3):
        for npix in (63, 127, 200, 4099):
            _, mask = R.det_mask_f64(pol, R.pixel_weights(7, npix))
            last = mask[(npix // 64) * 64:]
            assert last.min() == 0 and last.max() == 1, (pol, npix)
        assert R.det_mask_f64(pol, R.pixel_weights(7, 65))[1][-1] == 1
        assert R.det_mask_f64(pol, R.pixel_weights(7, 65, shift=1))[1][-1] == 0


@pytest.mark.parametrize("family", ["a", "b"])
def test_bounds_hold_for_float64(family):
    """Every float64 restatement and a NumPy float64 product of every reduction and contraction
    stays within c 2^-53 S of the extended reference."""
    worst = {}

    def ok(name, got, ref, S, c):
        worst[name] = max(worst.get(name, 0.0), R.assert_within(got, ref, S, c, name))

    for n in (1, 257, 4099):
        x, y = _pair(family, 10 + n, n)
        a = 0.37
        ok("axpy", R.axpy_f64(a, x, y), *R.axpy_ref(a, x, y), R.C_AXPY)
        ok("scal", R.scal_f64(a, x), *R.scal_ref(a, x), R.C_SCAL)
        ok("xmy", R.xmy_f64(x, y), *R.xmy_ref(x, y), R.C_XMY)
        ok("update_p", R.update_p_f64(0.7, 1.9, x, y), *R.update_p_ref(0.7, 1.9, x, y), R.C_UPDATE_P)
        p, q = _pair(family, 20 + n, n)
        xn, rn = R.update_xr_f64(0.7, 1.9, p, q, x, y)
        (xr, Sx), (rr_, Sr) = R.update_xr_ref(0.7, 1.9, p, q, x, y)
        ok("update_xr x", xn, xr, Sx, R.C_UPDATE_XR)
        ok("update_xr r", rn, rr_, Sr, R.C_UPDATE_XR)
        ok("update_xr rr", [np.dot(rn, rn)], *R.update_xr_rr_ref(0.7, 1.9, q, y), R.c_update_xr_rr(n))
    for n in (1, 255, 262145, 786437):
        x, y = _pair(family, 30 + n, n)
        ok("dot", [np.dot(x, y)], *R.dot_ref(x, y), R.c_dot(n))
    for r in (1, 5, 16, 32, 200):
        for n in (1, 3, 4097):
            x, Z = _pair(family, 40 + n + r, n, None, r)
            for aligned in (True, False):
                ok("Zt", Z.T @ x, *R.zt_ref(Z, x), R.c_zt(n, r, aligned))
            yv = R.normals(41, r)
            ref, S = R.z_apply_ref(Z, yv)
            ok("Z_apply restated", R.z_apply_f64(Z, yv), ref, S, R.c_serial(r))
            ok("Z_apply @", Z @ yv, ref, S, R.c_serial(r))
            ref, S = R.z_axpy_ref(Z, yv, -0.3, x)
            ok("Z_axpy restated", R.z_axpy_f64(Z, yv, -0.3, x), ref, S, R.c_z_axpy(r, False))
            ok("Z_axpy @", x + (-0.3) * (Z @ yv), ref, S, R.c_z_axpy(r, False))
    for r1, r2 in ((16, 16), (64, 64), (3, 7), (64, 16)):
        for n in (1, 5, 2049):
            Z1, Z2 = _pair(family, 50 + n + r1, n, r1, r2)
            for aligned in (True, False):
                ok("gemm_tn", Z1.T @ Z2, *R.gemm_tn_ref(Z1, Z2), R.c_gemm_tn(n, r1, r2, aligned))
    for rin, rout in ((32, 16), (5, 3)):
        P, W, o0 = R.normals(60, 17, rin), R.normals(61, rin, rout), R.normals(62, 17, rout)
        ok("panel_gemm", P @ W + o0, *R.panel_gemm_ref(P, W, o0), R.c_panel_gemm(rin, False))
        ok("panel_gemm", P @ W, *R.panel_gemm_ref(P, W), R.c_panel_gemm(rin, False))
    for r in (1, 32, 256):
        M, v = R.normals(70, r, r), R.normals(71, r)
        ok("small_matvec", M @ v, *R.matmul_ref(M, v), R.c_serial(r))
    A, B = R.normals(72, 40, 32), R.normals(73, 32, 40)
    ok("gemm_atbt", A.T @ B.T, *R.gemm_atbt_ref(A, B), R.c_serial(40))
    for pol in (1, 2, 3):
        for r in (5, 32):
            Z, AZ, y, res, W, det, mask = _m2_case(pol, r, 127)
            ref, S = R.m2_finish_ref(pol, Z, AZ, y, res, W, det, mask)
            ok("m2 restated", R.m2_finish_f64(pol, Z, AZ, y, res, W, det, mask), ref, S,
               R.c_m2(pol, r, False))
            t = (res - AZ @ y).reshape(-1, pol)
            got = (R.bd_inverse_f64(pol, W, det, mask, t) + (Z @ y).reshape(-1, pol)).reshape(-1)
            ok("m2 @", got, ref, S, R.c_m2(pol, r, False))
    print("largest |got - ref| / bound per operation:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0


def test_restatement_masked_pixels_are_zero_plus_zy():
    for pol in (1, 2, 3):
        Z, AZ, y, res, W, det, mask = _m2_case(pol, 5, 70)
        out = R.m2_finish_f64(pol, Z, AZ, y, res, W, det, mask).reshape(-1, pol)
        zy = R.z_apply_f64(Z, y).reshape(-1, pol)
        assert (mask == 0).any() and (mask == 1).any()
        R.assert_bit_equal(out[mask == 0], 0.0 + zy[mask == 0])


@pytest.mark.parametrize("family", ["a", "b"])
def test_bounds_bite(family):
    """Wrong variants, made in NumPy only, break the bound: one dropped last element, the last
    row taken from row n - 2, two columns swapped, one masked pixel treated as unmasked, beta and
    1 / beta exchanged.  Every factor |got - ref| / (c 2^-53 S) must exceed 1.  The smallest seen
    is 8.0e+03: family b, Z^T x with two result columns swapped, where both columns are ~1e-9 of
    S by construction (next: 1.8e+05, Z1^T Z2 with two columns swapped, family b).  With family a
    the smallest is 2.4e+09 (Z^T x without its last row); an unmasked singular pixel gives inf."""
    factors = {}

    def bites(name, got, ref, S, c):
        f = R.excess(got, ref, S, c)
        factors[name] = min(factors.get(name, np.inf), f)

    for n in (257, 4097):
        # --- one dropped last element
        x, y = _pair(family, 100 + n, n)
        ref, S = R.dot_ref(x, y)
        bites("dot drops last", [np.dot(x[:-1], y[:-1])], ref, S, R.c_dot(n))
        p, q = _pair(family, 101 + n, n)
        _, rn = R.update_xr_f64(0.7, 1.9, p, q, x, y)
        bites("rr drops last", [np.dot(rn[:-1], rn[:-1])], *R.update_xr_rr_ref(0.7, 1.9, q, y),
              R.c_update_xr_rr(n))
        for r in (5, 16):
            x, Z = _pair(family, 102 + n + r, n, None, r)
            yv = R.normals(103, r)
            sw = np.arange(r)
            sw[[1, 2]] = [2, 1]
            for aligned in (True, False):
                c = R.c_zt(n, r, aligned)
                bites("Zt drops last row", Z[:-1].T @ x[:-1], *R.zt_ref(Z, x), c)
                bites("Zt swaps columns", (Z.T @ x)[sw], *R.zt_ref(Z, x), c)
            # --- the last row taken from row n - 2
            Zw = Z.copy()
            Zw[-1] = Z[-2]
            ref, S = R.z_apply_ref(Z, yv)
            bites("Z_apply last row", R.z_apply_f64(Zw, yv), ref, S, R.c_serial(r))
            bites("Z_apply swaps columns", R.z_apply_f64(Z[:, sw], yv), ref, S, R.c_serial(r))
            ref, S = R.z_axpy_ref(Z, yv, -0.3, x)
            bites("Z_axpy last row", R.z_axpy_f64(Zw, yv, -0.3, x), ref, S, R.c_z_axpy(r, False))
            bites("Z_axpy swaps columns", R.z_axpy_f64(Z[:, sw], yv, -0.3, x), ref, S,
                  R.c_z_axpy(r, False))
        for r1, r2 in ((16, 16), (3, 7)):
            Z1, Z2 = _pair(family, 104 + n, n, r1, r2)
            sw = np.arange(r2)
            sw[[0, r2 - 1]] = [r2 - 1, 0]
            ref, S = R.gemm_tn_ref(Z1, Z2)
            for aligned in (True, False):
                c = R.c_gemm_tn(n, r1, r2, aligned)
                bites("gemm_tn drops last row", Z1[:-1].T @ Z2[:-1], ref, S, c)
                bites("gemm_tn swaps columns", Z1.T @ Z2[:, sw], ref, S, c)
        # --- beta and 1 / beta exchanged
        bites("update_p beta inverted", R.update_p_f64(1.9, 0.7, x, y), *R.update_p_ref(0.7, 1.9, x, y),
              R.C_UPDATE_P)
    P, W, o0 = R.normals(110, 17, 32), R.normals(111, 32, 16), R.normals(112, 17, 16)
    Pw = P.copy()
    Pw[-1] = P[-2]
    sw = np.arange(16)
    sw[[3, 4]] = [4, 3]
    ref, S = R.panel_gemm_ref(P, W, o0)
    bites("panel_gemm last row", Pw @ W + o0, ref, S, R.c_panel_gemm(32, True))
    bites("panel_gemm swaps columns", P @ W[:, sw] + o0, ref, S, R.c_panel_gemm(32, True))
    M, v = R.normals(113, 32, 32), R.normals(114, 32)
    bites("small_matvec swaps columns", M[:, np.r_[1, 0, 2:32]] @ v, *R.matmul_ref(M, v), R.c_serial(32))
    for pol in (1, 2, 3):
        for r, wide in ((5, False), (32, True), (32, False)):
            Z, AZ, y, res, W, det, mask = _m2_case(pol, r, 127)
            ref, S = R.m2_finish_ref(pol, Z, AZ, y, res, W, det, mask)
            c = R.c_m2(pol, r, wide)
            Zw, AZw = Z.copy(), AZ.copy()
            Zw[-1], AZw[-1] = Z[-2], AZ[-2]
            bites("m2 last row of Z", R.m2_finish_f64(pol, Zw, AZ, y, res, W, det, mask), ref, S, c)
            bites("m2 last row of AZ", R.m2_finish_f64(pol, Z, AZw, y, res, W, det, mask), ref, S, c)
            sw = np.r_[1, 0, 2:r]
            bites("m2 swaps columns", R.m2_finish_f64(pol, Z[:, sw], AZ[:, sw], y, res, W, det, mask),
                  ref, S, c)
            # --- one masked pixel treated as unmasked
            m1 = mask.copy()
            m1[np.flatnonzero(mask == 0)[-1]] = 1
            bites("m2 unmasks a pixel", R.m2_finish_f64(pol, Z, AZ, y, res, W, det, m1), ref, S, c)
    print("smallest violation factors:", {k: "%.3g" % v for k, v in sorted(factors.items(), key=lambda kv: kv[1])})
    assert min(factors.values()) > 1.0, factors
