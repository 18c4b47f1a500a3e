"""
The pointing expansion without a GPU: the two restatements of _pointing_expand_ref.py against each other, the
condition on the committed seeds that lets tests/test_gpu_pointing_expand.py demand equal pixels everywhere, the host
HEALPix helpers vec2pix / pix2vec, the quaternion helpers, and the argument checks of expand_pointing.
"""
import os
import re

import numpy as np
import pytest

import _pointing_expand_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(kind, nside, nest) for kind in ("random", "scan") for nside in R.NSIDES for nest in (False, True)]


def test_header_declares_the_entry_point_and_the_abi_is_unchanged():
    hdr = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    assert re.search(r"\bint cm2_pointing_expand\(int64_t ns, int ndet,", hdr)
    assert re.search(r"#define CM2_ABI_VERSION 2\b", hdr)
    from cosmomap2_amd import _hip
    assert len(_hip.PROTOTYPES["cm2_pointing_expand"]) == 13
    assert "cm2_pointing_expand" in _hip.RESTARTABLE


@pytest.mark.parametrize("kind,nside,nest", CASES)
def test_both_restatements_agree_and_the_committed_seeds_are_decided(kind, nside, nest):
    b, d, E, L = R.reference(kind, nside, nest)
    assert E[0].shape == (R.DMAX, R.NS) and L.pix.shape == (R.DMAX, R.NS)
    dec = L.decided
    np.testing.assert_array_equal(E[0][dec], L.pix[dec])
    assert E[0].min() >= 0 and E[0].max() < 12 * nside * nside
    # the condition of the GPU test: no undecided sample in the committed sets (change the seed, not the rule)
    assert dec.all(), "%d undecided samples" % int((~dec).sum())


def test_the_undecided_margin_is_thousands_of_ulps():
    for v in (0.3, 1.0, 1.999, 2.0, 777.7, 4.5 * 8192):
        assert float(R.THRESH) * max(1.0, v) / np.spacing(v) >= R.UNDECIDED_ULPS
    assert float(R.THRESH) / np.spacing(1.0) == R.UNDECIDED_ULPS
    assert R.UNDECIDED_ULPS > 100 * (1 + R.ROUNDINGS_AFTER_ATAN2)


@pytest.mark.parametrize("nside", [1, 2, 4, 16])
@pytest.mark.parametrize("nest", [False, True])
def test_vec2pix_inverts_pix2vec_on_every_pixel(nside, nest):
    from cosmomap2_amd.utilities.healpix_fits import pix2vec, vec2pix
    p = np.arange(12 * nside * nside)
    x, y, z = pix2vec(nside, p, nest=nest)
    np.testing.assert_allclose(x * x + y * y + z * z, 1.0, rtol=0, atol=1e-15)       # a few roundings each
    np.testing.assert_array_equal(vec2pix(nside, x, y, z, nest=nest), p)
    assert vec2pix(nside, float(x[-1]), float(y[-1]), float(z[-1]), nest=nest) == p[-1]
    assert pix2vec(nside, 0, nest=nest) == (float(x[0]), float(y[0]), float(z[0]))


def _directions(L):
    return tuple(np.asarray(c, dtype=np.float64) for c in L._d)


@pytest.mark.parametrize("nside", R.NSIDES)
def test_vec2pix_orderings_are_tied_by_nest2ring(nside):
    from cosmomap2_amd.utilities.healpix_fits import nest2ring, vec2pix
    L = R.reference("random", nside, False)[3]
    x, y, z = _directions(L)
    np.testing.assert_array_equal(nest2ring(nside, vec2pix(nside, x, y, z, nest=True)),
                                  vec2pix(nside, x, y, z, nest=False))


@pytest.mark.parametrize("kind,nside,nest", CASES)
def test_vec2pix_equals_the_long_double_restatement(kind, nside, nest):
    from cosmomap2_amd.utilities.healpix_fits import vec2pix
    L = R.reference(kind, nside, nest)[3]
    x, y, z = _directions(L)
    got = vec2pix(nside, x, y, z, nest=nest)
    np.testing.assert_array_equal(got[L.decided], L.pix[L.decided])


@pytest.mark.parametrize("nest", [False, True])
def test_pixel_centres_of_nside_8_come_back_through_E(nest):
    from cosmomap2_amd.utilities.healpix_fits import pix2vec
    from cosmomap2_amd.utilities.pointing_expand import quat_from_angles, quat_mult
    p = np.arange(12 * 8 * 8)
    x, y, z = pix2vec(8, p, nest=nest)
    psi = 0.01 + 3.0 * p / p.size
    q = quat_from_angles(np.arccos(z), np.arctan2(y, x), psi)
    det = np.array([[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, np.sin(0.2), np.cos(0.2)]])     # the second: psi + 0.4
    pix, c, s, _ = R.expand_E(q, det, 8, nest)
    np.testing.assert_array_equal(pix[0], p)
    np.testing.assert_array_equal(pix[1], p)
    np.testing.assert_allclose(c[0], np.cos(2 * psi), rtol=0, atol=1e-13)
    np.testing.assert_allclose(s[0], np.sin(2 * psi), rtol=0, atol=1e-13)
    np.testing.assert_allclose(c[1], np.cos(2 * (psi + 0.4)), rtol=0, atol=1e-13)
    np.testing.assert_allclose(s[1], np.sin(2 * (psi + 0.4)), rtol=0, atol=1e-13)
    # quat_mult is the product of the definition
    np.testing.assert_array_equal(quat_mult(q, det[1]), R.qmul_E(q, det[1][None, :]))


@pytest.mark.parametrize("hwp", [None, "plate", "big"])
def test_fp64_error_against_long_double_within_the_derived_count(hwp):
    chi = None if hwp is None else R.hwp_angles(big=hwp == "big")
    worst = 0.0
    for kind in ("random", "scan"):
        b, d = R.INPUTS[kind](R.DMAX)
        E, L = R.expand_E(b, d, 64, False, hwp=chi), R.expand_L(b, d, 64, False, hwp=chi)
        err = np.maximum(np.abs(E[1].astype(R.LD) - L.cos), np.abs(E[2].astype(R.LD) - L.sin)).astype(np.float64)
        k = err / R.U
        share = float((k / R.k_E(L.s, hwp is not None)).max())
        print("\n%s, hwp %s: largest error %.1f x 2^-53 (at sin(theta) = %.3g), largest k_E sin(theta) = %.1f, "
              "%.3g of the derived count" % (kind, hwp, k.max(), L.s.ravel()[k.argmax()], (k * L.s).max(), share))
        worst = max(worst, share)
    # inside the derived worst case, and the worst case not vacuous: within twenty times of what is measured
    assert 0.05 <= worst <= 1.0


def test_handmade_set_is_consistent_between_the_restatements():
    b, names = R.handmade()
    det = np.array([[0.0, 0.0, 0.0, 1.0]])
    for nside in R.NSIDES:
        for nest in (False, True):
            E, L = R.expand_E(b, det, nside, nest), R.expand_L(b, det, nside, nest)
            for i, nm in enumerate(names):
                assert int(E[0][0, i]) in L.allowed(0, i), (nm, nside, nest, int(E[0][0, i]), L.allowed(0, i))
    assert not L.decided.all()                     # the set does reach the undecided branch


def test_arguments_are_refused_before_the_gpu_is_needed():
    from cosmomap2_amd import _hip
    from cosmomap2_amd.utilities import expand_pointing, quat_from_angles, quat_mult      # exported
    assert callable(quat_from_angles) and callable(quat_mult)
    b, d = R.random_inputs(3, ns=10)
    bad = [
        dict(nside=3), dict(nside=0), dict(nside=16384), dict(nside=2.5), dict(nside="x"),
        dict(pol=4), dict(boresight=b[:, :3]), dict(boresight=b.ravel()), dict(detquats=d[:0]),
        dict(detquats=d.T), dict(hwp=np.zeros(9)), dict(flags=np.zeros((10, 1))),
        dict(frame=[1.0, 0.0, 0.0]), dict(frame=[0.0, 0.0, 0.0, 0.0]), dict(frame=[np.nan, 0.0, 0.0, 1.0]),
        dict(detquats=np.array([[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0]])),
        dict(detquats=np.array([[np.inf, 0.0, 0.0, 1.0]])),
        dict(out=(np.zeros(30, dtype=np.int32), None, None)), dict(out=(None, None)),
    ]
    for kw in bad:
        args = dict(boresight=b, detquats=d, nside=64)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            expand_pointing(**args)
        assert str(e.value)
    with pytest.raises(ValueError, match="3"):
        expand_pointing(b, d, 3)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipError):
            expand_pointing(b, d, 64)
