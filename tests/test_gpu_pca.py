"""
The PCA filter on the GPU (cm2_pca_*, PCAFilterLO) against tests/_pca_ref.py.

Covariance, entry by entry: |got - ref| <= (L + 2) 2^-53 S_ab 1.01 with L the chunk length and S_ab = sum |x_a| |x_b|
(any order of an L-term dot product obeys it; derived, never measured here), exactly 0 where S_ab = 0, exactly
symmetric, the same bits in two calls and the same bits for a unit computed alone and inside a longer stream.
Apply, fit and status: bit-equal to the float64 restatement (cm2_cmode's unit per chunk with that chunk's modes), or
within _cmode_ref's bound of the extended-precision reference, as in test_gpu_cmode.py; the classes are the
reference's.  Outputs go in guarded buffers.
"""
import ctypes
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cmode_ref as C  # noqa: E402
import _pca_ref as R  # noqa: E402
import _pointing_expand_ref as PE  # noqa: E402
from _guarded import Guarded, GuardedInt  # noqa: E402

pytestmark = pytest.mark.gpu
LD, U53, V = R.LD, R.U53, R.V
SEG, TILE = R.SEGMENT, R.TILE


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import cosmomap2_amd
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device
    from cosmomap2_amd.interfaces import linearoperators as L
    return SimpleNamespace(I=I, U=U, L=L, D=device, hip=_hip, cg=cosmomap2_amd.cg, torch=torch)


def same_bits(a, b):
    return np.array_equal(R.bits(np.asarray(a)), R.bits(np.asarray(b)))


def edges_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ------------------------------------------------------------- covariance cases ----
# name: (group sizes, chunk lengths).  "sizes": one below, at and one above the 16-row MFMA block and the 128-row
# workgroup tile, three tiles with a partial last one, a group of one; chunks of 1, 3, 4, 5 samples that start at 1,
# 4, 8 and 13, ns odd.  "lengths": four unequal groups; segment - 1, segment, segment + 1 and 2 segments + 7 between
# short chunks, so that they start at 3, 4098, 8194, 8199, 12296: not multiples of 4; ns odd.  "tiles_x_segments": two
# tiles and two segments at once (the item of pair p > 0, segment s > 0).
COV_CASES = {
    "sizes": ([1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 44], [1, 3, 4, 5, 32]),
    "lengths": ([1, 17, 64, 30], [3, SEG - 1, SEG, 5, SEG + 1, 2 * SEG + 7, 1, 4, 1]),
    "tiles_x_segments": ([TILE + 2, 3], [SEG + 4, 1]),
}
COV_PATTERNS = {"sizes": ("null", "none", "random", "dead", "chunk"), "lengths": ("random",),
                "tiles_x_segments": ("random",)}


@functools.lru_cache(maxsize=None)
def cov_case(name):
    sizes, lengths = COV_CASES[name]
    gedges, cedges = edges_of(sizes), edges_of(lengths)
    ndet, ns = int(gedges[-1]), int(cedges[-1])
    assert ns % 2 == 1
    rng = np.random.default_rng(900 + sorted(COV_CASES).index(name))
    d = rng.standard_normal((ndet, ns)) * 3.0 + 50.0 * rng.standard_normal(ns)[None, :]     # correlated detectors
    return SimpleNamespace(name=name, sizes=sizes, gedges=gedges, cedges=cedges, ndet=ndet, ns=ns, d=d.reshape(-1))


@functools.lru_cache(maxsize=None)
def cov_flags(name, pattern):
    """the flags of a pattern as a pix array (None: the NULL pointer), and what the pattern singles out"""
    cs = cov_case(name)
    rng = np.random.default_rng(77)
    ok = np.ones((cs.ndet, cs.ns), dtype=bool)
    if pattern == "null":
        return None
    if pattern == "random":
        ok = rng.random(ok.shape) >= 0.30
    elif pattern == "dead":
        ok[cs.gedges[-1] - 50] = False                       # in the third tile of the last group
        ok[cs.gedges[2] + 3] = False
    elif pattern == "chunk":
        ok[:, cs.cedges[2]:cs.cedges[3]] = False
    pix = np.where(ok, rng.integers(0, 1000, ok.shape), -1 - rng.integers(0, 3, ok.shape)).astype(np.int32)
    return pix.reshape(-1)


@functools.lru_cache(maxsize=None)
def cov_reference(name, pattern):
    cs = cov_case(name)
    return R.cov_ref(cs.d, cov_flags(name, pattern), cs.ndet, cs.gedges, cs.cedges)


_ops = {}


def cov_op(cm, name, pattern="none"):
    """the operator of a covariance case (its flags are those of the pattern; NULL is a call's choice)"""
    key = (name, "none" if pattern == "null" else pattern)
    if key not in _ops:
        cs = cov_case(name)
        _ops[key] = cm.I.PCAFilterLO(cov_flags(name, key[1]), cs.ndet, groups=cs.gedges, chunks=cs.cedges)
    return _ops[key]


def check_units(cs, cov, ref, S, what):
    worst = 0.0
    for c in range(len(cs.cedges) - 1):
        L = int(cs.cedges[c + 1] - cs.cedges[c])
        for g in range(len(cs.sizes)):
            got = cov[c][g]
            assert got.shape == (cs.sizes[g], cs.sizes[g]) and same_bits(got, got.T), (what, c, g)
            e = R.cov_excess(got, ref[c][g], S[c][g], L)
            assert e <= 1.0, "%s: unit (%d, %d) is %.3g x the bound" % (what, c, g, e)
            worst = max(worst, e)
    return worst


# ------------------------------------------------------------- 1: the covariance ----
@pytest.mark.parametrize("name,pattern", [(n, p) for n in COV_CASES for p in COV_PATTERNS[n]])
def test_covariance_within_the_derived_bound(cm, name, pattern):
    cs = cov_case(name)
    F = cov_op(cm, name, pattern)
    ref, S = cov_reference(name, pattern)
    total = len(cs.cedges[:-1]) * int((np.array(cs.sizes) ** 2).sum())
    assert F.filter_info()["cov_doubles"] == total == cm.hip.load().cm2_pca_cov_doubles(F._handle.h)
    # the C entry point, into a guarded buffer, twice
    d_in, d_a, d_b = Guarded(cm, cs.ndet * cs.ns, cs.d), Guarded(cm, total), Guarded(cm, total)
    flags = None if pattern == "null" else cm.D.ptr(F._d_pix)
    for out in (d_a, d_b):
        cm.hip.call("cm2_pca_cov", F._handle.h, d_in.ptr, flags, out.ptr, cm.D.stream())
    a = d_a.get()
    assert same_bits(a, d_b.get())                                       # the same bits in two calls
    for g in (d_in, d_a, d_b):
        g.intact("cov %s %s" % (name, pattern))
    assert same_bits(d_in.get(), cs.d)
    cov = F.covariance(cs.d, use_flags=pattern != "null")
    offs = R.cov_offsets(cs.gedges, len(cs.cedges) - 1)
    for c, row in enumerate(cov):
        for g, unit in enumerate(row):
            assert same_bits(unit.reshape(-1), a[offs[c][g]:offs[c][g] + unit.size]), (c, g)     # the stated layout
    worst = check_units(cs, cov, ref, S, "%s %s" % (name, pattern))
    print("%s %s: the worst entry uses %.3g of the bound" % (name, pattern, worst))
    if pattern == "dead":                                                # S = 0: exactly 0
        k = cs.sizes[-1] - 50
        assert not cov[4][-1][k].any() and not cov[4][-1][:, k].any() and cov[4][-1].any()
        assert not cov[0][2][3].any() and not cov[0][2][:, 3].any()
    if pattern == "chunk":
        assert all(not unit.any() for unit in cov[2]) and all(unit.any() for unit in cov[3])
        assert all(not np.signbit(unit).any() for unit in cov[2])        # +0.0


def test_covariance_of_cancelling_streams(cm):
    n = SEG + 7                                                          # two segments, the second of 7 samples
    A, B = V.cancelling(31, n, 4, 4)
    x = np.ascontiguousarray(np.concatenate([A.T, B.T]))                 # 8 detectors: <a_i, b_j> cancels to ~1e-9 S
    F = cm.I.PCAFilterLO(np.zeros(8 * n, dtype=np.int32), 8)
    ref, S = R.cov_ref(x.reshape(-1), None, 8, [0, 8], [0, n])
    assert float(np.abs(ref[0][0][:4, 4:]).max() / S[0][0][:4, 4:].min()) < 1e-6
    for use in (True, False):
        got = F.covariance(x.reshape(-1), use_flags=use)[0][0]
        assert same_bits(got, got.T) and R.cov_excess(got, ref[0][0], S[0][0], n) <= 1.0


def test_a_unit_keeps_its_bits_alone_and_inside_a_longer_stream(cm):
    name, pattern = "lengths", "random"
    cs, pix = cov_case(name), cov_flags(name, pattern)
    cov = cov_op(cm, name, pattern).covariance(cs.d)
    d2, p2 = cs.d.reshape(cs.ndet, cs.ns), pix.reshape(cs.ndet, cs.ns)
    for c, g in ((4, 2), (5, 3), (1, 1), (0, 0)):                        # segment + 1, 2 segments + 7, segment - 1, 3
        rows, cols = slice(cs.gedges[g], cs.gedges[g + 1]), slice(cs.cedges[c], cs.cedges[c + 1])
        d1, p1 = np.ascontiguousarray(d2[rows, cols]), np.ascontiguousarray(p2[rows, cols])
        alone = cm.I.PCAFilterLO(p1.reshape(-1), cs.sizes[g]).covariance(d1.reshape(-1))
        assert len(alone) == 1 and len(alone[0]) == 1 and same_bits(alone[0][0], cov[c][g]), (c, g)


def test_a_nan_stays_in_its_row_and_column(cm):
    name = "sizes"
    cs, pix = cov_case(name), cov_flags(name, "random")
    F = cov_op(cm, name, "random")
    clean = F.covariance(cs.d)
    ok = (pix >= 0).reshape(cs.ndet, cs.ns)
    g, c = 7, 4                                                          # the group of three tiles, the chunk of 32
    k = int(cs.gedges[g]) + 2 * TILE + 5
    i_used = int(cs.cedges[c] + np.flatnonzero(ok[k, cs.cedges[c]:cs.cedges[c + 1]])[0])
    i_flag = int(cs.cedges[c] + np.flatnonzero(~ok[k + 1, cs.cedges[c]:cs.cedges[c + 1]])[0])
    d = cs.d.copy().reshape(cs.ndet, cs.ns)
    d[k + 1, i_flag] = np.nan                                            # on a flagged sample: never read
    assert all(same_bits(x, y) for a, b in zip(F.covariance(d.reshape(-1)), clean) for x, y in zip(a, b))
    d[k, i_used] = np.nan
    got = F.covariance(d.reshape(-1))
    a = k - int(cs.gedges[g])
    for cc in range(len(cs.cedges) - 1):
        for gg in range(len(cs.sizes)):
            if (cc, gg) != (c, g):
                assert same_bits(got[cc][gg], clean[cc][gg])
    mine = np.zeros_like(clean[c][g], dtype=bool)
    mine[a, :] = mine[:, a] = True
    assert not np.isfinite(got[c][g][mine]).any() and same_bits(got[c][g][~mine], clean[c][g][~mine])
    rows = slice(cs.gedges[g], cs.gedges[g + 1])                         # learn names the units that are not finite
    F2 = cm.I.PCAFilterLO(np.ascontiguousarray(pix.reshape(cs.ndet, cs.ns)[rows]).reshape(-1), cs.sizes[g],
                          chunks=cs.cedges)
    with pytest.raises(ValueError) as e:
        F2.learn(np.ascontiguousarray(d[rows]).reshape(-1))
    assert "(%d, 0)" % c in str(e.value) and "1 (chunk, group) unit" in str(e.value) and F2.modes is None


# ---------------------------------------------------------- 2: apply, fit, status ----
APPLY_CASES = {1: "ones7", 2: "user2_8", 3: "order1_9", 6: "order2_12", 7: "user7_14", 10: "order3_16"}
APPLY_CEDGES = np.array([0, 1, 255, 256, 257, 513, C.NS], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def apply_modes(K):
    """modes that differ in every chunk and span what the case's own templates span (so that the flag patterns of
    _cmode_ref keep their classes): Phi_c = Phi A_c with A_0 = 1 and A_c = 1 + 0.3 x normals"""
    cs = C.case(APPLY_CASES[K])
    rng = np.random.default_rng(500 + K)
    out = [cs.modes] + [cs.modes @ (np.eye(K) + 0.3 * rng.standard_normal((K, K))) for _ in APPLY_CEDGES[2:]]
    return np.ascontiguousarray(np.stack(out))


@functools.lru_cache(maxsize=None)
def apply_refs(K, pattern):
    cs, d = C.case(APPLY_CASES[K]), C.data(APPLY_CASES[K], pattern)
    f = R.pca_f64(d.pix, cs.ndet, cs.edges, APPLY_CEDGES, apply_modes(K), d.v)
    r = R.pca_ref(d.pix, cs.ndet, cs.edges, APPLY_CEDGES, apply_modes(K), d.v) if pattern != "nan" else None
    return f, r


def apply_op(cm, K, pattern):
    key = ("apply", K, pattern)
    if key not in _ops:
        cs, d = C.case(APPLY_CASES[K]), C.data(APPLY_CASES[K], pattern)
        _ops[key] = cm.I.PCAFilterLO(d.pix, cs.ndet, groups=cs.edges, chunks=APPLY_CEDGES, modes=apply_modes(K))
    return _ops[key]


@pytest.mark.parametrize("K", sorted(APPLY_CASES))
def test_apply_fit_and_status_against_the_restatement(cm, K):
    cs = C.case(APPLY_CASES[K])
    assert cs.K == K and cs.ns == C.NS == 773 and len(cs.sizes) == 1
    G, st = 1, cm.D.stream()
    for pattern in C.PATTERNS:
        d = C.data(APPLY_CASES[K], pattern)
        f64, ref = apply_refs(K, pattern)
        F = apply_op(cm, K, pattern)
        assert same_bits(F.modes, apply_modes(K)) and F.K == K and F.nchunks == 6
        d_in, d_out, d_cf = Guarded(cm, cs.nt, d.v), Guarded(cm, cs.nt), Guarded(cm, G * K * cs.ns)
        d_st = GuardedInt(cm, G * cs.ns, "uint8")
        cm.hip.call("cm2_pca_apply", F._handle.h, d_in.ptr, d_out.ptr, st)
        cm.hip.call("cm2_pca_fit", F._handle.h, d_in.ptr, d_cf.ptr, st)
        cm.hip.call("cm2_pca_status", F._handle.h, d_st.ptr)
        out, cf, status = d_out.get(), d_cf.get().reshape(G, K, cs.ns), d_st.get().reshape(G, cs.ns)
        for g in (d_in, d_out, d_cf, d_st):
            g.intact("K = %d, %s" % (K, pattern))
        assert np.array_equal(status, f64.status)
        count = np.bincount(f64.status.reshape(-1), minlength=4)
        info = F.filter_info()
        assert [info[k] for k in F.CLASSES] == count.tolist() and info["modes_set"] == 1
        assert (info["ns"], info["ndet"], info["ngroups"], info["nchunks"], info["K"]) == (cs.ns, cs.ndet, G, 6, K)
        skipped = np.repeat(f64.status != R.FITTED, cs.sizes, axis=0).reshape(-1)
        assert not out[(d.pix < 0) | skipped].any()
        assert not cf[np.broadcast_to((f64.status != R.FITTED)[:, None, :], cf.shape)].any()
        if pattern == "nan":                     # "random" and one NaN: it stays in its unit, the rest is "random"'s
            g_, s_, k_ = d.nan_at
            f_r, r_r = apply_refs(K, "random")
            col = np.zeros((cs.ndet, cs.ns), dtype=bool)
            col[:, s_] = True
            col = col.reshape(-1)
            assert np.isnan(out[col & (d.pix >= 0)]).all() and not out[col & (d.pix < 0)].any()
            assert np.isnan(cf[0, :, s_]).all() and np.isfinite(np.delete(cf, s_, axis=2)).all()
            cS = C.c_samples(cs.ndet, cs.ns, cs.edges, K)
            C.assert_accepted(out[~col], f_r.out[~col], r_r.out[~col], r_r.S[~col], cS[~col], "apply beside a NaN")
            continue
        assert np.array_equal(f64.status, ref.status)
        same_o = float((R.bits(out) == R.bits(f64.out)).mean())
        same_c = float((R.bits(cf) == R.bits(f64.coeff)).mean())
        eo = C.assert_accepted(out, f64.out, ref.out, ref.S, C.c_samples(cs.ndet, cs.ns, cs.edges, K), "apply")
        ec = C.assert_accepted(cf, f64.coeff, ref.coeff, ref.Sc, C.c_coeffs(cs.ns, cs.edges, K), "fit")
        print("K = %d %s: %.4f of the outputs and %.4f of the coefficients bit-equal to the restatement; the others "
              "use %.3g / %.3g of the bound" % (K, pattern, same_o, same_c, eo, ec))
        y = F * d.v
        assert isinstance(y, np.ndarray) and same_bits(y, out)
        assert same_bits(F.coefficients(d.v), cf) and np.array_equal(F.status(), status)
        assert F.shape == (cs.nt, cs.nt) and F.symmetric


def test_every_class_occurs_in_the_apply_cases():
    seen = np.zeros(4, dtype=np.int64)
    for K in APPLY_CASES:
        for p in C.PATTERNS:
            seen += np.bincount(apply_refs(K, p)[0].status.reshape(-1), minlength=4)
    assert (seen > 0).all(), seen


@pytest.mark.parametrize("K", [1, 6, 10])
def test_in_place_and_repeated_applications_give_the_same_bits(cm, K):
    cs, d = C.case(APPLY_CASES[K]), C.data(APPLY_CASES[K], "random")
    F = apply_op(cm, K, "random")
    st, h = cm.D.stream(), F._handle.h
    d_in, d_a, d_b = Guarded(cm, cs.nt, d.v), Guarded(cm, cs.nt), Guarded(cm, cs.nt)
    cm.hip.call("cm2_pca_apply", h, d_in.ptr, d_a.ptr, st)
    cm.hip.call("cm2_pca_apply", h, d_in.ptr, d_b.ptr, st)
    assert same_bits(d_a.get(), d_b.get())
    cm.hip.call("cm2_pca_apply", h, d_in.ptr, d_in.ptr, st)              # d_out == d_in exactly
    assert same_bits(d_in.get(), d_a.get())
    for g in (d_in, d_a, d_b):
        g.intact("K = %d" % K)


@pytest.mark.parametrize("K", [2, 7])
def test_the_modes_of_every_chunk_are_annihilated(cm, K):
    cs = C.case(APPLY_CASES[K])
    modes = apply_modes(K)
    rng = np.random.default_rng(6)
    v = np.zeros((cs.ndet, cs.ns))
    for c, (a, b) in enumerate(zip(APPLY_CEDGES[:-1], APPLY_CEDGES[1:])):
        v[:, a:b] = modes[c] @ (100.0 * rng.standard_normal((K, b - a)))
    for pattern in ("none", "random"):
        d = C.data(APPLY_CASES[K], pattern)
        r = R.pca_ref(d.pix, cs.ndet, cs.edges, APPLY_CEDGES, modes, v.reshape(-1))
        out = apply_op(cm, K, pattern) * v.reshape(-1)
        # v itself is rounded: one more rounding of every term of S
        c = C.c_samples(cs.ndet, cs.ns, cs.edges, K) + 1
        assert C.excess(out, np.zeros(cs.nt), r.S, c) <= 1.0


# ------------------------------------------- 2b: one unit, two filters, the same bits ----
# The PCA filter and the common-mode filter run the same unit (cm2_modefit.h): the same operations in the same order,
# no contraction, IEEE division and square root.  So where they are given the same detectors, flags, modes and data
# they agree bit for bit, NaNs included -- not within a bound.
def both_filters(F, Fc, v):
    return (F * v, Fc * v), (F.coefficients(v), Fc.coefficients(v)), (F.status(), Fc.status())


@pytest.mark.parametrize("K", [1, 3, 6, 10])
def test_one_chunk_is_the_common_mode_filter_bit_for_bit(cm, K):
    cs = C.case(APPLY_CASES[K])
    assert cs.K == K and cs.ns == C.NS == 773
    for pattern in C.PATTERNS:
        d = C.data(APPLY_CASES[K], pattern)
        F = cm.I.PCAFilterLO(d.pix, cs.ndet, groups=cs.edges, chunks=None, modes=cs.modes[None])
        Fc = cm.I.CommonModeFilterLO(d.pix, cs.ndet, modes=cs.modes, groups=cs.edges)
        assert F.nchunks == 1 and F.K == Fc.K == K
        out, cf, st = both_filters(F, Fc, d.v)
        assert same_bits(*out), pattern
        assert same_bits(*cf) and cf[0].shape == (len(cs.sizes), K, cs.ns), pattern
        assert np.array_equal(*st) and st[0].dtype == np.uint8, pattern
        info, info_c = F.filter_info(), Fc.filter_info()
        assert [info[k] for k in F.CLASSES] == [info_c[k] for k in Fc.CLASSES], pattern
        assert sum(info[k] for k in F.CLASSES) == len(cs.sizes) * cs.ns
        assert np.isnan(out[0]).any() == (pattern == "nan")


@pytest.mark.parametrize("K", [1, 3, 6, 10])
def test_every_chunk_is_a_common_mode_filter_on_its_columns(cm, K):
    """chunks of 1, 254, 1, 1, 256 and 260 samples: a chunk of one sample, chunks that end one short of, on and one
    past the 256-thread slab, and a last chunk that is no multiple of 256"""
    cs, modes = C.case(APPLY_CASES[K]), apply_modes(K)
    assert APPLY_CEDGES.tolist() == [0, 1, 255, 256, 257, 513, 773] and cs.ndet >= K + 1
    for pattern in C.PATTERNS:
        d = C.data(APPLY_CASES[K], pattern)
        F = apply_op(cm, K, pattern)
        out, cf, st = F * d.v, F.coefficients(d.v), F.status()
        pix2, v2 = d.pix.reshape(cs.ndet, cs.ns), d.v.reshape(cs.ndet, cs.ns)
        for c, (a, b) in enumerate(zip(APPLY_CEDGES[:-1], APPLY_CEDGES[1:])):
            Fc = cm.I.CommonModeFilterLO(np.ascontiguousarray(pix2[:, a:b]).reshape(-1), cs.ndet, modes=modes[c],
                                         groups=cs.edges)
            vc = np.ascontiguousarray(v2[:, a:b]).reshape(-1)
            what = (pattern, c)
            assert same_bits(out.reshape(cs.ndet, cs.ns)[:, a:b], (Fc * vc).reshape(cs.ndet, b - a)), what
            assert same_bits(cf[:, :, a:b], Fc.coefficients(vc)), what
            assert np.array_equal(st[:, a:b], Fc.status()), what


# ---------------------------------------------------------------------- 3: chain ----
def test_learn_then_apply_and_the_quality_case(cm):
    q, host = R.quality(), R.quality_on_the_host()
    assert host.gap_filled <= 2.0 and host.unfiltered >= 100.0           # the reference first
    F = cm.I.PCAFilterLO(q.pix, q.ndet, nmodes=q.K, groups=q.gedges, chunks=q.cedges)
    assert F.modes is None and F.filter_info()["modes_set"] == 0
    filled = cm.U.fill_gaps_linear(q.d, q.pix, [q.ns] * q.ndet)
    assert F.learn(filled, use_flags=False) is F
    cov = F.covariance(filled, use_flags=False)
    assert same_bits(F.modes, R.learn(cov, q.ndet, q.gedges, q.K))       # the restated selection, the GPU's covariance
    for c in range(4):
        for g in range(2):
            assert same_bits(F.eigenvalues[c][g], R.select_modes(cov[c][g], q.K)[1])
            assert F.eigenvalues[c][g].shape == (12,) and (np.diff(F.eigenvalues[c][g]) <= 0).all()
    out = F * q.d
    f64 = R.pca_f64(q.pix, q.ndet, q.gedges, q.cedges, F.modes, q.d)
    ref = R.pca_ref(q.pix, q.ndet, q.gedges, q.cedges, F.modes, q.d)
    C.assert_accepted(out, f64.out, ref.out, ref.S, C.c_samples(q.ndet, q.ns, q.gedges, q.K), "learnt modes")
    assert np.array_equal(F.status(), f64.status)
    got, raw = R.rms_over_noise(q, out), R.rms_over_noise(q, q.d)
    print("rms over noise: filtered %.4g (host pipeline %.4g), unfiltered %.4g" % (got, host.gap_filled, raw))
    assert got <= 2.0 and raw >= 100.0


# ------------------------------------------------------------------ 4: end to end ----
def test_a_drifting_atmosphere_does_not_reach_the_map(cm):
    """expand_pointing -> P; d = P m + noise, with and without a two-mode atmosphere a thousand times the noise whose
    detector pattern drifts from chunk to chunk; modes learnt from the gap-filled dirty stream; x = cg(P^T F P,
    P^T F d) for the dirty and for the atmosphere-free stream under the same F.
    The bound: with F fixed the solutions differ by dx = A^-1 P^T F atm, A = P^T F P.  F is a symmetric projector, so
    with r = F atm: dx^T A dx = r^T (F P A^-1 P^T F) r <= |r|^2, because F P A^-1 P^T F is a symmetric projector as
    well.  With rho = dx^T A dx / dx^T dx (the Rayleigh quotient of dx itself) that is |dx| <= |F atm| / sqrt(rho).
    Both solves stop at rtol = 1e-10 of |b|; the residuals are checked to be below 1e-8 |b|, and one part in a
    thousand of the bound is allowed for what they leave in dx.  The rounding of F, P and P^T (1e-13 relative) is
    far below that."""
    nside, nd, K = 16, 12, 2
    npix, ns = 12 * nside * nside, PE.NS
    b, dq = PE.inputs("scan")
    rng = np.random.default_rng(79)
    pixs, c, s = cm.U.expand_pointing(b, dq[:nd], nside)
    drop = cm.torch.from_numpy(rng.random(nd * ns) < 0.05).to(pixs.device)
    pixs[drop] = -1
    ces = cm.U.ProcessTimeSamples(pixs, npix, pol=3, cos_sin=(c, s))
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nd * ns, pixs, pol=3, angle_processed=ces)
    Mbd = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=3)
    gedges, chunk = cm.I.cmode_groups(nd, 6), 1000
    m_true = rng.standard_normal(3 * n)
    base = np.asarray(P * m_true) + rng.standard_normal(nd * ns)
    cedges = cm.I.hwpss_plan(ns, chunk)
    atm = np.zeros((nd, ns))
    t1, t2 = R.one_over_f(rng, ns), R.one_over_f(rng, ns)
    g0, s0 = rng.uniform(0.7, 1.3, nd), rng.uniform(-1.0, 1.0, nd)
    for k, (a, e) in enumerate(zip(cedges[:-1], cedges[1:])):
        atm[:, a:e] = 1.0e3 * (np.outer(g0 * (1 + 0.03 * k), t1[a:e]) + 0.5 * np.outer(s0 + 0.05 * k, t2[a:e]))
    dirty = base + atm.reshape(-1)
    F = cm.I.PCAFilterLO(pixs, nd, nmodes=K, groups=gedges, chunks=cedges)
    F.learn(cm.U.fill_gaps_linear(dirty, cm.D.to_host(pixs), [ns] * nd), use_flags=False)
    info = F.filter_info()
    assert info["fitted"] >= 0.99 * 2 * ns
    A = P.T * F * P
    solve = lambda v: cm.cg(A, np.asarray(P.T * (F * v)), M=Mbd, rtol=1e-10, maxiter=2000)
    (x_dirty, i1), (x_base, i0) = solve(dirty), solve(base)
    assert i1 == 0 and i0 == 0
    x_raw, i2 = cm.cg(P.T * P, np.asarray(P.T * dirty), M=Mbd, rtol=1e-10, maxiter=2000)
    assert i2 == 0
    dx = np.asarray(x_dirty) - np.asarray(x_base)
    lam = float(dx @ np.asarray(A * dx) / (dx @ dx))                     # rho
    left = float(np.linalg.norm(np.asarray(F * atm.reshape(-1))))
    for x, v in ((x_dirty, dirty), (x_base, base)):
        bv = np.asarray(P.T * (F * v))
        assert np.linalg.norm(bv - np.asarray(A * np.asarray(x))) <= 1e-8 * np.linalg.norm(bv)
    bound = left / np.sqrt(lam) * (1.0 + 1e-3)
    off, off_raw = float(np.linalg.norm(dx)), float(np.linalg.norm(np.asarray(x_raw) - np.asarray(x_base)))
    print("maps differ by %.3g (bound %.3g, |F atm| = %.3g, Rayleigh quotient %.3g); unfiltered by %.3g; |m| = %.3g"
          % (off, bound, left, lam, off_raw, float(np.linalg.norm(m_true))))
    assert off <= bound
    assert off_raw >= 100.0 * off                                        # orders of magnitude without the filter


# -------------------------------------------------------------------- 5: refusals ----
def test_refused_calls_leave_their_outputs_untouched(cm):
    K = 3
    cs, d = C.case(APPLY_CASES[K]), C.data(APPLY_CASES[K], "random")
    F = apply_op(cm, K, "random")
    lib, st, h = cm.hip.load(), cm.D.stream(), F._handle.h
    G, ncov = 1, 6 * cs.ndet ** 2
    d_in, d_out, d_cf = Guarded(cm, cs.nt, d.v), Guarded(cm, cs.nt), Guarded(cm, G * K * cs.ns)
    d_cov, d_st = Guarded(cm, ncov), GuardedInt(cm, G * cs.ns, "uint8")
    pix_t, modes_t = F._d_pix, cm.D.f64(apply_modes(K))
    pixp = cm.D.ptr(pix_t)

    def untouched(what):
        for g in (d_out, d_cf, d_cov):
            g.intact(what)
            assert np.isnan(g.get()).all(), what + ": an output was written"
        d_st.intact(what)
        assert (d_st.get() == d_st.fill).all(), what + ": the status was written"
        assert same_bits(d_in.get(), d.v), what

    fresh = cm.I.PCAFilterLO(d.pix, cs.ndet, nmodes=K, groups=cs.edges, chunks=APPLY_CEDGES)     # no modes yet
    h0 = fresh._handle.h
    small = cm.I.PCAFilterLO(d.pix, cs.ndet, nmodes=K, groups=[0, K, cs.ndet], chunks=APPLY_CEDGES)
    refused = [
        ("cm2_pca_apply", (None, d_in.ptr, d_out.ptr, st)),
        ("cm2_pca_apply", (h, None, d_out.ptr, st)),
        ("cm2_pca_apply", (h, d_in.ptr, None, st)),
        ("cm2_pca_apply", (h, d_in.ptr, d_in.ptr + 8, st)),                     # overlapping, not the same
        ("cm2_pca_apply", (h, d_in.ptr, d_in.ptr + 8 * (cs.nt - 1), st)),
        ("cm2_pca_apply", (h, d_in.ptr + 8 * (cs.nt - 1), d_in.ptr, st)),
        ("cm2_pca_apply", (h0, d_in.ptr, d_out.ptr, st)),                       # before modes are set
        ("cm2_pca_fit", (None, d_in.ptr, d_cf.ptr, st)),
        ("cm2_pca_fit", (h, None, d_cf.ptr, st)),
        ("cm2_pca_fit", (h, d_in.ptr, None, st)),
        ("cm2_pca_fit", (h, d_in.ptr, d_in.ptr, st)),
        ("cm2_pca_fit", (h, d_in.ptr, d_in.ptr + 8 * (cs.nt - 1), st)),
        ("cm2_pca_fit", (h0, d_in.ptr, d_cf.ptr, st)),
        ("cm2_pca_status", (None, d_st.ptr)),
        ("cm2_pca_status", (h, None)),
        ("cm2_pca_status", (h0, d_st.ptr)),
        ("cm2_pca_cov", (None, d_in.ptr, pixp, d_cov.ptr, st)),
        ("cm2_pca_cov", (h, None, pixp, d_cov.ptr, st)),
        ("cm2_pca_cov", (h, d_in.ptr, pixp, None, st)),
        ("cm2_pca_cov", (h, d_in.ptr, pixp, d_in.ptr, st)),
        ("cm2_pca_cov", (h, d_in.ptr, pixp, d_in.ptr + 8 * (cs.nt - 1), st)),
        ("cm2_pca_cov", (h, d_in.ptr, pixp, pixp, st)),
        ("cm2_pca_set_modes", (None, cm.D.ptr(modes_t), st)),
        ("cm2_pca_set_modes", (h0, None, st)),
        ("cm2_pca_set_modes", (small._handle.h, cm.D.ptr(modes_t), st)),        # a group of K detectors
    ]
    for fn, args in refused:
        assert getattr(lib, fn)(*args) == cm.hip.ERR_ARGUMENT, (fn, args)
        assert lib.cm2_last_error()
        untouched("%s%r" % (fn, args))
    assert fresh.filter_info()["modes_set"] == 0 and small.filter_info()["modes_set"] == 0
    assert lib.cm2_pca_info(None, (ctypes.c_int64 * 13)()) == cm.hip.ERR_ARGUMENT
    assert lib.cm2_pca_info(h, None) == cm.hip.ERR_ARGUMENT and lib.cm2_pca_cov_doubles(None) == -1
    for call in (lambda: fresh * d.v, lambda: fresh.coefficients(d.v), fresh.status):
        with pytest.raises(cm.hip.HipError):
            call()
    for call in (lambda: small.learn(d.v), lambda: small.set_modes(apply_modes(K))):
        with pytest.raises(ValueError):
            call()
    assert len(small.covariance(d.v)) == 6                               # the covariance takes any grouping
    with pytest.raises(cm.L.lp.ShapeError):
        fresh.set_modes(apply_modes(K)[:, :, :2])
    with pytest.raises(cm.L.lp.ShapeError):
        F * d.v[:-1]
    # create: the handle variable keeps its value
    MARK, I64 = 0x1234, ctypes.c_int64

    def create(ns=cs.ns, ndet=cs.ndet, gedges=cs.edges, cedges=APPLY_CEDGES, K=K, pix=pix_t, out=True):
        ge = None if gedges is None else (I64 * len(gedges))(*[int(x) for x in gedges])
        ce = None if cedges is None else (I64 * len(cedges))(*[int(x) for x in cedges])
        ng = 0 if gedges is None else len(gedges) - 1
        nc = 0 if cedges is None else len(cedges) - 1
        hv = ctypes.c_void_p(MARK)
        rc = lib.cm2_pca_create(ctypes.byref(hv) if out else None, ns, ndet, ng, ge, nc, ce, K, cm.D.ptr(pix), st)
        return rc, hv

    for kw in (dict(K=0), dict(K=11), dict(K=-1), dict(ns=0, cedges=[0, 0]), dict(ndet=0, gedges=[0, 0]),
               dict(gedges=[0]), dict(gedges=[0, cs.ndet - 1]), dict(gedges=[1, cs.ndet]),
               dict(gedges=[0, 4, 4, cs.ndet]), dict(gedges=[0, 6, 3, cs.ndet]), dict(gedges=None),
               dict(cedges=[0]), dict(cedges=[0, cs.ns - 1]), dict(cedges=[1, cs.ns]), dict(cedges=[0, 300, 300, cs.ns]),
               dict(cedges=[0, 500, 200, cs.ns]), dict(cedges=None), dict(pix=None),
               dict(ns=1 << 30, ndet=(1 << 16) + 2, gedges=[0, (1 << 16) + 2], cedges=[0, 1 << 30]),
               dict(ns=4, ndet=(1 << 23) + 2, gedges=[0, (1 << 23) + 2], cedges=[0, 4]),
               dict(ns=1 << 45, ndet=2, gedges=[0, 2], cedges=[0, 1 << 45])):
        rc, hv = create(**kw)
        assert rc == cm.hip.ERR_ARGUMENT and hv.value == MARK, kw
        assert lib.cm2_last_error()
    assert create(out=False)[0] == cm.hip.ERR_ARGUMENT
    untouched("after the refused creates")
    rc, hv = create()
    assert rc == 0 and hv.value not in (None, MARK)
    assert lib.cm2_pca_set_modes(hv, cm.D.ptr(modes_t), st) == 0
    assert lib.cm2_pca_apply(hv, d_in.ptr, d_out.ptr, st) == 0
    assert lib.cm2_pca_status(hv, d_st.ptr) == 0
    assert lib.cm2_pca_cov(hv, d_in.ptr, pixp, d_cov.ptr, st) == 0
    assert same_bits(d_out.get(), F * d.v) and np.array_equal(d_st.get().reshape(1, -1), F.status())
    assert same_bits(d_cov.get(), np.concatenate([u.reshape(-1) for row in F.covariance(d.v) for u in row]))
    for g in (d_out, d_st, d_cov):
        g.intact("valid calls")
    assert lib.cm2_pca_destroy(hv) == 0 and lib.cm2_pca_destroy(None) == 0
