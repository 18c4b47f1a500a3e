"""
The glitch flagger on the GPU against the NumPy restatement of _glitch_ref.py: residuals compared with ==, classes,
counts and sigma bit for bit.  The shapes are the smallest at which the kernels can go wrong (the lists are in
_glitch_ref.py and checked in test_glitch_cpu.py); outputs sit in the sentinel-guarded buffers of _guarded.py.
"""

import numpy as np
import pytest

import _glitch_ref as R
from _guarded import Guarded, GuardedInt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.utilities import glitches as G
    from types import SimpleNamespace
    return SimpleNamespace(I=I, U=U, G=G, hip=_hip, torch=torch, D=D)


def case_of(d, flags=None, prev=None):
    from types import SimpleNamespace
    return SimpleNamespace(d=d, flags=flags, prev=prev)


def same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


class Raw(object):
    """The C entry points on guarded buffers: every output comes back with its guards checked."""

    def __init__(self, cm, sizes, h):
        self.cm, self.sizes, self.nt, self.nb = cm, sizes, sum(sizes), len(sizes)
        self.g = cm.G._Glitch(self.nt, sizes, h)

    def stream(self, c):
        cm = self.cm
        self.d = Guarded(cm, self.nt, c.d)
        if c.flags is not None and c.flags.dtype == np.uint8:        # bytes as a uint8 tensor brings them: kind 1
            self.f, self.kind = cm.D.to_dev(c.flags), 1
        else:
            self.f, self.kind = (None, 0) if c.flags is None else cm.G._flags_to_dev(c.flags)
        self.prev = None if c.prev is None else cm.D.to_dev(c.prev)
        return self

    def _args(self):
        return self.cm.D.ptr(self.f), self.kind, self.cm.D.ptr(self.prev)

    def residual(self):
        r = Guarded(self.cm, self.nt)
        f, kind, prev = self._args()
        self.cm.hip.call("cm2_glitch_residual", self.g.h, self.d.ptr, f, kind, prev, r.ptr, self.cm.D.stream())
        out = r.get()
        r.intact("cm2_glitch_residual")
        self.d.intact("cm2_glitch_residual (input)")
        return out

    def scale(self, r):
        rr, s = Guarded(self.cm, self.nt, r), Guarded(self.cm, self.nb)
        f, kind, prev = self._args()
        self.cm.hip.call("cm2_glitch_scale", self.g.h, self.d.ptr, rr.ptr, f, kind, prev, s.ptr, self.cm.D.stream())
        out = s.get()
        s.intact("cm2_glitch_scale")
        return out

    def classify(self, r, sigma, nsigma, grow):
        rr, s = Guarded(self.cm, self.nt, r), Guarded(self.cm, self.nb, sigma)
        cls, counts = GuardedInt(self.cm, self.nt, "uint8"), GuardedInt(self.cm, self.nb * 5, "int64")
        f, kind, prev = self._args()
        self.cm.hip.call("cm2_glitch_classify", self.g.h, self.d.ptr, rr.ptr, f, kind, prev, s.ptr, float(nsigma),
                         int(grow), cls.ptr, counts.ptr, self.cm.D.stream())
        out = cls.get(), counts.get().reshape(self.nb, 5)
        cls.intact("cm2_glitch_classify (classes)")
        counts.intact("cm2_glitch_classify (counts)")
        return out


# ------------------------------------------------------------------------------ median ----
@pytest.mark.parametrize("name", R.MEDIAN_CASES)
def test_residual_and_scale_of_the_median_cases(cm, name):
    c, want = R.median_case(name), R.median_expected(name)
    raw = Raw(cm, c.sizes, c.h).stream(c)
    r = raw.residual()
    bad = np.flatnonzero(~(r == want.r))
    assert bad.size == 0, (name, bad[:10], r[bad[:10]], want.r[bad[:10]])
    sigma = raw.scale(r)
    assert same_bits(sigma, want.sigma), (name, sigma, want.sigma)
    info = raw.g.info()
    assert (info["nt"], info["nblocks"], info["half_width"], info["run"], info["tier"]) == \
        (sum(c.sizes), len(c.sizes), c.h, R.RUN, R.tier_of(c.h))
    assert info["bytes"] == 3 * 8 * (len(c.sizes) + 1) + 24 * len(c.sizes) + 8192 * len(c.sizes)


def test_python_layer_gives_the_same_residual_and_scale(cm):
    c, want = R.median_case("prev_and_flags"), R.median_expected("prev_and_flags")
    gf = cm.U.GlitchFlagger(c.sizes, half_width=c.h)
    for d, flags, prev in ((c.d, c.flags, c.prev), (cm.D.f64(c.d), cm.D.i32(c.flags), cm.D.to_dev(c.prev)),
                           (c.d, c.flags < 0, c.prev), (c.d, c.flags.astype(np.int64), c.prev)):
        r = gf.residual(d, flags=flags, prev=prev)
        assert cm.D.is_dev(r) and r.dtype == cm.torch.float64
        assert np.array_equal(cm.D.to_host(r) == want.r, np.ones(want.r.size, dtype=bool))
        sigma = gf.scale(d, r, flags=flags, prev=prev)
        assert cm.D.is_dev(sigma) and same_bits(cm.D.to_host(sigma), want.sigma)
    assert gf.info(sum(c.sizes))["tier"] == 0


# --------------------------------------------------------------------------- selection ----
@pytest.mark.parametrize("name", R.SELECTION_CASES)
def test_selection(cm, name):
    c = R.selection_case(name)
    want, _ = R.scale(c.d, c.r, c.sizes, c.h, c.flags)
    raw = Raw(cm, c.sizes, c.h).stream(c)
    for _ in range(2):                                       # the second call finds the histograms cleared
        sigma = raw.scale(c.r)
        assert same_bits(sigma, want), (name, sigma, want)


# ------------------------------------------------------------------ threshold and grow ----
@pytest.mark.parametrize("grow", [0, 1, 64])
@pytest.mark.parametrize("sigma", [R.SIGMA_GIVEN, 0.0, np.inf])
def test_threshold_and_grow(cm, grow, sigma):
    s = R.spike_case()
    raw = Raw(cm, s.sizes, s.h).stream(case_of(s.d, s.flags))
    r = raw.residual()
    ok = np.isfinite(s.d) & (s.flags >= 0)
    assert np.array_equal(r[ok], s.d[ok])                    # r = d exactly
    want_cls, want_counts = R.classify(s.d, r, s.sizes, [sigma] * 2, R.NSIGMA, grow, s.flags)
    cls, counts = raw.classify(r, [sigma] * 2, R.NSIGMA, grow)
    assert np.array_equal(cls, want_cls), np.flatnonzero(cls != want_cls)[:10]
    assert np.array_equal(counts, want_counts) and counts.sum(axis=1).tolist() == s.sizes
    if sigma == R.SIGMA_GIVEN:
        assert cls[100] == cls[400] == R.CLEAN and cls[200] == cls[300] == R.HIT          # equality is no hit
        assert cls[2999] == R.HIT and cls[3000] == R.CLEAN                                # no NEAR across a block
        assert cls[999] == cls[1001] == R.INPUT
    if sigma == 0.0:
        assert (cls[ok & (s.d != 0)] == R.HIT).all()
    if np.isinf(sigma):
        assert counts[:, R.HIT].sum() == 0 and counts[:, R.NEAR].sum() == 0


def test_classes_with_prev_and_both_flag_encodings(cm):
    c = R.median_case("prev_and_flags")
    want_r = R.median_expected("prev_and_flags").r
    sigma = [0.3, 0.4]
    for flags in (c.flags, c.flags < 0):
        raw = Raw(cm, c.sizes, c.h).stream(case_of(c.d, flags, c.prev))
        want_cls, want_counts = R.classify(c.d, want_r, c.sizes, sigma, 2.0, 3, flags, c.prev)
        cls, counts = raw.classify(want_r, sigma, 2.0, 3)
        assert np.array_equal(cls, want_cls) and np.array_equal(counts, want_counts)
        assert (cls[(c.flags >= 0) & np.isin(c.prev, (R.HIT, R.NEAR))] == c.prev[(c.flags >= 0) &
                                                                                 np.isin(c.prev, (R.HIT, R.NEAR))]).all()


def test_flag_with_a_given_sigma(cm):
    s = R.spike_case()
    want, winfo = R.flag(s.d, s.sizes, s.h, s.flags, nsigma=R.NSIGMA, grow=1, iterations=1, sigma=R.SIGMA_GIVEN)
    for sigma in (R.SIGMA_GIVEN, [R.SIGMA_GIVEN] * 2, cm.D.f64(np.full(2, R.SIGMA_GIVEN))):
        cls, info = cm.U.flag_glitches(s.d, s.sizes, flags=s.flags, half_width=s.h, nsigma=R.NSIGMA, grow=1,
                                       iterations=1, sigma=sigma)
        assert cm.D.is_dev(cls) and cls.dtype == cm.torch.uint8
        assert np.array_equal(cm.D.to_host(cls), want)
        assert np.array_equal(info["counts"], winfo["counts"]) and info["passes"] == 1
        assert same_bits(info["sigma"], np.full(2, R.SIGMA_GIVEN)) and info["hits_per_pass"] == winfo["hits_per_pass"]


# --------------------------------------------------------------------------- iteration ----
def test_iteration_follows_the_restatement(cm):
    c = R.iteration_case()
    gf = cm.U.GlitchFlagger(c.sizes, half_width=c.h)
    cls, info = gf.flag(c.d, nsigma=5.0, grow=0, iterations=3)
    assert info["passes"] == c.info["passes"] == 3 and info["hits_per_pass"] == c.info["hits_per_pass"]
    assert info["hits_per_pass"][1] >= 1 and info["hits_per_pass"][2] == 0
    assert np.array_equal(cm.D.to_host(cls), c.cls)
    assert np.array_equal(info["counts"], c.info["counts"]) and same_bits(info["sigma"], c.info["sigma"])
    assert info["short_blocks"].size == 0
    for k in (1, 2):                                                  # stopped early: the classes of that pass
        cls_k, info_k = gf.flag(c.d, nsigma=5.0, grow=0, iterations=k)
        assert np.array_equal(cm.D.to_host(cls_k), c.info["each"][k - 1].cls) and info_k["passes"] == k
        assert same_bits(info_k["sigma"], c.info["each"][k - 1].sigma)


def test_short_blocks_are_reported(cm):
    c = R.selection_case("short_and_exact")
    d = np.random.default_rng(9).standard_normal(sum(c.sizes))
    want, winfo = R.flag(d, c.sizes, c.h, c.flags, nsigma=3.0, grow=1, iterations=2)
    cls, info = cm.U.GlitchFlagger(c.sizes, c.h).flag(d, flags=c.flags, nsigma=3.0, grow=1, iterations=2)
    assert np.array_equal(cm.D.to_host(cls), want) and same_bits(info["sigma"], winfo["sigma"])
    assert info["short_blocks"].tolist() == winfo["short_blocks"].tolist() and 0 in info["short_blocks"] \
        and 4 in info["short_blocks"]
    assert info["hits_per_pass"] == winfo["hits_per_pass"]


# ------------------------------------------------------------------ guards and overlap ----
def test_overlaps_and_bad_arguments_are_refused(cm):
    nt, sizes = 1000, [600, 400]
    g = cm.G._Glitch(nt, sizes, 4)
    buf = Guarded(cm, 2 * nt, np.zeros(2 * nt))
    before = buf.get()
    p = buf.ptr
    sig, cls, counts = cm.D.zeros(2), cm.D.zeros(nt, cm.torch.uint8), cm.D.zeros(10, cm.torch.int64)
    st = cm.D.stream()

    def refused(name, *args):
        with pytest.raises(cm.hip.HipError) as e:
            cm.hip.call(name, *args)
        assert e.value.status == cm.hip.ERR_ARGUMENT and name in str(e.value), str(e.value)

    refused("cm2_glitch_residual", g.h, p, None, 0, None, p, st)                     # d_r is d_in
    refused("cm2_glitch_residual", g.h, p, None, 0, None, p + 8 * (nt - 1), st)      # one shared sample
    refused("cm2_glitch_residual", g.h, p + 8 * 5, None, 0, None, p, st)
    refused("cm2_glitch_residual", g.h, p, cm.D.ptr(cls), 2, None, p + 8 * nt, st)   # flag_kind
    refused("cm2_glitch_residual", g.h, p, None, 0, None, None, st)
    refused("cm2_glitch_scale", g.h, p, p + 8 * nt, None, 0, None, p + 8, st)        # sigma inside d_in
    refused("cm2_glitch_classify", g.h, p, p + 8 * nt, None, 0, cm.D.ptr(cls), cm.D.ptr(sig), 5.0, 2, cm.D.ptr(cls),
            cm.D.ptr(counts), st)                                                    # classes in place of prev
    refused("cm2_glitch_classify", g.h, p, p + 8 * nt, None, 0, None, cm.D.ptr(sig), 5.0, 2, p + 16,
            cm.D.ptr(counts), st)                                                    # classes inside d_in
    refused("cm2_glitch_classify", g.h, p, p + 8 * nt, None, 0, None, cm.D.ptr(sig), 0.0, 2, cm.D.ptr(cls),
            cm.D.ptr(counts), st)
    refused("cm2_glitch_classify", g.h, p, p + 8 * nt, None, 0, None, cm.D.ptr(sig), 5.0, 65, cm.D.ptr(cls),
            cm.D.ptr(counts), st)
    assert same_bits(buf.get(), before)
    buf.intact("refused calls")
    # the last sample of d_in next to the first of d_r is no overlap
    cm.hip.call("cm2_glitch_residual", g.h, p, None, 0, None, p + 8 * nt, st)
    assert not buf.get().any()
    buf.intact("cm2_glitch_residual")


def test_apply_flags(cm):
    rng = np.random.default_rng(11)
    nt = 5000
    pix = rng.integers(-1, 100, nt).astype(np.int32)
    cls = rng.choice(np.array([0, 0, 0, 1, 2, 3, 4], dtype=np.uint8), nt)
    want = np.where(cls != 0, -1, pix).astype(np.int32)
    out = cm.U.apply_flags(pix, cls)                                   # an array: a copy
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and np.array_equal(out, want)
    assert not np.array_equal(pix, want)
    out = cm.U.apply_flags(pix.astype(np.int64), cm.D.to_dev(cls))
    assert np.array_equal(out, want)
    guarded = GuardedInt(cm, nt, "int32", pix)
    out = cm.U.apply_flags(guarded.v, cm.D.to_dev(cls))                # a tensor in HBM: in place
    assert out.data_ptr() == guarded.v.data_ptr() and np.array_equal(guarded.get(), want)
    guarded.intact("cm2_glitch_apply_pix")


# --------------------------------------------------------------------------- end to end ----
def test_end_to_end(cm):
    e = R.end_to_end()
    pix_dev = cm.D.i32(e.pix)
    cls, info = cm.U.flag_glitches(cm.D.f64(e.d), e.sizes, flags=pix_dev, half_width=16, nsigma=5.0, grow=2,
                                   iterations=3)
    got = cm.D.to_host(cls)
    assert np.array_equal(got, e.cls) and np.array_equal(info["counts"], e.info["counts"])
    assert same_bits(info["sigma"], e.info["sigma"]) and info["passes"] == e.info["passes"]
    assert info["hits_per_pass"] == e.info["hits_per_pass"] and info["short_blocks"].size == 0
    hits = np.flatnonzero(got == R.HIT)
    assert np.isin(e.where, hits).all()                                # 1. every injected position is a hit
    assert np.setdiff1d(hits, e.where).size <= 2                       # 2. at most 2 hits elsewhere
    # 3. the flagged stream and the clean one give the same right-hand side, bit for bit
    pixs = cm.U.apply_flags(e.pix, cls)
    assert (pixs[e.where] == -1).all() and np.array_equal(pixs < 0, got != 0)
    assert (e.d == e.clean)[pixs >= 0].all()                           # every sample where they differ is skipped
    nt = sum(e.sizes)
    ces = cm.U.ProcessTimeSamples(pixs, e.npix, pol=1)               # (renumbers pixs in place, as SparseLO wants it)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pixs, pol=1, angle_processed=ces)
    N = cm.I.BlockLO(e.sizes[0], [1.0 / s ** 2 for s in info["sigma"]])
    b_glitched, b_clean = P.T * N * e.d, P.T * N * e.clean
    assert same_bits(b_glitched, b_clean) and np.isfinite(b_clean).all() and b_clean.any()
    # the gap filler takes the flagged pixs
    bands = [np.array([1.0, -0.2, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0]) / s ** 2 for s in info["sigma"]]
    Nt = cm.I.BlockLO(e.sizes, bands, offdiag=True)
    gap = cm.U.GapFiller(pixs, Nt)
    assert gap.ng == int((pixs < 0).sum()) >= int((got != 0).sum())
    filled, rc = gap.fill(e.d, rtol=1e-8, maxiter=200)
    assert rc == 0 and np.array_equal(filled[pixs >= 0], e.clean[pixs >= 0]) and np.isfinite(filled).all()
    assert np.abs(filled[e.where]).max() < 10.0                        # the glitches are gone from the stream
