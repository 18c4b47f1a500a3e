"""
Cases and float64 restatements for the time-order pointing kernels (csrc/cm2_pointing.hip, csrc/cm2_pixindex.hip)
and the per-pixel kernels (csrc/cm2_pixel.hip).  NumPy only; tests/test_pixel_ref_cpu.py proves the restatements
against the oracle's serial loops and asserts the feature every case claims, tests/test_gpu_pointing_kernels.py and
tests/test_gpu_pixel_kernels.py compare the kernels with them bit for bit.

Every case is laid out by construction: hit counts are prescribed per pixel, the samples are interleaved by a
fixed-seed permutation, the flagged samples (pixel id -1) are counted in.  Every expression keeps the kernel's
association, e.g. (w*c)*c and 0.0 + (x0 + x1*c + x2*s); the serial per-pixel sums are np.add.at in sample order.

The *_struct functions restate the same operations through the structure the kernels have (stable radix sort on
end_bit bits, unrolled body plus tail, chunked hot sums, rank of the last pixel plus its keep flag).  With their
defaults they equal the plain forms; with one argument altered they are the wrong variants that the cases must catch.
"""
import functools
from types import SimpleNamespace

import numpy as np

SLICE = 64                   # pixels per sliced-ELL slice (one wavefront)
GRID_TRIP = 2048 * 256       # elements per grid-stride trip of a capped grid (grid_for)
HOT_MIN = 8192               # kWeightsHotMin
CHUNK = 4096                 # kWeightsChunk
POW2 = (63, 64, 65, 4095, 4096, 4097)
TAIL_HITS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17)     # 6 and 14: a tail of 6 rows, a tail of 2 after a body


# ----------------------------------------------------------------------------------- cases ----
def _layout(name, hits, nflag, seed):
    hits = np.asarray(hits, dtype=np.int64)
    npix = hits.size
    rng = np.random.default_rng(seed)
    pix = np.concatenate([np.repeat(np.arange(npix, dtype=np.int32), hits), np.full(nflag, -1, dtype=np.int32)])
    pix = np.ascontiguousarray(pix[rng.permutation(pix.size)])
    nt = pix.size
    phi = rng.uniform(0.0, np.pi, nt)
    cs = SimpleNamespace(name=name, npix=npix, nt=nt, hits=hits, nflag=int(nflag), pix=pix, phi=phi,
                         cos=np.cos(2. * phi), sin=np.sin(2. * phi), w=rng.uniform(0.5, 2.0, nt),
                         w2=rng.uniform(0.5, 2.0, nt), v=rng.standard_normal(nt), x=rng.standard_normal(3 * npix))
    if nt:
        cs.v[0], cs.x[2], cs.x[-1] = -0.0, -0.0, 5e-324           # a signed zero and a denormal among the data
    return cs


def _hits_tails():
    return np.resize(np.asarray(TAIL_HITS), 130)                  # 9 or 10 pixels of every count


def _hits_pow2(npix):
    h = np.where(np.arange(npix) % 3 == 1, 0, 1 + (np.arange(npix) * 5) % 3)
    h[0] = h[-1] = 2
    return h


def _hits_hot():
    h = np.zeros(128, dtype=np.int64)
    h[:64] = 1 + np.arange(64) % 3
    h[5] = 20000
    return h


def _hits_stride():
    h = np.zeros(524293, dtype=np.int64)
    h[0:400000:2] = 2
    h[1:400000:2] = 1
    h[-1] = 1
    return h


def _hits_hotw():
    h = 1 + (np.arange(64) * 7) % 40
    h[[3, 20, 41, 63]] = (8191, 8192, 8193, 3 * CHUNK + 255)
    return h


_LAYOUTS = {
    "tails": lambda: _layout("tails", _hits_tails(), 100, 11),
    "empty-flagged": lambda: _layout("empty-flagged", np.zeros(70, dtype=np.int64), 20, 12),
    "empty-nt0": lambda: _layout("empty-nt0", np.zeros(70, dtype=np.int64), 0, 13),
    "hot": lambda: _layout("hot", _hits_hot(), 50, 14),
    "stride": lambda: _layout("stride", _hits_stride(), 5000, 15),
    "hotw": lambda: _layout("hotw", _hits_hotw(), 300, 16),
}
for _n in POW2:
    _LAYOUTS["pow2-%d" % _n] = functools.partial(
        lambda n: _layout("pow2-%d" % n, _hits_pow2(n), n // 8 + 3, 100 + n), _n)

POINTING_CASES = ["tails"] + ["pow2-%d" % n for n in POW2] + ["empty-flagged", "empty-nt0", "hot", "stride"]
SMALL = [c for c in POINTING_CASES if c != "stride"]
WEIGHT_CASES = ["tails", "pow2-64", "pow2-4096", "stride"]


@functools.lru_cache(maxsize=None)
def case(name):
    return _LAYOUTS[name]()


def pols_of(name):
    return (1, 3) if name.startswith("pow2") else (1, 2, 3)


def assert_bit_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float64:
        bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    else:
        bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %r, want %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def differing(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return int((a.view(np.int64) != b.view(np.int64)).sum())


# ------------------------------------------------------------------- the sliced-ELL plan ----
def end_bit(npix):
    """bits of the radix-sort key: the keys take the values 0..npix (npix = flagged)"""
    b = 1
    while (1 << b) <= npix:
        b += 1
    return b


def nslices(npix):
    return -(-npix // SLICE)


def sell_len(hits):
    """64 x the sum over slices of the largest hit count of the slice; pixels in descending hit count, padded to a
    multiple of 64 with empty slots"""
    h = np.sort(np.asarray(hits, dtype=np.int64))[::-1]
    h = np.concatenate([h, np.zeros(nslices(h.size) * SLICE - h.size, dtype=np.int64)])
    return int(SLICE * h.reshape(-1, SLICE).max(axis=1).sum())


def sell_direct(cs):
    """the plan built slot by slot, as k_counts / the stable descending sort / k_pad_slots / k_slice_len /
    k_fill_sell do -> (sell_pix, sell_cnt, slice_ptr, sell_t with 0xFFFFFFFF in the padding rows)"""
    order = np.argsort(-cs.hits, kind="stable")
    nslots = nslices(cs.npix) * SLICE
    sell_pix = np.full(nslots, -1, dtype=np.int64)
    sell_cnt = np.zeros(nslots, dtype=np.int64)
    sell_pix[:cs.npix], sell_cnt[:cs.npix] = order, cs.hits[order]
    slice_ptr = [0]
    for s in range(nslots // SLICE):
        slice_ptr.append(slice_ptr[-1] + SLICE * int(sell_cnt[s * SLICE]))
    sell_t = np.full(slice_ptr[-1], 0xFFFFFFFF, dtype=np.int64)
    samples = [np.flatnonzero(cs.pix == p) for p in range(cs.npix)] if cs.npix <= 4097 else None
    if samples is not None:
        for slot in range(nslots):
            if sell_pix[slot] >= 0:
                t = samples[sell_pix[slot]]
                sell_t[slice_ptr[slot // SLICE] + (slot % SLICE) + SLICE * np.arange(t.size)] = t
    return sell_pix, sell_cnt, np.asarray(slice_ptr), sell_t


def pixindex(pix, npix, key_bits=None):
    """build_pixindex: stable sort of (key, sample) on the low key_bits bits (default end_bit(npix)), ptr by lower
    bound -> (sorted_t, ptr[npix + 1], sorted keys).  Flagged samples get the key npix."""
    bits = end_bit(npix) if key_bits is None else key_bits
    keys = np.where(pix < 0, npix & ((1 << bits) - 1), pix).astype(np.int64)
    sorted_t = np.argsort(keys, kind="stable")
    sk = keys[sorted_t]
    return sorted_t, np.searchsorted(sk, np.arange(npix + 1), side="left"), sk


# --------------------------------------------------------------------- P, P^T, P^T W P ----
def _xk(x, pol, p):
    return [x[pol * p + k] for k in range(pol)]


def P(pol, pix, c, s, x):
    """k_P_time: 0.0 + value for a valid sample, 0.0 for a flagged one"""
    ok = pix >= 0
    p = np.where(ok, pix, 0).astype(np.int64)
    if pix.size == 0:
        return np.zeros(0)
    xs = _xk(np.asarray(x), pol, p)
    if pol == 1:
        val = xs[0]
    elif pol == 2:
        val = xs[0] * c + xs[1] * s
    else:
        val = xs[0] + xs[1] * c + xs[2] * s
    return np.where(ok, 0.0 + val, 0.0)


def _scatter(pol, npix, p, terms):
    out = np.zeros(pol * npix)
    for k, t in enumerate(terms):
        np.add.at(out, pol * p + k, t)               # in the order of p: the serial loop's order per pixel
    return out


def _pt_terms(pol, v, c, s):
    return [v] if pol == 1 else [v * c, v * s] if pol == 2 else [v, v * c, v * s]


def Pt(pol, npix, pix, c, s, v):
    """k_Pt_sell: per pixel the terms of its samples added in time order to 0.0; every pixel is written"""
    t = np.flatnonzero(pix >= 0)
    return _scatter(pol, npix, pix[t].astype(np.int64), _pt_terms(pol, v[t], c[t], s[t]))


def _fused_terms(pol, x, p, c, s, w):
    xs = _xk(np.asarray(x), pol, p)
    if pol == 1:
        return [w * (0.0 + xs[0])]
    if pol == 2:
        vv = w * (0.0 + (xs[0] * c + xs[1] * s))
        return [vv * c, vv * s]
    vv = w * (0.0 + (xs[0] + xs[1] * c + xs[2] * s))
    return [vv, vv * c, vv * s]


def fused(pol, npix, pix, c, s, w, x):
    """k_PtNP_sell: d = P x of the sample, vv = w * d, vv * (1, c, s) added in time order; w None: 1.0"""
    t = np.flatnonzero(pix >= 0)
    p = pix[t].astype(np.int64)
    wt = np.ones(t.size) if w is None else w[t]
    return _scatter(pol, npix, p, _fused_terms(pol, x, p, c[t], s[t], wt))


def _struct_rows(cs, unroll, drop_tail, key_bits):
    """samples in the order a lane of the plan visits them; drop_tail: only the rows of the unrolled body"""
    sorted_t, ptr, sk = pixindex(cs.pix, cs.npix, key_bits)
    nv = ptr[cs.npix]
    t, p = sorted_t[:nv], sk[:nv]
    if drop_tail:
        cnt = np.diff(ptr)
        rank = np.arange(nv) - ptr[p]
        keep = rank < (cnt[p] // unroll) * unroll
        t, p = t[keep], p[keep]
    return t, p


def Pt_struct(cs, pol, drop_tail=False, key_bits=None):
    t, p = _struct_rows(cs, 4, drop_tail, key_bits)
    return _scatter(pol, cs.npix, p, _pt_terms(pol, cs.v[t], cs.cos[t], cs.sin[t]))


def fused_struct(cs, pol, drop_tail=False, key_bits=None):
    t, p = _struct_rows(cs, 8, drop_tail, key_bits)
    return _scatter(pol, cs.npix, p, _fused_terms(pol, cs.x, p, cs.cos[t], cs.sin[t], cs.w[t]))


# ------------------------------------------------------------------------- weight sums ----
WSUMS = ("counts", "cosine", "sine", "cos2", "sin2", "sincos")
WRITTEN = {1: ("counts",), 2: ("cos2", "sin2", "sincos"), 3: WSUMS}


def _wterms(w, c, s):
    return dict(counts=w, cosine=w * c, sine=w * s, cos2=(w * c) * c, sin2=(w * s) * s, sincos=(w * s) * c)


def hot_sum(terms, chunk=CHUNK):
    """k_weights_hot + k_weights_hot_combine: chunks of `chunk` terms from the pixel's first sample; thread t of 256
    adds the terms at positions t, t + 256, ... of the chunk to 0.0; red[t] += red[t + half] for half = 128 ... 1;
    the chunk sums are added in ascending order to 0.0.  (Padding a chunk with +0.0 changes no bit: a running sum
    that started at +0.0 is never -0.0.)"""
    total = np.float64(0.0)
    for b in range(0, terms.size, chunk):
        part = terms[b:b + chunk]
        pad = np.zeros(-(-part.size // 256) * 256)
        pad[:part.size] = part
        red = np.zeros(256)
        for row in pad.reshape(-1, 256):
            red = red + row
        half = 128
        while half >= 1:
            red[:half] = red[:half] + red[half:2 * half]
            half //= 2
        total = total + red[0]
    return total


def weights(cs, pol, w, order="serial", chunk=CHUNK):
    """cm2_weights_accumulate -> {name: array of npix, or None where pol does not write it}.  order "hot": pixels
    with at least HOT_MIN samples are summed by hot_sum, as the library does by default."""
    t = np.flatnonzero(cs.pix >= 0)
    p = cs.pix[t].astype(np.int64)
    wt = np.ones(t.size) if w is None else w[t]
    terms = _wterms(wt, cs.cos[t], cs.sin[t])
    out = dict.fromkeys(WSUMS)
    for name in WRITTEN[pol]:
        out[name] = np.zeros(cs.npix)
        np.add.at(out[name], p, terms[name])
    if order == "hot":
        for hp in np.flatnonzero(cs.hits >= HOT_MIN):
            sel = p == hp
            for name in WRITTEN[pol]:
                out[name][hp] = hot_sum(terms[name][sel], chunk)
    return out


def hot_share(cs, pol, w, got):
    """the largest |got - exact| / ((n + 2) 2^-53 sum |term|) over the hot pixels and the sums of pol: n - 1 additions
    and at most two product roundings per term.  exact: the np.longdouble sum of the terms formed in np.longdouble."""
    L = np.longdouble
    worst = 0.0
    for hp in np.flatnonzero(cs.hits >= HOT_MIN):
        t = np.flatnonzero(cs.pix == hp)
        wt = np.ones(t.size, dtype=L) if w is None else w[t].astype(L)
        terms = _wterms(wt, cs.cos[t].astype(L), cs.sin[t].astype(L))
        for name in WRITTEN[pol]:
            exact, mag = terms[name].sum(dtype=L), np.abs(terms[name]).sum(dtype=L)
            bound = L(t.size + 2) * L(2.0) ** -53 * mag
            worst = max(worst, float(abs(L(got[name][hp]) - exact) / bound))
    return worst


# ------------------------------------------------------------ mask, compaction, flagging ----
def pixel_mask(pol, counts, cos2, sin2, sincos, threshold):
    """k_pixel_mask -> (keep as uint8, cond)"""
    if pol == 1:
        return (counts > 0.0).astype(np.uint8), None
    with np.errstate(all="ignore"):
        det = (cos2 * sin2) - (sincos * sincos)
        tr = cos2 + sin2
        sq = np.sqrt(tr * tr / 4. - det)
        lmax = tr / 2. + sq
        lmin = tr / 2. - sq
        cond = np.abs(lmax / lmin)
        k = cond <= threshold
    if pol == 3:
        k = k & (counts > 2.0)
    return k.astype(np.uint8), cond


THRESHOLDS = (1e3, float(np.nextafter(1e3, 0.0)))
# (counts, cos2, sin2, sincos) -> what the row is for
MASK_ROWS = [
    (5.0, 1000.0, 1.0, 0.0),                         # 0: cond = 1000.0 exactly
    (5.0, 0.0, 0.0, 0.0),                            # 1: 0/0 = NaN
    (5.0, 1.0, 0.0, 0.0),                            # 2: lmin = 0 -> inf
    (2.0, 2.0, 1.0, 0.0),                            # 3: counts 2.0 (pol 3 drops)
    (float(np.nextafter(2.0, 3.0)), 2.0, 1.0, 0.0),  # 4: just above 2 (pol 3 keeps)
    (3.0, 2.0, 1.0, 0.0),                            # 5
    (0.0, 2.0, 1.0, 0.5),                            # 6: counts 0 (pol 1 drops)
    (5e-324, 1.0, 1.0, 0.0),                         # 7: smallest denormal (pol 1 keeps)
    (4.0, 3.25, 2.5, -1.125),                        # 8: ordinary, kept
    (7.0, 50.0, 50.0, 49.99),                        # 9: ordinary, cond ~ 1e4, dropped
    (6.0, 1.5, 0.75, 0.25),                          # 10: ordinary, kept
]
MASK_KEEP = {   # expected keep flags of the rows, worked out by hand: {(pol, threshold index): bits}
    (1, 0): (1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1), (1, 1): (1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1),
    (2, 0): (1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1), (2, 1): (0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1),
    (3, 0): (1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1), (3, 1): (0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1),
}


def mask_arrays(npix):
    """the rows repeated to npix pixels (11 is coprime to 64: every row meets every lane)"""
    rows = np.asarray(MASK_ROWS)
    return [np.ascontiguousarray(np.resize(rows[:, k], npix)) for k in range(4)]


def compact(keep, use_last_keep=True):
    """cm2_pixel_compact: exclusive prefix sum of the keep flags, -1 where dropped; new_npix = rank of the last pixel
    plus its keep flag -> (old2new int32, new_npix)"""
    k = (np.asarray(keep) != 0).astype(np.int64)
    rank = np.cumsum(k) - k
    new_npix = int(rank[-1] + (k[-1] if use_last_keep else 0))
    return np.where(k == 1, rank, -1).astype(np.int32), new_npix


COMPACT_CASES = ("all", "none", "last-kept", "last-dropped", "one-kept", "one-dropped", "stride")


@functools.lru_cache(maxsize=None)
def keep_pattern(name):
    rng = np.random.default_rng(21)
    if name == "all":
        k = np.ones(130)
    elif name == "none":
        k = np.zeros(130)
    elif name in ("last-kept", "last-dropped"):
        k = (rng.uniform(size=130) < 0.6)
        k[-1] = name == "last-kept"
        k[0] = name != "last-kept"
    elif name == "one-kept":
        k = np.ones(1)
    elif name == "one-dropped":
        k = np.zeros(1)
    else:
        k = (rng.uniform(size=524293) < 0.6)
        k[-1] = True
    k = np.ascontiguousarray(k, dtype=np.uint8)
    k.setflags(write=False)
    return k


def compact_apply(old2new, data, fill):
    """k_compact: out[old2new[i]] = in[i] for the kept pixels, every other position keeps `fill`"""
    out = np.full(old2new.size, fill, dtype=data.dtype)
    kept = old2new >= 0
    out[old2new[kept]] = data[kept]
    return out


def flag(pix, old2new):
    """k_flag: -1 stays -1, every other id is mapped"""
    if pix.size == 0:
        return pix.copy()
    return np.where(pix == -1, -1, old2new[np.where(pix < 0, 0, pix)]).astype(np.int32)


# --------------------------------------------------------------------- block operators ----
DET_MIN = 1e-5
DET_UP = float(np.nextafter(1e-5, 1.0))


@functools.lru_cache(maxsize=None)
def blocks(npix):
    """per-pixel sums for the block operators.  Pixels 0..3: counts 1, cosine = sine = sincos = 0, sin2 = 1 and
    cos2 = 1e-5, nextafter(1e-5, 1), -1e-5, -nextafter(1e-5, 1): det = cos2 exactly for pol 2 and 3.  Pixel 4 and
    every 9th pixel: all sums 0 (never observed).  The rest: random."""
    rng = np.random.default_rng(31 + npix)
    b = SimpleNamespace(npix=npix, new_npix=npix)
    b.counts = rng.integers(1, 6, npix).astype(np.float64)
    b.cosine, b.sine = rng.standard_normal(npix), rng.standard_normal(npix)
    b.cos2, b.sin2 = rng.uniform(0.5, 3.0, npix), rng.uniform(0.5, 3.0, npix)
    b.sincos = rng.standard_normal(npix)
    zero = np.arange(npix) % 9 == 4
    for a in (b.counts, b.cosine, b.sine, b.cos2, b.sin2, b.sincos):
        a[zero] = 0.0
    b.counts[:4], b.cosine[:4], b.sine[:4], b.sincos[:4], b.sin2[:4] = 1.0, 0.0, 0.0, 0.0, 1.0
    b.cos2[:4] = (DET_MIN, DET_UP, -DET_MIN, -DET_UP)
    b.x = rng.standard_normal(3 * npix)
    return b


def bd_det_mask(pol, b):
    """k_bd_det_mask -> (det, mask uint8); pol 1: det = counts"""
    if pol == 1:
        return b.counts.copy(), (b.counts > 0.0).astype(np.uint8)
    if pol == 3:
        d = b.counts * (b.cos2 * b.sin2 - b.sincos * b.sincos) - b.cosine * b.cosine * b.sin2 \
            - b.sine * b.sine * b.cos2 + 2. * b.cosine * b.sine * b.sincos
    else:
        d = (b.cos2 * b.sin2) - (b.sincos * b.sincos)
    return d, (np.abs(d) > 1e-5).astype(np.uint8)


def bd_precond(pol, b, det, mask, x):
    """bd_inverse_block: the closed-form solve where mask, 0.0 elsewhere"""
    m = mask != 0
    h, c, s, c2, s2, cs = b.counts, b.cosine, b.sine, b.cos2, b.sin2, b.sincos
    xs = [x[k:pol * b.npix:pol] for k in range(pol)]
    with np.errstate(all="ignore"):
        if pol == 1:
            ys = [xs[0] / h]
        elif pol == 2:
            ys = [(s2 * xs[0] - cs * xs[1]) / det, (-cs * xs[0] + c2 * xs[1]) / det]
        else:
            ys = [((c2 * s2 - cs * cs) * xs[0] + (s * cs - c * s2) * xs[1] + (c * cs - s * c2) * xs[2]) / det,
                  ((s * cs - c * s2) * xs[0] + (h * s2 - s * s) * xs[1] + (s * c - h * cs) * xs[2]) / det,
                  ((c * cs - s * c2) * xs[0] + (-h * cs + c * s) * xs[1] + (h * c2 - c * c) * xs[2]) / det]
    y = np.empty(pol * b.npix)
    for k in range(pol):
        y[k::pol] = np.where(m, ys[k], 0.0)
    return y


def bd_apply(pol, b, x):
    h, c, s, c2, s2, cs = b.counts, b.cosine, b.sine, b.cos2, b.sin2, b.sincos
    xs = [x[k:pol * b.npix:pol] for k in range(pol)]
    if pol == 1:
        ys = [xs[0] * h]
    elif pol == 2:
        ys = [c2 * xs[0] + cs * xs[1], cs * xs[0] + s2 * xs[1]]
    else:
        ys = [h * xs[0] + c * xs[1] + s * xs[2], c * xs[0] + c2 * xs[1] + cs * xs[2],
              s * xs[0] + cs * xs[1] + s2 * xs[2]]
    y = np.empty(pol * b.npix)
    for k in range(pol):
        y[k::pol] = ys[k]
    return y


# ------------------------------------------------------------------- cut sky <-> full sky ----
SKIES = {"small": (16, 130), "stride": (256, 524293)}          # name -> (nside, observed pixels)


@functools.lru_cache(maxsize=None)
def sky(name):
    """a strict subset of the 12 nside^2 pixels that holds pixel 0 and the last one, in increasing order"""
    nside, npix = SKIES[name]
    nfull = 12 * nside * nside
    rng = np.random.default_rng(41 + npix)
    inner = np.sort(rng.choice(np.arange(1, nfull - 1), npix - 2, replace=False))
    obspix = np.concatenate([[0], inner, [nfull - 1]]).astype(np.int64)
    return SimpleNamespace(nside=nside, nfull=nfull, npix=npix, obspix=obspix, map=rng.standard_normal(3 * npix))


def cut_to_full(pol, obspix, m, nfull):
    full = np.zeros(pol * nfull)
    for k in range(pol):
        full[k * nfull + obspix] = m[k:pol * obspix.size:pol]
    return full


def full_to_cut(pol, obspix, full, nfull):
    m = np.empty(pol * obspix.size)
    for k in range(pol):
        m[k::pol] = full[k * nfull + obspix]
    return m
