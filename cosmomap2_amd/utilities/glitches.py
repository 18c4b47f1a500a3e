"""
Glitch flags from the time streams, on the GPU: cosmic-ray hits, readout jumps of a few samples and non-finite
samples, found per noise block with a running median and the median absolute deviation (the reference reads its
flags from the data files, utilities/IOfiles.py:142-152, and has no de-glitcher).

    gf = GlitchFlagger(blocksize, half_width=16)               # blocksize as BlockLO takes it
    cls, info = gf.flag(d, flags=pixs, nsigma=5.0, grow=2)     # one class byte per sample, in HBM
    apply_flags(pixs, cls)                                     # pixs[cls != 0] = -1
    r     = gf.residual(d, flags=pixs)                         # the median-detrended stream
    sigma = gf.scale(d, r, flags=pixs)                         # robust sigma per block
    cls, info = flag_glitches(d, blocksize, flags=pixs)        # the same in one call

**Definition** (include/cosmomap2.h, f2e, has it in full).  Everything is cut at the block boundaries.  A sample is
*usable* when it is not flagged, finite, and not ``hit`` / ``near`` in the pass before.  ``med_i`` is the median of
the usable samples within ``half_width`` of a usable ``i`` (the mean of the two middle ones when their number is
even), ``r_i = d_i - med_i`` (0 where unusable).  ``sigma_b = 1.4826 x`` the lower median of ``|r|`` over the usable
samples of block ``b``; a block with fewer usable samples than one window is *short*, has ``sigma = inf`` and gets
no hits.  A usable sample with ``|r_i| > nsigma sigma_b`` is a hit.  Classes, the first that applies:
``input`` (flagged on input), ``nonfinite``, ``hit`` / ``near`` carried from the pass before, ``hit``, ``near`` (a hit
of the same block within ``grow`` samples), ``clean``.

**Iteration.**  Glitches bias the medians and inflate the scale, so :meth:`GlitchFlagger.flag` repeats the pass with
the classes of the pass before, until a pass adds no hit or ``iterations`` passes have run.

**Flags** as :func:`fill_gaps_linear` takes them: ``flags[i] < 0`` for an integer array (the ``pix`` array), true
for a bool array; NumPy or tensor; ``None``: nothing flagged.  ``d`` is a float64 tensor in HBM or a NumPy array.
Every result is an order statistic or a count: the same bits on every run.  Every argument is checked before the GPU
is touched (``ValueError``); without a GPU a valid call raises ``HipError``.  On several GPUs each rank flags its own
blocks (``sharding.shard_blocks``): blocks are independent, so this is the same result.
"""
import numpy as np

from .. import _hip
from .. import device as D
from ._stream_args import MAX_ITERATIONS                     # noqa: F401  (a limit of flag(), public here)
from ._stream_args import _flags_to_dev                      # noqa: F401  (tests/test_gpu_glitch.py looks it up here)
from ._stream_args import (_MAX_NT, _BlockStage, _StageHandle, _check_classes, _check_iterations, _check_nsigma,
                           _check_sigma, _int, _tod_length)

__all__ = ["GlitchFlagger", "flag_glitches", "apply_flags", "GLITCH_CLASSES"]

GLITCH_CLASSES = ("clean", "input", "nonfinite", "hit", "near")
CLEAN, INPUT, NONFINITE, HIT, NEAR = range(5)
MAX_HALF_WIDTH = 64            # CM2_GLITCH_MAX_HALF_WIDTH
MAX_GROW = 64                  # CM2_GLITCH_MAX_GROW


def _check_half_width(h):
    h = _int("half_width", h)
    if not 1 <= h <= MAX_HALF_WIDTH:
        raise ValueError("half_width=%d outside [1, %d]" % (h, MAX_HALF_WIDTH))
    return h


def _check_grow(grow):
    grow = _int("grow", grow)
    if not 0 <= grow <= MAX_GROW:
        raise ValueError("grow=%d outside [0, %d]" % (grow, MAX_GROW))
    return grow


class _Glitch(_StageHandle):
    """Owns a cm2_glitch handle (block tables and the histograms of the selection)."""
    prefix, info_names = "glitch", ("nt", "nblocks", "half_width", "run", "tier", "bytes")


class GlitchFlagger(_BlockStage):
    """
    Flags the glitches of time streams cut into the noise blocks ``blocksize`` (BlockLO's convention: an int that
    divides the stream, or the list of block sizes) with windows of ``2 half_width + 1`` samples,
    ``1 <= half_width <= 64``.  The object owns the block tables and the selection's histograms of the stream
    lengths it has met (8 KB per block), and no buffer of the stream's size.
    """
    handle_class, window = _Glitch, "half_width"
    noun, histograms = "glitch flagger", "the selection's histograms"

    def __init__(self, blocksize, half_width=16):
        self.half_width = _check_half_width(half_width)
        _BlockStage.__init__(self, blocksize)

    def info(self, nt):
        """The library's description of the handle for streams of ``nt`` samples (tier, run length, bytes owned)."""
        return _BlockStage.info(self, nt)

    def _residual(self, g, x, f, kind, prev, out=None):
        r = out if out is not None else D.empty(x.numel())
        _hip.call("cm2_glitch_residual", g.h, D.ptr(x), D.ptr(f), kind, D.ptr(prev), D.ptr(r), D.stream())
        return r

    def _scale(self, g, x, r, f, kind, prev, nblocks):
        sigma = D.empty(nblocks)
        _hip.call("cm2_glitch_scale", g.h, D.ptr(x), D.ptr(r), D.ptr(f), kind, D.ptr(prev), D.ptr(sigma), D.stream())
        return sigma

    def residual(self, d, flags=None, prev=None):
        """``r``: ``d`` minus its running median where usable, 0 elsewhere; a float64 tensor in HBM."""
        nt, sizes = self._check_stream(d, flags, prev)
        D.require_gpu()
        f, kind = self._dev_flags(flags)
        p = None if prev is None else D.to_dev(prev)
        return self._residual(self._handle(nt, sizes), D.f64(d), f, kind, p)

    def scale(self, d, r, flags=None, prev=None):
        """``sigma`` per block (a float64 tensor in HBM) from the residual ``r`` of the same ``d``, flags and prev."""
        nt, sizes = self._check_stream(d, flags, prev)
        if _tod_length(r) != nt:
            raise ValueError("r has %d samples, d %d" % (_tod_length(r), nt))
        D.require_gpu()
        f, kind = self._dev_flags(flags)
        p = None if prev is None else D.to_dev(prev)
        return self._scale(self._handle(nt, sizes), D.f64(d), D.f64(r), f, kind, p, len(sizes))

    def flag(self, d, flags=None, nsigma=5.0, grow=2, iterations=3, sigma=None):
        """
        ``(cls, info)``: ``cls`` a uint8 tensor in HBM with the class of every sample (``GLITCH_CLASSES``), ``info``
        a dict with ``counts`` ([nblocks, 5] int64, samples per block and class), ``sigma`` ([nblocks], the last
        pass's), ``short_blocks`` (indices of the blocks with fewer usable samples than one window in the last pass),
        ``passes`` and ``hits_per_pass``.  ``sigma`` (one number, or one per block) replaces the robust scale, e.g.
        with a white level from ``estimate_offset_prior``.
        """
        nt, sizes = self._check_stream(d, flags)
        nsigma, grow, iterations = _check_nsigma(nsigma), _check_grow(grow), _check_iterations(iterations)
        given = _check_sigma(sigma, len(sizes))
        D.require_gpu()
        t = D.torch
        nb, W = len(sizes), 2 * self.half_width + 1
        g = self._handle(nt, sizes)
        x = D.f64(d)
        f, kind = self._dev_flags(flags)
        r = D.empty(nt)
        cls = [D.empty(nt, t.uint8), D.empty(nt, t.uint8)]         # prev and the new classes change places
        counts_dev = D.empty(nb * 5, t.int64)
        sig = D.to_dev(given) if given is not None else None
        prev, hits, before = None, [], np.zeros((nb, 5), dtype=np.int64)
        for k in range(iterations):
            self._residual(g, x, f, kind, prev, out=r)
            if given is None:
                sig = self._scale(g, x, r, f, kind, prev, nb)
            out = cls[k & 1]
            _hip.call("cm2_glitch_classify", g.h, D.ptr(x), D.ptr(r), D.ptr(f), kind, D.ptr(prev), D.ptr(sig),
                      nsigma, grow, D.ptr(out), D.ptr(counts_dev), D.stream())
            counts = D.to_host(counts_dev).reshape(nb, 5)
            # the usable samples of this pass: not input, not non-finite, not carried from the pass before
            usable = np.asarray(sizes) - counts[:, INPUT] - counts[:, NONFINITE] - before[:, HIT] - before[:, NEAR]
            hits.append(int(counts[:, HIT].sum() - before[:, HIT].sum()))
            prev, before = out, counts
            if hits[-1] == 0:
                break
        info = dict(counts=counts, sigma=D.to_host(sig), short_blocks=np.flatnonzero(usable < W),
                    passes=len(hits), hits_per_pass=hits)
        return prev, info


def flag_glitches(d, blocksize, flags=None, half_width=16, nsigma=5.0, grow=2, iterations=3, sigma=None):
    """``GlitchFlagger(blocksize, half_width).flag(d, ...)`` for a single stream."""
    return GlitchFlagger(blocksize, half_width).flag(d, flags=flags, nsigma=nsigma, grow=grow, iterations=iterations,
                                                     sigma=sigma)


def apply_flags(pixs, cls):
    """
    ``pixs[cls != 0] = -1``: every sample that is not ``clean`` leaves the map-making (``SparseLO`` and its
    neighbours skip ``pixs < 0``).  An int32 tensor in HBM is changed in place and returned; a NumPy array (or a
    host tensor) is left alone and a changed int32 copy of its kind is returned.
    """
    if D.is_tensor(pixs):
        if pixs.dtype != D.torch.int32 or pixs.dim() != 1:
            raise ValueError("a pixs tensor must be one-dimensional int32, got %s %s" % (pixs.dtype,
                                                                                        tuple(pixs.shape)))
        if pixs.is_cuda and not pixs.is_contiguous():
            raise ValueError("a pixs tensor in HBM must be contiguous to be changed in place")
        nt = int(pixs.numel())
    else:
        a = np.asarray(pixs)
        if a.ndim != 1 or not np.issubdtype(a.dtype, np.signedinteger):
            raise ValueError("pixs must be a one-dimensional array of signed integers, got %s %s" % (a.dtype, a.shape))
        if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
            raise ValueError("pixs does not fit int32")
        nt = int(a.size)
    if nt < 1:
        raise ValueError("pixs has no samples")
    if nt > _MAX_NT:
        raise ValueError("%d samples do not fit the 32-bit sample counts of the glitch flagger" % nt)
    _check_classes("cls", cls, nt)
    D.require_gpu()
    inplace = D.is_dev(pixs)
    p = pixs if inplace else D.i32(np.asarray(pixs) if not D.is_tensor(pixs) else pixs)
    _hip.call("cm2_glitch_apply_pix", nt, D.ptr(D.to_dev(cls)), D.ptr(p), D.stream())
    return p if inplace else D.like_input(p, pixs)
