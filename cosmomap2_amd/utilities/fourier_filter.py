"""
The Fourier filter of the time streams on the GPU: per noise block the transform is multiplied by a response
``H_b(f)`` and transformed back.  It undoes (or, for simulations, applies) the one-pole response
``1 / (1 + 2 pi i f tau)`` of a bolometer, the first thing a bolometer pipeline does to its data, and gives a sharp
Butterworth low-pass and high-pass, ``cos^2`` notches at the pulse-tube and mains lines and an arbitrary tabulated
response (a whitening filter ``1 / sqrt(PSD)`` for a filter-and-bin map ``P^T F P``), real or complex, shared or per
block.  The reference has no counterpart.

    ff = FourierFilter(blocksize, fsample, tau=taus, lowpass=(20.0, 4))       # blocksize as BlockLO takes it
    clean = ff.apply(d)                                    # a new stream; ff.apply(d, out=d) works in place
    H = ff.response(0)                                     # complex H_0 at the bins k fs / L of block 0
    clean = deconvolve_time_constant(d, blocksize, fsample, taus, lowpass=(20.0, 4))    # the same in one call
    y = fourier_filter(d, blocksize, fsample, highpass=(0.1, 2), notch=[(1.4, 0.02)], pad=4096)

**Definition** (include/cosmomap2.h, f2j, has it in full).  Everything is cut at the block boundaries.  Per block of
``n`` samples: with ``detrend="ends"`` the line through the means of the first and the last ``min(end_mean, n)`` samples
is subtracted; the block is padded with zeros to ``L = fft_length(n, pad)``, the smallest even 7-smooth integer
``>= max(2, n + pad)``; at bin ``k``, ``f = k fs / L`` and ``H = T G_lp G_hp prod G_notch R`` with ``T = 1 + i u``
(``mode="deconvolve"``) or ``(1 - i u) / (1 + u^2)`` (``"convolve"``), ``u = 2 pi f tau_b``;
``G_lp = 1 / sqrt(1 + (f / fc)^(2 order))``, ``G_hp = 1 / sqrt(1 + (fc / f)^(2 order))`` and 0 at ``f = 0``; a notch
``(f0, w)`` is ``sin^2(pi |f - f0| / (2 w))`` within ``w`` of ``f0`` and 1 elsewhere; ``R`` is interpolated linearly
from ``response`` on the grid ``r (fs / 2) / (Rn - 1)``.  The real inverse transform of ``H X`` is cut back to ``n``
samples and ``Re H(0)`` times the line is put back (the constant ``tau slope fs`` a deconvolved ramp would carry is
not restored).

The padding keeps the circular convolution from wrapping the end of a block onto its start: ``pad=1024`` is a
convention that suits time constants and low-passes; a high-pass at ``fc`` rings for about ``fs / fc`` samples and
wants ``pad >~ fs / fc``.  The stage takes no flags: fill the gaps first (``fill_gaps_linear`` or ``GapFiller``).  A
block with a non-finite sample comes out as NaN, every sample of it, and is counted in ``info``; no other block is
affected.

Arrays or tensors are taken as :func:`flag_glitches` takes them.  Every argument is checked before the GPU is touched
(``ValueError``); without a GPU a valid call raises ``HipError``.  On several GPUs each rank handles its own blocks:
blocks are independent.
"""
import ctypes

import numpy as np

from .. import _hip
from .. import device as D
from ._stream_args import _BlockStage, _check_fsample, _check_out, _int

__all__ = ["FourierFilter", "fourier_filter", "deconvolve_time_constant", "fft_length", "FOURIER_MODES"]

FOURIER_MODES = ("deconvolve", "convolve")       # CM2_FOURIER_DECONVOLVE, CM2_FOURIER_CONVOLVE
DETREND = ("none", "ends")
MAX_ORDER = 16                 # CM2_FOURIER_MAX_ORDER
MAX_NOTCH = 16                 # CM2_FOURIER_MAX_NOTCH
MAX_END_MEAN = 1024            # CM2_FOURIER_MAX_END_MEAN
MAX_LENGTHS = 8                # CM2_FOURIER_MAX_LENGTHS
MAX_LENGTH = 1 << 28
DEFAULT_WORK_BYTES = 512 << 20
_INFO = 5 + 3 * MAX_LENGTHS


def _smooth7(v):
    for p in (2, 3, 5, 7):
        while v % p == 0:
            v //= p
    return v == 1


def fft_length(n, pad=1024):
    """The transform length of a block of ``n`` samples: the smallest even integer ``>= max(2, n + pad)`` whose prime
    factors all lie in {2, 3, 5, 7} (fft_length of csrc/cm2_fourier_policy.h)."""
    n, pad = _int("n", n), _int("pad", pad)
    if n < 1 or pad < 0:
        raise ValueError("n=%d must be >= 1 and pad=%d >= 0" % (n, pad))
    L = max(2, n + pad)
    L += L & 1
    while L <= MAX_LENGTH:
        if _smooth7(L):
            return L
        L += 2
    raise ValueError("n=%d with pad=%d needs a transform longer than 2^28" % (n, pad))


def _number(name, v, what="a finite number >= 0"):
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be %s, got %r" % (name, what, v))
    if not (np.isfinite(x) and x >= 0):
        raise ValueError("%s must be %s, got %r" % (name, what, v))
    return x


def _check_cut(name, cut):
    """``None`` or ``(fc, order)`` -> (fc, order); fc = 0 means absent"""
    if cut is None:
        return 0.0, 1
    try:
        fc, order = cut
    except (TypeError, ValueError):
        raise ValueError("%s must be None or the pair (cut-off frequency, order), got %r" % (name, cut))
    fc = _number("the cut-off of %s" % name, fc, "a finite number > 0")
    if fc <= 0:
        raise ValueError("the cut-off of %s must be a finite number > 0, got %r" % (name, cut[0]))
    order = _int("the order of %s" % name, order)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError("the order of %s is %d, outside [1, %d]" % (name, order, MAX_ORDER))
    return fc, order


def _check_notch(notch):
    try:
        pairs = [tuple(pr) for pr in notch]
    except TypeError:
        raise ValueError("notch must be a sequence of (f0, width) pairs, got %r" % (notch,))
    if len(pairs) > MAX_NOTCH:
        raise ValueError("%d notches are more than %d" % (len(pairs), MAX_NOTCH))
    out = np.zeros((len(pairs), 2))
    for j, pr in enumerate(pairs):
        if len(pr) != 2:
            raise ValueError("notch[%d] must be the pair (f0, width), got %r" % (j, pr))
        out[j, 0] = _number("the frequency of notch[%d]" % j, pr[0])
        out[j, 1] = _number("the width of notch[%d]" % j, pr[1], "a finite number > 0")
        if out[j, 1] <= 0:
            raise ValueError("the width of notch[%d] must be a finite number > 0, got %r" % (j, pr[1]))
    return out


def _check_response(response):
    """None, or the table as (float64 array [rows, Rn(, 2)] flattened later, kind, per_block, Rn)"""
    if response is None:
        return None, 0, 0, 0
    if D.is_tensor(response):
        response = D.to_host(response)
    try:
        a = np.asarray(response)
        if not (np.issubdtype(a.dtype, np.number) or a.dtype == np.bool_):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("response must be an array of real or complex numbers, got %r" % (type(response),))
    if a.ndim not in (1, 2) or a.shape[-1] < 2:
        raise ValueError("response must have the shape [Rn] or [nblocks, Rn] with Rn >= 2, got %s" % (a.shape,))
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        kind = 2
    else:
        a = np.ascontiguousarray(a, dtype=np.float64)
        kind = 1
    if not np.isfinite(a).all():
        raise ValueError("every value of response must be finite")
    return a, kind, int(a.ndim == 2), int(a.shape[-1])


class _Fourier(_hip.Handle):
    """Owns a cm2_fourier handle: the plans per transform length, the work rows, tau, the notches and the table."""

    def __init__(self, nt, sizes, ff, tau):
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        dp = ctypes.POINTER(ctypes.c_double)
        tp = None if tau is None else tau.ctypes.data_as(dp)
        notch = np.ascontiguousarray(ff.notch.reshape(-1))
        table = None if ff._table is None else np.ascontiguousarray(ff._table).view(np.float64).reshape(-1)
        h = ctypes.c_void_p()
        _hip.call("cm2_fourier_create", ctypes.byref(h), int(nt), sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                  len(sizes), ff.fsample, tp, FOURIER_MODES.index(ff.mode), ff.lowpass[0], ff.lowpass[1],
                  ff.highpass[0], ff.highpass[1], notch.ctypes.data_as(dp) if notch.size else None,
                  int(ff.notch.shape[0]), None if table is None else table.ctypes.data_as(dp), ff._Rn, ff._table_kind,
                  ff._per_block, DETREND.index(ff.detrend), ff.end_mean, ff.pad, int(ff.conjugate),
                  ff.max_work_bytes, D.stream())
        _hip.Handle.__init__(self, "cm2_fourier_destroy", h)

    def info(self):
        raw = (ctypes.c_int64 * _INFO)()
        _hip.call("cm2_fourier_info", self.h, raw, D.stream())
        v = [int(x) for x in raw]
        ng = v[2]
        return dict(nt=v[0], nblocks=v[1], work_bytes=v[3], bad_blocks=v[4], lengths=v[5:5 + ng],
                    batches=v[5 + MAX_LENGTHS:5 + MAX_LENGTHS + ng],
                    blocks=v[5 + 2 * MAX_LENGTHS:5 + 2 * MAX_LENGTHS + ng])


class FourierFilter(_BlockStage):
    """
    ``FourierFilter(blocksize, fsample, tau=None, mode="deconvolve", lowpass=None, highpass=None, notch=(),
    response=None, detrend="ends", end_mean=32, pad=1024, max_work_bytes=None)``

    ``blocksize``: the noise blocks (BlockLO's convention: an int that divides the stream, or the list of block
    sizes).  ``tau``: ``None`` (no time constant), one number for every block or one per block, in seconds, ``>= 0``.
    ``mode``: ``"deconvolve"`` multiplies by ``1 + 2 pi i f tau``, ``"convolve"`` by its inverse.  ``lowpass``,
    ``highpass``: ``(fc, order)`` of a Butterworth magnitude response, ``fc > 0`` in the unit of ``fsample``,
    ``1 <= order <= 16``.  ``notch``: up to 16 pairs ``(f0, width)``.  ``response``: a table ``[Rn]`` or
    ``[nblocks, Rn]``, real or complex, on the grid ``r (fsample / 2) / (Rn - 1)``.  ``detrend``: ``"ends"`` or
    ``"none"``; ``end_mean``: the samples averaged at either end, in ``[1, 1024]``.  ``pad``: zeros appended before the
    transform length is rounded up (a high-pass at ``fc`` wants ``pad >~ fsample / fc``).  ``max_work_bytes``: the
    cap on the work rows and the plan of one transform length (default 512 MB).  ``conjugate=True`` gives the filter
    with ``conj(H)``: the transpose of the linear filter (``detrend="none"``).

    Fill the gaps before filtering (``fill_gaps_linear``, ``GapFiller``): the stage takes no flags.  The object
    owns, per stream length it has met, the plans and work rows of its transform lengths (at most 8 distinct ones).
    """
    noun, histograms = "Fourier filter", "the block tables"

    def __init__(self, blocksize, fsample, tau=None, mode="deconvolve", lowpass=None, highpass=None, notch=(),
                 response=None, detrend="ends", end_mean=32, pad=1024, max_work_bytes=None, conjugate=False):
        self.fsample = _check_fsample(fsample)
        if mode not in FOURIER_MODES:
            raise ValueError("mode must be 'deconvolve' or 'convolve', got %r" % (mode,))
        self.mode = mode
        if tau is None:
            self.tau = None
        else:
            if D.is_tensor(tau):
                tau = D.to_host(tau)
            try:
                t = np.array(tau, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("tau must be None, a number or one number per block, got %r" % (type(tau),))
            if t.ndim > 1 or (t.ndim == 1 and t.size < 1):
                raise ValueError("tau must be None, a number or one number per block, got shape %s" % (t.shape,))
            if not (np.isfinite(t).all() and (t >= 0).all()):
                raise ValueError("every time constant must be finite and >= 0")
            self.tau = t
        self.lowpass = _check_cut("lowpass", lowpass)
        self.highpass = _check_cut("highpass", highpass)
        self.notch = _check_notch(notch)
        self._table, self._table_kind, self._per_block, self._Rn = _check_response(response)
        if detrend not in DETREND:
            raise ValueError("detrend must be 'ends' or 'none', got %r" % (detrend,))
        self.detrend = detrend
        self.end_mean = _int("end_mean", end_mean)
        if not 1 <= self.end_mean <= MAX_END_MEAN:
            raise ValueError("end_mean=%d outside [1, %d]" % (self.end_mean, MAX_END_MEAN))
        self.pad = _int("pad", pad)
        if not 0 <= self.pad <= MAX_LENGTH:
            raise ValueError("pad=%d outside [0, 2^28]" % self.pad)
        self.max_work_bytes = DEFAULT_WORK_BYTES if max_work_bytes is None else _int("max_work_bytes", max_work_bytes)
        if self.max_work_bytes < 1:
            raise ValueError("max_work_bytes=%d < 1" % self.max_work_bytes)
        if not isinstance(conjugate, (bool, np.bool_)):
            raise ValueError("conjugate must be True or False, got %r" % (conjugate,))
        self.conjugate = bool(conjugate)
        _BlockStage.__init__(self, blocksize)
        if np.ndim(self.blocksize) != 0:
            self._check_per_block(len(self.blocksize))

    # ---- checks (no GPU) ----
    @property
    def real_response(self):
        """Whether ``H`` is real at every bin: no time constant and no complex table."""
        return (self.tau is None or not self.tau.any()) and self._table_kind != 2

    def _check_per_block(self, nblocks):
        if self.tau is not None and self.tau.ndim == 1 and self.tau.size != nblocks:
            raise ValueError("tau has %d values, the stream %d blocks" % (self.tau.size, nblocks))
        if self._per_block and self._table.shape[0] != nblocks:
            raise ValueError("response has %d rows, the stream %d blocks" % (self._table.shape[0], nblocks))

    def _sizes(self, nt):
        sizes = _BlockStage._sizes(self, nt)
        self._check_per_block(len(sizes))
        lengths = {}
        for n in sizes:
            if n not in lengths:
                lengths[n] = fft_length(n, self.pad)
        if len(set(lengths.values())) > MAX_LENGTHS:
            raise ValueError("the blocks need %d distinct transform lengths, more than %d"
                             % (len(set(lengths.values())), MAX_LENGTHS))
        return sizes

    def _block(self, nt, block):
        sizes = self._sizes(_int("nt", nt))
        block = _int("block", block)
        if not 0 <= block < len(sizes):
            raise ValueError("block=%d outside [0, %d)" % (block, len(sizes)))
        return sizes, block

    def fft_length(self, block, nt=None):
        """The transform length of block ``block`` (of a stream of ``nt`` samples, which a list of block sizes
        already says)."""
        sizes, block = self._block(self._nt(nt), block)
        return fft_length(sizes[block], self.pad)

    def _nt(self, nt):
        if nt is not None:
            return nt
        if np.ndim(self.blocksize) != 0:
            return sum(self.blocksize)
        if len(self._handles) == 1:
            return next(iter(self._handles))
        raise ValueError("nt is needed: blocksize=%d does not say how long the stream is" % self.blocksize)

    # ---- device ----
    def _handle(self, nt, sizes):
        if nt not in self._handles:
            tau = None
            if self.tau is not None:
                tau = np.ascontiguousarray(np.broadcast_to(self.tau, (len(sizes),)), dtype=np.float64)
            self._handles[nt] = _Fourier(nt, sizes, self, tau)
        return self._handles[nt]

    def apply(self, d, out=None):
        """The filtered stream: float64, in HBM for a tensor in HBM, else a NumPy array.  ``out``: where to write it
        (``out is d`` filters in place; any other overlap is refused)."""
        nt, sizes = self._check_stream(d)
        _check_out(out, nt)
        D.require_gpu()
        g = self._handle(nt, sizes)
        x = D.f64(d)
        dst = out if (out is not None and D.is_tensor(out)) else D.empty(nt)
        _hip.call("cm2_fourier_apply", g.h, D.ptr(x), D.ptr(dst), D.stream())
        if out is None:
            return D.like_input(dst, d)
        if not D.is_tensor(out):
            out[:] = D.to_host(dst)
        return out

    def response(self, block, nt=None):
        """``H`` of block ``block`` at the bins ``k fsample / L``, ``k = 0 .. L/2`` with ``L = fft_length(block)``, as
        the filter kernel evaluates it: a complex NumPy array."""
        sizes, block = self._block(self._nt(nt), block)
        D.require_gpu()
        nt = sum(sizes)
        L = fft_length(sizes[block], self.pad)
        H = D.empty(2 * (L // 2 + 1))
        _hip.call("cm2_fourier_response", self._handle(nt, sizes).h, block, D.ptr(H), D.stream())
        return D.to_host(H).view(np.complex128).copy()

    def info(self, nt=None):
        """The library's description of the handle for streams of ``nt`` samples: the transform ``lengths``, the rows
        of a batch (``batches``) and the ``blocks`` of each, ``work_bytes``, and the ``bad_blocks`` of the last
        :meth:`apply`."""
        nt = _int("nt", self._nt(nt))
        sizes = self._sizes(nt)
        D.require_gpu()
        return self._handle(nt, sizes).info()


def fourier_filter(d, blocksize, fsample, **kw):
    """``FourierFilter(blocksize, fsample, **kw).apply(d)`` for a single stream."""
    return FourierFilter(blocksize, fsample, **kw).apply(d)


def deconvolve_time_constant(d, blocksize, fsample, tau, lowpass=None):
    """The stream with the one-pole response of time constant ``tau`` (one number, or one per block) divided out,
    and a Butterworth low-pass ``(fc, order)`` against the noise that ``1 + 2 pi i f tau`` lifts."""
    if tau is None:
        raise ValueError("tau must be a number or one number per block")
    return FourierFilter(blocksize, fsample, tau=tau, mode="deconvolve", lowpass=lowpass).apply(d)
