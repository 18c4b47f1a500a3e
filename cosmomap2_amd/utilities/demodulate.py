"""
Lock-in demodulation and decimation of the time streams on the GPU: the last stage at the detector sample rate for an
instrument with a rotating half-wave plate.  The stream and its products with the polarisation carrier ``cos 2 phi,
sin 2 phi`` (``expand_pointing(..., hwp=chi)`` writes it to HBM) are low-passed by a FIR filter and one sample in
``factor`` is kept: three slow streams ``T, Q, U`` that each map with a plain ``pol=1`` pointing, and every kernel
downstream works on ``1/factor`` of the samples.  Without a carrier the same kernel decimates (the reference has no
counterpart).

    dm = Demodulator(blocksize, factor=8)                          # blocksize as BlockLO takes it; taps = lowpass_taps(8)
    T, Q, U, cls, info = dm.demodulate(d, carrier=(cos2, sin2), flags=pixs)
    T, cls, info       = dm.decimate(d, flags=pixs)
    pix_slow           = dm.pick(pixs, cls, drop_from=1)           # the pixel of every output's centre, -1 where dropped
    P = SparseLO(npix, len(pix_slow), pix_slow, pol=1)             # one such map each for T, Q and U
    blocks_slow        = dm.out_blocksize(len(d))                  # the noise blocks of the slow streams
    T, Q, U, cls, info = demodulate(d, blocksize, factor, carrier=(cos2, sin2))    # the same in one call

**Definition** (include/cosmomap2.h, f2h, has it in full).  Everything is cut at the block boundaries.  A sample is
*usable* when it is not flagged and finite.  Block ``b`` of ``n_b`` samples gives ``ceil(n_b / factor)`` outputs,
output ``j`` centred on sample ``j factor`` of the block.  With the taps ``h_0 .. h_{L-1}`` (``L`` odd, ``c = (L-1)/2``)
the sums ``sT += h_k d_i``, ``sQ += h_k (d_i cos_i)``, ``sU += h_k (d_i sin_i)`` and ``W += h_k`` run over
``k = 0 .. L-1`` in ascending order, ``i = j factor - c + k``, over the terms whose sample lies in the block and is
usable.  ``T = sT / W``, ``Q = 2 (sQ / W)``, ``U = 2 (sU / W)`` when ``W >= min_weight Wfull`` (``Wfull`` the sum of
all taps), 0 otherwise.  Classes: ``full`` (all ``L`` terms), ``partial`` (fewer, the weight test passed),
``rejected``.  A truncated window no longer averages the carrier over whole periods, so ``partial`` outputs carry far
larger errors than ``W / Wfull`` suggests: map with ``drop_from=1``.  Fill the gaps first (``fill_gaps_linear`` or
``GapFiller``): a normalised sum across a gap leaks intensity into ``Q`` and ``U``.

Arrays or tensors are taken as :func:`flag_glitches` takes them.  Every result has the bits the definition gives.
Every argument is checked before the GPU is touched (``ValueError``); without a GPU a valid call raises ``HipError``.
On several GPUs each rank handles its own blocks: blocks are independent.
"""
import ctypes
import math

import numpy as np

from .. import _hip
from .. import device as D
from ._stream_args import _BlockStage, _StageHandle, _check_classes, _int, _tod_length

__all__ = ["Demodulator", "demodulate", "decimate", "lowpass_taps", "DEMOD_CLASSES"]

DEMOD_CLASSES = ("full", "partial", "rejected")
FULL, PARTIAL, REJECTED = range(3)
MAX_FACTOR = 64                # CM2_DEMOD_MAX_FACTOR
MAX_TAPS = 1025                # CM2_DEMOD_MAX_TAPS


def _check_factor(factor):
    factor = _int("factor", factor)
    if not 1 <= factor <= MAX_FACTOR:
        raise ValueError("factor=%d outside [1, %d]" % (factor, MAX_FACTOR))
    return factor


def _check_ntaps(ntaps):
    ntaps = _int("ntaps", ntaps)
    if not 1 <= ntaps <= MAX_TAPS or ntaps % 2 == 0:
        raise ValueError("ntaps=%d must be odd and in [1, %d]" % (ntaps, MAX_TAPS))
    return ntaps


def tap_sum(taps):
    """``Wfull``: the taps added from 0.0 in ascending order, as the kernel's ``W`` adds them."""
    w = 0.0
    for h in taps:
        w = w + float(h)
    return w


def _check_taps(taps):
    if D.is_tensor(taps):
        taps = D.to_host(taps)
    try:
        h = np.ascontiguousarray(taps, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("taps must be real numbers, got %r" % (type(taps),))
    if h.ndim != 1:
        raise ValueError("taps must be one-dimensional, got shape %s" % (h.shape,))
    _check_ntaps(int(h.size))
    if not np.isfinite(h).all():
        raise ValueError("every tap must be finite")
    w = tap_sum(h)
    if not (np.isfinite(w) and w > 0):
        raise ValueError("the sum of the taps must be finite and > 0, got %r" % w)
    return h.copy(), w


def _check_min_weight(min_weight):
    try:
        v = float(min_weight)
    except (TypeError, ValueError):
        raise ValueError("min_weight must be a number in (0, 1], got %r" % (min_weight,))
    if not 0.0 < v <= 1.0:                                     # (a NaN fails this)
        raise ValueError("min_weight must be a number in (0, 1], got %r" % (min_weight,))
    return v


def _check_drop_from(drop_from):
    drop_from = _int("drop_from", drop_from)
    if drop_from not in (PARTIAL, REJECTED):
        raise ValueError("drop_from=%d is neither 1 (keep full outputs only) nor 2 (keep full and partial ones)"
                         % drop_from)
    return drop_from


def lowpass_taps(factor, ntaps=None, cutoff=None):
    """
    The taps of the default low-pass for decimation by ``factor``: a sinc of cut-off ``cutoff`` cycles per sample
    (default ``0.4 / factor``, below the slow streams' Nyquist frequency ``0.5 / factor``) under a Hamming window,
    ``ntaps`` of them (odd, default ``16 factor + 1``), symmetrised and divided by their ``math.fsum``.  Host NumPy.
    """
    factor = _check_factor(factor)
    ntaps = 16 * factor + 1 if ntaps is None else _check_ntaps(ntaps)
    if cutoff is None:
        cutoff = 0.4 / factor
    else:
        try:
            cutoff = float(cutoff)
        except (TypeError, ValueError):
            raise ValueError("cutoff must be a number in (0, 0.5], got %r" % (cutoff,))
        if not 0.0 < cutoff <= 0.5:
            raise ValueError("cutoff must be in (0, 0.5] cycles per sample, got %r" % (cutoff,))
    c = (ntaps - 1) // 2
    k = np.arange(ntaps, dtype=np.float64) - c
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * k) * (0.54 + 0.46 * np.cos(np.pi * k / (c + 1)))
    h = 0.5 * (h + h[::-1])
    return h / math.fsum(h)


class _Demod(_StageHandle):
    """Owns a cm2_demod handle (the block tables of the input units and of the outputs, the taps on the device).
    cm2_demod_create takes the factor and the taps where the other stages take one window, so the constructor is its
    own; ``info()`` and the release are the base's."""
    prefix = "demod"
    info_names = ("nt", "nblocks", "factor", "ntaps", "M", "unit", "outputs_per_thread", "lds_bytes", "bytes")

    def __init__(self, nt, sizes, factor, taps):
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        tp = np.ascontiguousarray(taps, dtype=np.float64)
        h = ctypes.c_void_p()
        _hip.call("cm2_demod_create", ctypes.byref(h), int(nt), sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                  len(sizes), int(factor), tp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(tp.size),
                  D.stream())
        _hip.Handle.__init__(self, "cm2_demod_destroy", h)


class Demodulator(_BlockStage):
    """
    Low-passes and decimates by ``factor`` (``1 <= factor <= 64``) time streams cut into the noise blocks
    ``blocksize`` (BlockLO's convention: an int that divides the stream, or the list of block sizes), with or without
    the carrier of a half-wave plate.  ``taps``: the FIR filter, an odd number (at most 1025) of finite numbers with
    a positive sum; default :func:`lowpass_taps` of the factor.  ``min_weight`` in ``(0, 1]``: the share of the taps'
    sum an output needs from usable samples.  The object owns, per stream length it has met, the block tables and the
    taps on the device, and no buffer of the stream's size.
    """
    handle_class = _Demod
    noun, histograms = "demodulator", "the block tables"

    def __init__(self, blocksize, factor, taps=None, min_weight=0.5):
        self.factor = _check_factor(factor)
        self.taps, self.wfull = _check_taps(lowpass_taps(self.factor) if taps is None else taps)
        self.min_weight = _check_min_weight(min_weight)
        _BlockStage.__init__(self, blocksize)

    # ---- checks (no GPU) ----
    def out_blocksize(self, nt):
        """The noise blocks of the slow streams of a stream of ``nt`` samples: ``ceil(n_b / factor)`` per block."""
        return [-(-s // self.factor) for s in self._sizes(_int("nt", nt))]

    def _check_carrier(self, carrier, nt):
        try:
            cos2, sin2 = carrier
        except (TypeError, ValueError):
            raise ValueError("carrier must be the pair (cos 2 phi, sin 2 phi)")
        for name, x in (("cos", cos2), ("sin", sin2)):
            if _tod_length(x) != nt:
                raise ValueError("the carrier's %s has %d samples, the stream %d" % (name, _tod_length(x), nt))
            if D.is_tensor(x) and not x.is_cuda:
                raise ValueError("a tensor for the carrier's %s must be in HBM, got device %s" % (name, x.device))
        return cos2, sin2

    # ---- device ----
    def _handle(self, nt, sizes):
        if nt not in self._handles:
            self._handles[nt] = _Demod(nt, sizes, self.factor, self.taps)
        return self._handles[nt]

    def info(self, nt):
        """The library's description of the handle for streams of ``nt`` samples (outputs ``M``, input samples per
        workgroup, outputs per thread, LDS bytes, bytes owned)."""
        return _BlockStage.info(self, nt)

    def _run(self, d, carrier, flags):
        nt, sizes = self._check_stream(d, flags)
        cs = None if carrier is None else self._check_carrier(carrier, nt)
        D.require_gpu()
        tt = D.torch
        nb, out_sizes = len(sizes), self.out_blocksize(nt)
        M = sum(out_sizes)
        g = self._handle(nt, sizes)
        x = D.f64(d)
        f, kind = self._dev_flags(flags)
        co, si = (None, None) if cs is None else (D.f64(cs[0]), D.f64(cs[1]))
        T, cls, counts = D.empty(M), D.empty(M, tt.uint8), D.empty(3 * nb, tt.int64)
        Q, U = (None, None) if cs is None else (D.empty(M), D.empty(M))
        _hip.call("cm2_demod_run", g.h, D.ptr(x), D.ptr(co), D.ptr(si), D.ptr(f), kind, self.min_weight, D.ptr(T),
                  D.ptr(Q), D.ptr(U), D.ptr(cls), D.ptr(counts), D.stream())
        info = dict(counts=D.to_host(counts).reshape(nb, 3).copy(), M=M, out_blocksize=out_sizes, Wfull=self.wfull,
                    taps=self.taps.copy())
        return T, Q, U, cls, info

    def decimate(self, d, flags=None):
        """``(T, classes, info)``: the low-passed stream, one sample in ``factor`` (float64, in HBM), the class byte
        of every output (uint8, in HBM; ``DEMOD_CLASSES``) and ``info``: ``counts`` ([nblocks, 3] int64: full,
        partial, rejected), ``M``, ``out_blocksize``, ``Wfull`` and the ``taps`` used."""
        T, _, _, cls, info = self._run(d, None, flags)
        return T, cls, info

    def demodulate(self, d, carrier, flags=None):
        """``(T, Q, U, classes, info)`` with ``carrier = (cos 2 phi, sin 2 phi)``, arrays or tensors of the stream's
        length (used only at usable samples); the rest as :meth:`decimate`."""
        if carrier is None:
            raise ValueError("carrier must be the pair (cos 2 phi, sin 2 phi); decimate() takes none")
        return self._run(d, carrier, flags)

    def pick(self, pixs, classes, drop_from=2):
        """The int32 pixel of every output's centre sample, ``-1`` where the output's class is at or above
        ``drop_from`` (1: keep ``full`` only; 2: keep ``full`` and ``partial``) or the centre's pixel is negative.
        ``pixs``: the pixels of the fast stream (signed integers, or an int32 tensor); ``classes``: what
        :meth:`decimate` or :meth:`demodulate` returned.  A tensor in HBM for ``pixs`` in HBM, else of its kind."""
        if D.is_tensor(pixs):
            if pixs.dtype != D.torch.int32 or pixs.dim() != 1:
                raise ValueError("a pixs tensor must be one-dimensional int32, got %s %s" % (pixs.dtype,
                                                                                            tuple(pixs.shape)))
            nt = int(pixs.numel())
        else:
            a = np.asarray(pixs)
            if a.ndim != 1 or not np.issubdtype(a.dtype, np.signedinteger):
                raise ValueError("pixs must be a one-dimensional array of signed integers, got %s %s"
                                 % (a.dtype, a.shape))
            if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
                raise ValueError("pixs does not fit int32")
            nt = int(a.size)
        if nt < 1:
            raise ValueError("pixs has no samples")
        sizes = self._sizes(nt)
        M = sum(self.out_blocksize(nt))
        _check_classes("classes", classes, M)
        drop_from = _check_drop_from(drop_from)
        D.require_gpu()
        p, c, out = D.i32(pixs), D.to_dev(classes), D.empty(M, D.torch.int32)      # held until the call is enqueued
        _hip.call("cm2_demod_pick", self._handle(nt, sizes).h, D.ptr(p), D.ptr(c), drop_from, D.ptr(out), D.stream())
        return D.like_input(out, pixs)


def decimate(d, blocksize, factor, taps=None, min_weight=0.5, flags=None):
    """``Demodulator(blocksize, factor, taps, min_weight).decimate(d, flags)`` for a single stream."""
    return Demodulator(blocksize, factor, taps, min_weight).decimate(d, flags=flags)


def demodulate(d, blocksize, factor, carrier, taps=None, min_weight=0.5, flags=None):
    """``Demodulator(blocksize, factor, taps, min_weight).demodulate(d, carrier, flags)`` for a single stream."""
    return Demodulator(blocksize, factor, taps, min_weight).demodulate(d, carrier, flags=flags)
