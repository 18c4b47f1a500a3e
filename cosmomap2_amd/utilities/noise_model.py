"""
Inverse-noise bands estimated from the time streams (the reference has no estimator: its
``BlockLO`` / ``ToeplitzLO``, interfaces/linearoperators.py:560-697, only define what a band is,
``y_k = a0 v_k + sum_{i>=1} a_i (v_{k+i} + v_{k-i})``).

    f, psd = noise_psd(d, blocksize, nperseg)          # Welch PSD per noise block, on the GPU
    bands  = inverse_noise_bands(psd, lam)             # [nb, lam] SPD bands
    N      = estimate_inverse_noise(d, blocksize, lam) # BlockLO(blocksize, bands, offdiag=True)

``blocksize`` follows ``BlockLO``: an int (equal blocks; ``len(d)`` must be a multiple of it) or a
list of per-block sizes adding up to ``len(d)``.  ``d`` may be a NumPy array or a float64 tensor in
HBM; for a tensor nothing of TOD size crosses PCIe and the outputs are device tensors, otherwise
they are NumPy arrays.  Every argument is checked before the GPU is touched (``ValueError``);
without a GPU a valid call raises ``HipError`` like every operator constructor.

Estimate from the noise alone: on a bright sky, take a residual such as ``d - P (M_BD P^T d)``
(the binned sky map scanned back) rather than ``d`` itself, or the sky's power ends up in the
noise model.  On several GPUs, each rank estimates the whole blocks ``sharding.shard_blocks`` gave
it, from its own part of the TOD: blocks are independent, no collective is needed.
"""
import ctypes

import numpy as np

from .. import _hip
from .. import device as D
from ._stream_args import (_MIN_L, _block_sizes, _call_refusing_bins, _check_detrend, _check_fits_blocks,
                           _check_fsample, _check_lam, _check_nperseg, _check_psd, _int, _tod_length)

__all__ = ["noise_psd", "inverse_noise_bands", "estimate_inverse_noise"]


class _Psd(_hip.Handle):
    """Owns a cm2_psd handle (plan and workspace of one nperseg)."""

    def __init__(self, L, detrend, work_bytes):
        h = ctypes.c_void_p()
        _hip.call("cm2_psd_create", ctypes.byref(h), int(L), int(detrend), int(work_bytes or 0), D.stream())
        _hip.Handle.__init__(self, "cm2_psd_destroy", h)

    def info(self):
        info = (ctypes.c_int64 * 3)()
        _hip.call("cm2_psd_info", self.h, info)
        return dict(nperseg=int(info[0]), segments_per_batch=int(info[1]), work_bytes=int(info[2]))


def noise_psd(d, blocksize, nperseg, fsample=1.0, detrend="constant", work_bytes=None):
    """
    Welch PSD of every noise block of the TOD ``d``: ``(f, psd)`` with ``f = numpy.fft.rfftfreq(L, 1/fs)``
    and ``psd[b]`` equal to ``scipy.signal.welch(d_b, fs, window='hann', nperseg=L, noverlap=L//2,
    detrend=detrend, scaling='density', average='mean')[1]`` of block ``b`` (to rounding).

    ``nperseg`` (L) is a power of two in [256, 65536], no longer than the shortest block; block b
    has ``(n_b - L) // (L/2) + 1`` segments and a tail that does not fill one is ignored.  ``detrend``
    is ``'constant'`` (subtract each segment's mean) or ``False``.  The work runs over batches of
    segments whose buffers take at most ``work_bytes`` (default 512 MB) of device memory; the
    result of a block does not depend on the other blocks nor on the batch boundaries (summed in
    segment order).  Estimate from a residual such as ``d - P (M_BD P^T d)`` when the sky is bright.
    """
    nt = _tod_length(d)
    sizes = _block_sizes(blocksize, nt)
    L = _check_nperseg(nperseg)
    _check_fits_blocks(L, sizes)
    fs = _check_fsample(fsample)
    dt = _check_detrend(detrend)
    if work_bytes is not None and _int("work_bytes", work_bytes) <= 0:
        raise ValueError("work_bytes must be positive, got %r" % (work_bytes,))
    D.require_gpu()
    x = D.f64(d)
    nb = len(sizes)
    psd = D.empty(nb * (L // 2 + 1))
    h = _Psd(L, dt, work_bytes)
    sz = np.ascontiguousarray(sizes, dtype=np.int64)
    _hip.call("cm2_psd_welch", h.h, D.ptr(x), sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), nb, fs,
              D.ptr(psd), D.stream())
    del h
    f = np.fft.rfftfreq(L, 1.0 / fs)
    psd = psd.view(nb, L // 2 + 1)
    if D.is_dev(d):
        return D.f64(f), psd
    return f, D.to_host(psd)


def _bands_from_psd(entry, psd, lam, fsample):
    """The bands ``[nb, lam]`` that the library's ``entry`` builds from the PSD, on the side where the PSD is."""
    nb, L = _check_psd(psd)
    lam = _check_lam(lam, L)
    fs = _check_fsample(fsample)
    D.require_gpu()
    p = D.f64(psd)
    bands = D.empty(nb * lam)
    _call_refusing_bins(entry, D.ptr(p), nb, L, fs, lam, D.ptr(bands), D.stream())
    bands = bands.view(nb, lam)
    return bands if D.is_dev(psd) else D.to_host(bands)


def inverse_noise_bands(psd, lam, fsample=1.0):
    """
    First rows ``[nb, lam]`` of SPD banded-Toeplitz inverse-noise blocks from a one-sided PSD
    ``[nb, L/2+1]`` (from :func:`noise_psd`, or a model evaluated at ``numpy.fft.rfftfreq(L, 1/fs)``):

        S_k = P_k fs / m_k  (m_k = 1 at k = 0 and L/2, else 2),  S_0 := S_1 (the DC bin is not used)
        G_k = 1 / S_k,   c_j = numpy.fft.irfft(G, L)[j],   a_j = (1 - j/lam) c_j,   1 <= lam <= L/2.

    The Bartlett taper makes the band's symbol G smoothed by the Fejer kernel, which is >= 0: every
    block built from ``a`` is SPD, with no positivity lift.  White noise of variance s^2 gives
    ``a ~ (1/s^2, 0, ...)``; ``lam = 1`` gives one white-noise weight per block.  ``S`` must be
    positive, finite and not so small that ``1/S`` overflows: any other bin raises ``ValueError``
    naming the block and the bin.
    """
    return _bands_from_psd("cm2_noise_bands_from_psd", psd, lam, fsample)


def estimate_inverse_noise(d, blocksize, lam, nperseg=None, fsample=1.0, detrend="constant", work_bytes=None):
    """
    ``BlockLO(blocksize, bands, offdiag=True)`` with the bands estimated from the TOD ``d``:
    :func:`noise_psd` with ``nperseg`` (default ``max(256, 4 * next_pow2(lam))``), then
    :func:`inverse_noise_bands`.  Estimate from a residual such as ``d - P (M_BD P^T d)`` when the sky
    is bright; on several GPUs each rank passes its own blocks (``sharding.shard_blocks``).
    """
    lam = _int("lam", lam)
    if lam < 1:
        raise ValueError("lam=%d < 1" % lam)
    if nperseg is None:
        nperseg = max(_MIN_L, 4 * (1 << (lam - 1).bit_length()))
    L = _check_nperseg(nperseg)
    _check_lam(lam, L)
    nt = _tod_length(d)
    sizes = _block_sizes(blocksize, nt)
    _check_fits_blocks(L, sizes)
    _check_fsample(fsample)
    _check_detrend(detrend)
    _, psd = noise_psd(d, blocksize, L, fsample, detrend, work_bytes)
    bands = D.to_host(inverse_noise_bands(psd, lam, fsample))
    from ..interfaces.linearoperators import BlockLO
    return BlockLO(blocksize, [b for b in bands], offdiag=True)
