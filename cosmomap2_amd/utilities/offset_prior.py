"""
The destriper's noise model estimated from the time streams: one white weight per noise block and the banded
prior ``C_a^-1`` on the baseline offsets (``interfaces/destriper.py`` takes both, ``weights=`` and ``prior=``).

    bands, sigma2 = offset_prior_bands(psd, baseline_length, lam)        # [nb, lam] SPD bands, [nb] white variances
    w, prior, info = estimate_offset_prior(r, blocksize, baseline_length)
    m, a, cg_info, op = solve_destriped(P, blocksize, baseline_length, d, Mbd, weights=w, prior=prior)

Per block, from one row ``P_k`` (``k = 0 .. n/2``, ``n = nperseg``) of the one-sided PSD of :func:`noise_psd`, with
the baseline length ``L`` (``cm2_offset_prior_from_psd`` in ``include/cosmomap2.h`` has the same definition):

    S_k = P_k fs / m_k  (m_k = 1 at k = 0 and n/2, else 2),  S_0 := S_1
    sigma^2 = (4/n) sum_{k = n/4}^{n/2 - 1} S_k              the white level, unless the caller gives one
    R_k = max(S_k - sigma^2, 0)                               the correlated part
    q_j = (1/n) sum_k m_k R_k D_k cos(w_k L j),  j < K = floor((n/2 + 1) / L),  w_k = 2 pi k / n,
          D_k = sin^2(L w_k / 2) / (L^2 sin^2(w_k / 2))       the covariance of two baseline means j apart
    Q_i = q~_0 + 2 sum_{j >= 1} q~_j cos(2 pi i j / M),  q~_j = (1 - j/K) q_j,  i <= M/2,  M = next_pow2(2K)
    H_i = 1 / max(Q_i, floor sigma^2 / L)
    band_i = (1 - i/lam) (1/M) sum_{k <= M/2} m'_k H_k cos(2 pi i k / M),  i < lam <= M/2.

The two Bartlett tapers keep ``Q >= 0`` and every block of the prior SPD; ``sigma^2 / L`` is the white variance of a
baseline mean, so the floor bounds the prior by ``wsum / floor``.  The weight of block ``b`` is ``1 / sigma_b^2``.

The model is stationary in units of whole baselines: the short last baseline of a block is treated like a full one,
and so is a baseline with flagged samples.

``psd`` and the TOD may be NumPy arrays or float64 tensors in HBM.  Every argument is checked before the GPU is
touched (``ValueError``); without a GPU a valid call raises ``HipError``.  Estimate from the noise alone: pass a
residual such as ``d - P (M_BD P^T d)``, as for :func:`estimate_inverse_noise`.
"""
import ctypes

import numpy as np

from .. import device as D
from ._stream_args import (_MAX_L, _MIN_L, _block_sizes, _call_refusing_bins, _check_detrend, _check_fits_blocks,
                           _check_fsample, _check_nperseg, _check_psd, _int, _tod_length)
from .noise_model import noise_psd

__all__ = ["offset_prior_bands", "estimate_offset_prior"]

_DBLP = ctypes.POINTER(ctypes.c_double)


def _next_pow2(v):
    return 1 << (int(v) - 1).bit_length()


def _check_baseline(baseline_length):
    Lb = _int("baseline_length", baseline_length)
    if Lb < 1:
        raise ValueError("baseline_length=%d < 1" % Lb)
    return Lb


def _lags(n, Lb):
    """(K, M): the baseline lags that nperseg = n holds, and the length of the offsets' spectrum."""
    K = (n // 2 + 1) // Lb
    if K < 2:
        need = _next_pow2(4 * Lb - 2)
        if need > _MAX_L:
            raise ValueError("baseline_length=%d is too long for any nperseg up to %d (two baseline lags need "
                             "nperseg/2 + 1 >= 2 baseline_length)" % (Lb, _MAX_L))
        raise ValueError("nperseg=%d holds %d lag(s) of baselines of %d samples, two are needed: the smallest "
                         "nperseg that would do is %d" % (n, K, Lb, need))
    return K, _next_pow2(2 * K)


def _check_band_length(lam, K, M):
    lam = _int("lam", lam)
    if not 1 <= lam <= M // 2:
        raise ValueError("lam=%d outside [1, M/2 = %d] (K = %d baseline lags, M = %d)" % (lam, M // 2, K, M))
    return lam


def _check_floor(floor):
    try:
        f = float(floor)
    except (TypeError, ValueError):
        raise ValueError("floor must be a number in (0, 1], got %r" % (floor,))
    if not 0.0 < f <= 1.0:
        raise ValueError("floor must be a number in (0, 1], got %r" % (floor,))
    return f


def _check_sigma2(sigma2, nb):
    if sigma2 is None:
        return None
    try:
        s = np.array(D.to_host(sigma2) if D.is_tensor(sigma2) else sigma2, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("sigma2 must be one positive number per block, got %r" % (sigma2,))
    if s.ndim == 0:
        s = np.full(nb, float(s))
    if s.ndim != 1 or s.size != nb:
        raise ValueError("sigma2 must hold one value per block (%d), got shape %r" % (nb, s.shape))
    if not np.all(np.isfinite(s) & (s > 0)):
        raise ValueError("sigma2 must be positive and finite, got %r" % (s.tolist(),))
    return np.ascontiguousarray(s)


def _check_host_bins(psd, fs):
    """A PSD on the host is looked through here, so that a bad bin is refused before the GPU is touched as well (one
    in HBM is reported by the library, with the same words)."""
    if D.is_tensor(psd):
        return
    try:
        p = np.asarray(psd, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("the PSD must hold real numbers")
    m = np.full(p.shape[1], 2.0)
    m[-1] = 1.0
    with np.errstate(all="ignore"):
        S = p * fs / m
    S[:, 0] = S[:, 1]
    bad = np.flatnonzero(~(np.isfinite(S) & (S > 0)).ravel())
    if bad.size:
        b, k = divmod(int(bad[0]), p.shape[1])
        k = max(k, 1)
        raise ValueError("PSD of block %d is not positive and finite at bin %d (value %g): no offset prior can be "
                         "built from it" % (b, k, p[b, k]))


def offset_prior_bands(psd, baseline_length, lam, fsample=1.0, sigma2=None, floor=1e-6):
    """
    ``(bands, sigma2)``: the first rows ``[nb, lam]`` of the SPD banded-Toeplitz prior blocks on the baseline offsets,
    and the white variance ``[nb]`` of every block, from a one-sided PSD ``[nb, nperseg/2 + 1]`` (the module's
    docstring has the definition).  ``sigma2`` None estimates the white level from the upper half of the band; a
    number or one per block fixes it.  ``floor`` in (0, 1] bounds the prior by ``wsum / floor``; ``1 <= lam <= M/2``.
    Both results are device tensors for a device ``psd`` and NumPy arrays otherwise.  A bin with ``S <= 0`` or not
    finite raises ``ValueError`` naming the block and the bin.

    The short last baseline of a block is treated like a full one, and so is a baseline with flagged samples.
    """
    nb, n = _check_psd(psd)
    Lb = _check_baseline(baseline_length)
    K, M = _lags(n, Lb)
    lam = _check_band_length(lam, K, M)
    fs = _check_fsample(fsample)
    fl = _check_floor(floor)
    s_in = _check_sigma2(sigma2, nb)
    _check_host_bins(psd, fs)
    D.require_gpu()
    p = D.f64(psd)
    bands = D.empty(nb * lam)
    s_out = np.empty(nb, dtype=np.float64)
    _call_refusing_bins("cm2_offset_prior_from_psd", D.ptr(p), nb, n, fs, Lb, lam,
                        None if s_in is None else s_in.ctypes.data_as(_DBLP), fl, D.ptr(bands),
                        s_out.ctypes.data_as(_DBLP), D.stream())
    bands = bands.view(nb, lam)
    if D.is_dev(psd):
        return bands, D.f64(s_out)
    return D.to_host(bands), s_out


def estimate_offset_prior(r, blocksize, baseline_length, lam=None, nperseg=None, fsample=1.0, detrend="constant",
                          floor=1e-6):
    """
    ``(weights, prior, info)`` for :func:`solve_destriped` from the noise time stream ``r`` (a residual such as
    ``d - P (M_BD P^T d)``): :func:`noise_psd` with ``nperseg`` (default: the largest allowed power of two no longer
    than the shortest block), then :func:`offset_prior_bands`.  ``weights`` is the array ``1 / sigma_b^2``, ``prior``
    the ``BlockLO(baselines per block, bands, offdiag=True)`` on the ``sum_b ceil(n_b / baseline_length)`` offsets,
    ``info`` a dict with ``sigma2`` (array), ``K``, ``M``, ``lam`` and ``nperseg``.  ``lam`` defaults to the smaller
    of ``M/2`` and the smallest number of baselines in a block; a longer band than that number is refused.

    The short last baseline of a block is treated like a full one, and so is a baseline with flagged samples.
    """
    nt = _tod_length(r)
    sizes = _block_sizes(blocksize, nt)
    Lb = _check_baseline(baseline_length)
    if nperseg is None:
        if min(sizes) < _MIN_L:
            raise ValueError("the shortest block (%d samples) is shorter than the smallest nperseg, %d"
                             % (min(sizes), _MIN_L))
        nperseg = min(_MAX_L, 1 << (min(sizes).bit_length() - 1))
    n = _check_nperseg(nperseg)
    _check_fits_blocks(n, sizes)
    K, M = _lags(n, Lb)
    per_block = [-(-s // Lb) for s in sizes]
    if lam is None:
        lam = min(M // 2, min(per_block))
    lam = _check_band_length(lam, K, M)
    if lam > min(per_block):                   # (M/2 <= 2K - 1 < n/L + 1: cannot bind while nperseg fits the block)
        raise ValueError("lam=%d is longer than the %d baselines of the shortest block" % (lam, min(per_block)))
    fs = _check_fsample(fsample)
    _check_detrend(detrend)
    fl = _check_floor(floor)
    _, psd = noise_psd(r, blocksize, n, fs, detrend)
    bands, sigma2 = offset_prior_bands(psd, Lb, lam, fs, None, fl)
    bands, sigma2 = D.to_host(bands), D.to_host(sigma2)
    from ..interfaces.linearoperators import BlockLO
    prior = BlockLO(per_block, [b for b in bands], offdiag=True)
    return 1.0 / sigma2, prior, dict(sigma2=sigma2, K=K, M=M, lam=lam, nperseg=n)
