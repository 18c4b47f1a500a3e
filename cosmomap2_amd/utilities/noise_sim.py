"""
Noise time streams drawn from a PSD on the GPU: the way back from :mod:`noise_model`'s time stream ->
PSD -> band (the reference has no simulator; its tests draw noise with NumPy on the host).

    w   = white_noise(n, seed)                              # Philox4x64-10, float64 tensor in HBM
    g   = noise_filter_bands(psd, lam)                      # [nb, lam] colouring bands
    sim = NoiseSimulator(blocksize, psd, lam, seed=7)       # owns the operator and its buffers
    sim.draw(0)                                             # realisation 0, a float64 tensor of nt samples
    sim.draw(1, out=d, add=True)                            # d += realisation 1, nothing allocated
    simulate_noise(blocksize, psd, lam, seed=7)             # the one-shot form

**White noise.**  The stream of (seed, realization, block) is Philox4x64-10 with key ``[seed, realization]``
and counter ``[j + 1, block, 0, 0]`` for output block j: ``numpy.random.Philox(key=[seed, realization],
counter=[0, block, 0, 0])``, bit for bit, and ``kind='uniform'`` is ``numpy.random.Generator(...).random()``.
``kind='normal'`` is Box-Muller over the pairs ``(u0, u1)``, ``(u2, u3)`` of a counter block:
``r = sqrt(-2 log(1 - u_a))``, ``z_a = r cos(2 pi u_b)``, ``z_b = r sin(2 pi u_b)``.  Sample i depends on
(seed, realization, block, i) alone, not on the call that asks for it.

**Coloured noise.**  Block b of a draw (global index ``first_block + b``, ``n_b`` samples) is the valid part
of the convolution of ``n_b + 2 (lam - 1)`` normals of the stream (seed, realization, first_block + b) with
the symmetric filter ``g_|j|``, ``|j| < lam``: every sample has the autocovariance ``g * g``, up to the block
edges.  Blocks are independent streams, so a rank that holds blocks ``[k0, k1)`` of
``sharding.shard_blocks`` passes its own block sizes and PSDs with ``first_block = k0`` and gets the samples
the single-GPU call gives for those blocks; no collective is needed.

Every argument is checked before the GPU is touched (``ValueError``); without a GPU a valid call raises
``HipError`` like every operator constructor.
"""
import ctypes

import numpy as np

from .. import _hip
from .. import device as D
from ._stream_args import _block_sizes, _check_fsample, _check_lam, _check_psd, _int, _u64
from .noise_model import _bands_from_psd

__all__ = ["white_noise", "noise_filter_bands", "NoiseSimulator", "simulate_noise"]

_KINDS = {"uniform": 0, "normal": 1}


def _check_kind(kind):
    if not isinstance(kind, str) or kind not in _KINDS:
        raise ValueError("kind must be 'normal' or 'uniform', got %r" % (kind,))
    return _KINDS[kind]


def white_noise(n, seed, realization=0, block=0, first=0, kind="normal"):
    """
    Samples ``first .. first + n - 1`` of the white stream (seed, realization, block) as a float64
    tensor in HBM: standard normals (``kind='normal'``) or uniforms in [0, 1) (``kind='uniform'``,
    bit-equal to ``numpy.random.Generator(numpy.random.Philox(key=[seed, realization],
    counter=[0, block, 0, 0])).random(first + n)[first:]``).  ``seed``, ``realization`` and ``block`` are
    integers in [0, 2^64); any cut of a stream into calls gives the same samples.
    """
    n = _int("n", n)
    if n < 0:
        raise ValueError("n=%d is negative" % n)
    seed, realization, block = _u64("seed", seed), _u64("realization", realization), _u64("block", block)
    first = _int("first", first)
    if first < 0 or first + n >= 1 << 62:
        raise ValueError("first=%d must be in [0, 2^62 - n)" % first)
    k = _check_kind(kind)
    D.require_gpu()
    out = D.empty(n)
    _hip.call("cm2_rng_fill", k, seed, realization, block, first, n, D.ptr(out), D.stream())
    return out


def noise_filter_bands(psd, lam, fsample=1.0):
    """
    Colouring bands ``[nb, lam]`` from a one-sided PSD ``[nb, L/2+1]``, with the conventions of
    :func:`inverse_noise_bands`:

        S_k = P_k fs / m_k  (m_k = 1 at k = 0 and L/2, else 2),  S_0 := S_1,
        h_j = numpy.fft.irfft(sqrt(S), L)[j],   g_j = (1 - j/lam) h_j,   1 <= lam <= L/2.

    White noise filtered with ``g_|j|`` has the spectrum ``|g^|^2``, where the symbol ``g^(w) = g_0 +
    2 sum_j g_j cos(w j)`` is sqrt(S) smoothed by the Fejer kernel (>= 0): the simulated spectrum is S up
    to that resolution, not S itself -- the same limit the estimated inverse-noise band has.  ``P = 0`` is
    allowed; a negative or non-finite bin raises ``ValueError`` naming the block and the bin.
    """
    return _bands_from_psd("cm2_noise_filter_from_psd", psd, lam, fsample)


def _sim_sizes(blocksize):
    """Per-block sizes of a simulator: an int (one block) or a list of block sizes."""
    if np.ndim(blocksize) == 0:
        bs = _int("blocksize", blocksize)
        if bs <= 0:
            raise ValueError("blocksize=%d is not positive" % bs)
        return [bs]
    sizes = [_int("blocksize[%d]" % i, b) for i, b in enumerate(blocksize)]
    if not sizes or any(s <= 0 for s in sizes):
        raise ValueError("blocksize must list positive block sizes, got %r" % (list(blocksize),))
    return sizes


def _check_sim_args(blocksize, psd, lam, fsample, seed, first_block, nt):
    """(sizes, rows of the PSD, L, lam, fs, seed, first_block) of a simulator, without touching the GPU."""
    if nt is not None:
        nt = _int("nt", nt)
        if nt <= 0:
            raise ValueError("nt=%d is not positive" % nt)
        sizes = _block_sizes(blocksize, nt)
    else:
        sizes = _sim_sizes(blocksize)
    nb_psd, L = _check_psd(psd)
    if nb_psd not in (1, len(sizes)):
        raise ValueError("the PSD has %d rows for %d blocks (1 or one per block)" % (nb_psd, len(sizes)))
    lam = _check_lam(lam, L)
    fs = _check_fsample(fsample)
    seed, first_block = _u64("seed", seed), _u64("first_block", first_block)
    if first_block + len(sizes) > 1 << 64:
        raise ValueError("first_block=%d plus %d blocks passes 2^64" % (first_block, len(sizes)))
    return sizes, nb_psd, L, lam, fs, seed, first_block


def _check_draw_args(nt, realization, out, add, scale):
    """(realization, add, scale) of a draw of ``nt`` samples, without touching the GPU."""
    realization = _u64("realization", realization)
    if not isinstance(add, (bool, np.bool_)):
        raise ValueError("add must be True or False, got %r" % (add,))
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        raise ValueError("scale must be a finite number, got %r" % (scale,))
    if not np.isfinite(scale):
        raise ValueError("scale must be a finite number, got %r" % (scale,))
    if out is None:
        if add:
            raise ValueError("add=True needs an out to add to")
    elif D.is_tensor(out):
        if not out.is_cuda or out.dtype != D.torch.float64:
            raise ValueError("an out tensor must be float64 in HBM, got %s on %s" % (out.dtype, out.device))
        if out.dim() != 1 or out.numel() != nt or not out.is_contiguous():
            raise ValueError("out must be a contiguous vector of %d samples, got shape %s" % (nt, tuple(out.shape)))
    elif isinstance(out, np.ndarray):
        if out.dtype != np.float64:
            raise ValueError("an out array must be float64, got %s" % out.dtype)
        if out.ndim != 1 or out.size != nt or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("out must be a writeable contiguous vector of %d samples, got shape %s" % (nt, out.shape))
    else:
        raise ValueError("out must be a float64 tensor in HBM or a NumPy array, got %r" % type(out))
    return realization, bool(add), scale


class NoiseSimulator(_hip.Handle):
    """
    Coloured noise for the blocks ``blocksize`` with the one-sided PSD ``psd``: ``[1, L/2+1]`` (shared by
    all blocks) or ``[nb, L/2+1]``, filtered with :func:`noise_filter_bands` of length ``lam``.

    ``blocksize`` is a list of block sizes, or an int together with ``nt`` (equal blocks; ``nt`` must be a
    multiple of it); an int alone is one block.  ``first_block`` is the global index of the first block
    (a rank's ``k0`` of ``sharding.shard_blocks``).  The object owns the Toeplitz operator on the padded
    blocks (direct sum up to lam = 32, the fused overlap-save kernel up to 2049, rocFFT beyond) and two
    buffers of ``nt + 2 nb (lam - 1)`` doubles; :meth:`draw` allocates nothing of TOD size.
    """

    def __init__(self, blocksize, psd, lam, fsample=1.0, seed=0, first_block=0, nt=None):
        sizes, nb_psd, L, lam, fs, self.seed, self.first_block = _check_sim_args(blocksize, psd, lam, fsample, seed,
                                                                                 first_block, nt)
        self.sizes, self.nt, self.lam = sizes, sum(sizes), lam
        D.require_gpu()
        g = np.ascontiguousarray(D.to_host(noise_filter_bands(psd, lam, fs)), dtype=np.float64)
        if nb_psd == 1 and len(sizes) > 1:
            g = np.ascontiguousarray(np.broadcast_to(g, (len(sizes), lam)))
        self.bands = g
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        h = ctypes.c_void_p()
        _hip.call("cm2_noise_sim_create", ctypes.byref(h), g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), lam,
                  sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(sizes), self.seed, self.first_block,
                  D.stream())
        _hip.Handle.__init__(self, "cm2_noise_sim_destroy", h)
        self._host_out = None          # device buffer behind a NumPy `out`, made on first use

    def info(self):
        info = (ctypes.c_int64 * 7)()
        _hip.call("cm2_noise_sim_info", self.h, info)
        keys = ("nt", "nblocks", "lam", "padded_samples", "method", "fft_length", "buffer_bytes")
        return dict(zip(keys, [int(v) for v in info]))

    def draw(self, realization, out=None, add=False, scale=1.0):
        """
        Realisation ``realization`` (an integer in [0, 2^64)) of the ``nt`` samples, times ``scale``.
        ``out=None`` returns a new float64 tensor in HBM; a given ``out`` (a float64 tensor in HBM or a
        NumPy array of ``nt`` samples) is overwritten, or added to with ``add=True``, and returned.  The
        same (seed, realization) always gives the same bits.
        """
        realization, add, scale = _check_draw_args(self.nt, realization, out, add, scale)
        D.require_gpu()
        if out is None:
            out = D.empty(self.nt)
        if D.is_tensor(out):
            _hip.call("cm2_noise_sim_draw", self.h, realization, scale, int(add), D.ptr(out), D.stream())
            return out
        if self._host_out is None:
            self._host_out = D.empty(self.nt)
        _hip.call("cm2_noise_sim_draw", self.h, realization, scale, 0, D.ptr(self._host_out), D.stream())
        y = D.to_host(self._host_out)
        if add:
            out += y
        else:
            out[:] = y
        return out


def simulate_noise(blocksize, psd, lam, seed, realization=0, fsample=1.0, first_block=0, nt=None, out=None,
                   add=False, scale=1.0):
    """One draw of ``NoiseSimulator(blocksize, psd, lam, fsample, seed, first_block, nt)``: realisation
    ``realization``, as :meth:`NoiseSimulator.draw` returns it.  For many realisations keep the simulator."""
    sizes = _check_sim_args(blocksize, psd, lam, fsample, seed, first_block, nt)[0]
    _check_draw_args(sum(sizes), realization, out, add, scale)
    sim = NoiseSimulator(blocksize, psd, lam, fsample=fsample, seed=seed, first_block=first_block, nt=nt)
    return sim.draw(realization, out=out, add=add, scale=scale)
