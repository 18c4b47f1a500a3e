"""
What the time-stream stages (noise model, noise simulation, offset prior, gap fill, glitch flags, jump correction and
the operators built on them) agree on before the GPU is touched: the checks of the arguments they share, each written
once with its message, and the skeleton of a stage that works block by block on streams of any length
(:class:`_BlockStage`, with the handle :class:`_StageHandle` it keeps per stream length).  Every check raises
``ValueError``; none touches the GPU.
"""
import ctypes

import numpy as np

from .. import _hip
from .. import device as D

_MIN_L, _MAX_L = 256, 65536
_MAX_NT = (1 << 32) - 2        # the 32-bit sample index of cm2_gaps, cm2_glitch and cm2_jump
_MAX_BLOCKS = 1 << 18          # kMaxBlocks of cm2_stream_policy.h
MAX_ITERATIONS = 8


def _is_pow2(n):
    return n > 0 and (n & (n - 1)) == 0


def _int(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, got %r" % (name, v))
    return int(v)


def _u64(name, v):
    v = _int(name, v)
    if not 0 <= v < 1 << 64:
        raise ValueError("%s=%d outside [0, 2^64)" % (name, v))
    return v


def _check_fsample(fsample):
    try:
        fs = float(fsample)
    except (TypeError, ValueError):
        raise ValueError("fsample must be a positive number, got %r" % (fsample,))
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("fsample must be a positive number, got %r" % (fsample,))
    return fs


def _check_nperseg(nperseg):
    L = _int("nperseg", nperseg)
    if not (_is_pow2(L) and _MIN_L <= L <= _MAX_L):
        raise ValueError("nperseg=%d must be a power of two in [%d, %d]" % (L, _MIN_L, _MAX_L))
    return L


def _check_fits_blocks(L, sizes):
    if L > min(sizes):
        raise ValueError("nperseg=%d is longer than the shortest block (%d samples)" % (L, min(sizes)))


def _call_refusing_bins(name, *args):
    """``_hip.call`` after the arguments were checked: an argument error is a bad bin, refused in the library's words"""
    try:
        _hip.call(name, *args)
    except _hip.HipError as e:
        if e.status == _hip.ERR_ARGUMENT:
            raise ValueError(str(e)) from None
        raise


def _check_lam(lam, L):
    lam = _int("lam", lam)
    if not 1 <= lam <= L // 2:
        raise ValueError("lam=%d outside [1, nperseg/2 = %d]" % (lam, L // 2))
    return lam


def _check_rtol(rtol):
    try:
        rtol = float(rtol)
    except (TypeError, ValueError):
        raise ValueError("rtol must be a positive number, got %r" % (rtol,))
    if not (np.isfinite(rtol) and rtol > 0):
        raise ValueError("rtol must be a positive number, got %r" % (rtol,))
    return rtol


def _tod_length(d):
    """Number of samples of a 1-D TOD (NumPy array or float64 tensor), without touching the GPU."""
    if D.is_tensor(d):
        if D.torch is None or d.dtype != D.torch.float64:
            raise ValueError("a TOD tensor must be float64, got %s" % d.dtype)
        if d.dim() != 1:
            raise ValueError("the TOD must be one-dimensional, got shape %s" % (tuple(d.shape),))
        return int(d.numel())
    a = np.asarray(d)
    if a.ndim != 1:
        raise ValueError("the TOD must be one-dimensional, got shape %s" % (a.shape,))
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError("the TOD must be real numbers, got dtype %s" % a.dtype)
    return int(a.size)


def _block_sizes(blocksize, nt):
    """Per-block sizes of ``blocksize`` (BlockLO's convention) for a TOD of ``nt`` samples."""
    if np.ndim(blocksize) == 0:
        bs = _int("blocksize", blocksize)
        if bs <= 0 or nt % bs:
            raise ValueError("blocksize=%d does not divide the %d samples of the TOD" % (bs, nt))
        return [bs] * (nt // bs)
    sizes = [_int("blocksize[%d]" % i, b) for i, b in enumerate(blocksize)]
    if not sizes or any(s <= 0 for s in sizes):
        raise ValueError("blocksize must list positive block sizes, got %r" % (list(blocksize),))
    if sum(sizes) != nt:
        raise ValueError("blocksize adds up to %d samples, the TOD has %d" % (sum(sizes), nt))
    return sizes


def _check_detrend(detrend):
    if detrend is False:
        return 0
    if isinstance(detrend, str) and detrend == "constant":
        return 1
    raise ValueError("detrend must be 'constant' or False, got %r" % (detrend,))


def _check_psd(psd):
    """(nb, L) of a PSD array [nb, L/2+1] (NumPy array or float64 tensor)."""
    if D.is_tensor(psd):
        if psd.dtype != D.torch.float64:
            raise ValueError("a PSD tensor must be float64, got %s" % psd.dtype)
        shape = tuple(psd.shape)
    else:
        shape = np.shape(psd)
    if len(shape) != 2 or shape[0] < 1:
        raise ValueError("the PSD must be an array [nblocks, nperseg/2 + 1], got shape %s" % (shape,))
    L = 2 * (shape[1] - 1)
    if not (_is_pow2(L) and _MIN_L <= L <= _MAX_L):
        raise ValueError("the PSD has %d bins per block: not nperseg/2 + 1 for a power of two nperseg in "
                         "[%d, %d]" % (shape[1], _MIN_L, _MAX_L))
    return shape[0], L


def _check_flags(flags, nt=None):
    """Length of a 1-D flag array (integer or bool, NumPy or tensor), without touching the GPU."""
    if D.is_tensor(flags):
        t = D.torch
        if flags.dtype not in (t.int32, t.bool, t.uint8):
            raise ValueError("a flags tensor must be int32 (flagged where negative) or bool, got %s" % flags.dtype)
        shape = tuple(flags.shape)
    else:
        a = np.asarray(flags)
        if not (a.dtype == np.bool_ or np.issubdtype(a.dtype, np.signedinteger)):
            raise ValueError("flags must be signed integers (flagged where negative) or bool, got dtype %s" % a.dtype)
        shape = a.shape
    if len(shape) != 1 or shape[0] < 1:
        raise ValueError("flags must be a one-dimensional array with at least one sample, got shape %s" % (shape,))
    n = int(shape[0])
    if n > _MAX_NT:
        raise ValueError("%d samples do not fit the 32-bit sample index of the gap table" % n)
    if nt is not None and n != nt:
        raise ValueError("%d flags for %d samples" % (n, nt))
    return n


def _flags_to_dev(flags):
    """(contiguous device tensor, kind) with kind 0 = int32 pixel ids, 1 = bytes."""
    t = D.torch
    if D.is_tensor(flags):
        if flags.dtype == t.int32:
            return D.to_dev(flags), 0
        return D.to_dev(flags).view(t.uint8), 1
    a = np.asarray(flags)
    if a.dtype == np.int32:
        return D.to_dev(a), 0
    if a.dtype != np.bool_:
        a = a < 0
    return D.to_dev(np.ascontiguousarray(a).view(np.uint8)), 1


def _check_tod(name, d, nt):
    if _tod_length(d) != nt:
        raise ValueError("%s has %d samples, the flags %d" % (name, _tod_length(d), nt))
    if D.is_tensor(d) and not d.is_cuda:
        raise ValueError("a %s tensor must be in HBM, got device %s" % (name, d.device))


def _check_out(out, nt):
    """``out`` as NoiseSimulator.draw takes it: None, a float64 tensor in HBM or a NumPy array of nt samples."""
    if out is None:
        return
    if D.is_tensor(out):
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


def _check_nsigma(nsigma):
    try:
        v = float(nsigma)
    except (TypeError, ValueError):
        raise ValueError("nsigma must be a positive finite number, got %r" % (nsigma,))
    if not (np.isfinite(v) and v > 0):
        raise ValueError("nsigma must be a positive finite number, got %r" % (nsigma,))
    return v


def _check_iterations(iterations):
    iterations = _int("iterations", iterations)
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError("iterations=%d outside [1, %d]" % (iterations, MAX_ITERATIONS))
    return iterations


def _check_sigma(sigma, nblocks):
    """None, or the caller's sigma per block as a float64 array (>= 0 or +inf)."""
    if sigma is None:
        return None
    if D.is_tensor(sigma):
        sigma = D.to_host(sigma)
    s = np.asarray(sigma, dtype=np.float64)
    if s.ndim == 0:
        s = np.full(nblocks, float(s))
    if s.shape != (nblocks,):
        raise ValueError("sigma must be one number or one per block (%d), got shape %s" % (nblocks, s.shape))
    if not (s >= 0).all():                                   # NaN and negative values fail this
        raise ValueError("every sigma must be >= 0 (or +inf)")
    return np.ascontiguousarray(s)


def _check_classes(name, cls, nt):
    """A class array (uint8, NumPy or tensor) of nt samples."""
    if D.is_tensor(cls):
        if cls.dtype != D.torch.uint8 or cls.dim() != 1:
            raise ValueError("%s must be a one-dimensional uint8 tensor, got %s %s" % (name, cls.dtype,
                                                                                      tuple(cls.shape)))
        n = int(cls.numel())
    else:
        a = np.asarray(cls)
        if a.dtype != np.uint8 or a.ndim != 1:
            raise ValueError("%s must be a one-dimensional uint8 array, got %s %s" % (name, a.dtype, a.shape))
        n = int(a.size)
    if n != nt:
        raise ValueError("%s has %d samples, the stream %d" % (name, n, nt))


def _check_dev(name, x, n, dtype):
    """A tensor in HBM of n elements that an earlier call of a stage returned."""
    if not (D.is_tensor(x) and x.is_cuda and x.dim() == 1 and x.is_contiguous()):
        raise ValueError("%s must be a contiguous one-dimensional tensor in HBM" % name)
    if str(x.dtype) != "torch." + dtype or int(x.numel()) != n:
        raise ValueError("%s must hold %d %s elements, got %d %s" % (name, n, dtype, x.numel(), x.dtype))


class _StageHandle(_hip.Handle):
    """Owns the library's handle of a :class:`_BlockStage` for one stream length: ``cm2_<prefix>_create`` with the
    block sizes and the stage's window, ``cm2_<prefix>_info`` (``info_names``) and ``cm2_<prefix>_destroy``."""
    prefix, info_names = None, ()

    def __init__(self, nt, sizes, window):
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        h = ctypes.c_void_p()
        _hip.call("cm2_%s_create" % self.prefix, ctypes.byref(h), int(nt),
                  sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(sizes), int(window), D.stream())
        _hip.Handle.__init__(self, "cm2_%s_destroy" % self.prefix, h)

    def info(self):
        info = (ctypes.c_int64 * len(self.info_names))()
        _hip.call("cm2_%s_info" % self.prefix, self.h, info)
        return dict(zip(self.info_names, [int(v) for v in info]))


class _BlockStage(object):
    """
    A stage over the noise blocks ``blocksize`` (BlockLO's convention) of time streams of any length: the checks of a
    stream and its block sizes, and one handle per stream length met.  A stage names its ``handle_class``, the
    attribute that holds its ``window``, itself (``noun``) and whose limit the number of blocks is (``histograms``)
    for the messages, and the argument that brings the classes of an earlier pass (``prev_name``).
    """
    handle_class, window, noun, histograms, prev_name = None, None, None, None, "prev"

    def __init__(self, blocksize):
        if np.ndim(blocksize) == 0:
            self.blocksize = _int("blocksize", blocksize)
            if self.blocksize < 1:
                raise ValueError("blocksize=%d < 1" % self.blocksize)
        else:
            self.blocksize = _block_sizes(blocksize, sum(_int("blocksize[%d]" % i, b)
                                                         for i, b in enumerate(blocksize)))
        self._handles = {}

    # ---- checks (no GPU) ----
    def _sizes(self, nt):
        sizes = _block_sizes(self.blocksize, nt)
        if nt > _MAX_NT:
            raise ValueError("%d samples do not fit the 32-bit sample counts of the %s" % (nt, self.noun))
        if len(sizes) > _MAX_BLOCKS:
            raise ValueError("%d blocks are more than the %d %s allow" % (len(sizes), _MAX_BLOCKS, self.histograms))
        return sizes

    def _check_stream(self, d, flags=None, prev=None):
        nt = _tod_length(d)
        if nt < 1:
            raise ValueError("the TOD has no samples")
        if flags is not None:
            _check_flags(flags, nt)
        _check_tod("d", d, nt)
        if prev is not None:
            _check_classes(self.prev_name, prev, nt)
        return nt, self._sizes(nt)

    # ---- device ----
    def _handle(self, nt, sizes):
        if nt not in self._handles:
            self._handles[nt] = self.handle_class(nt, sizes, getattr(self, self.window))
        return self._handles[nt]

    def info(self, nt):
        sizes = self._sizes(_int("nt", nt))
        D.require_gpu()
        return self._handle(int(nt), sizes).info()

    @staticmethod
    def _dev_flags(flags):
        if flags is None:
            return None, 0
        return _flags_to_dev(flags)
