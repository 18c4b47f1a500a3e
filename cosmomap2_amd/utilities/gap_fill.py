"""
Gap filling: values for the flagged samples of a time stream, on the GPU (the reference flags samples with
``pix = -1``, utilities/IOfiles.py:142-152 and process_ces.py:403-418, and has no gap filling).

    d0 = fill_gaps_linear(d, pix, blocksize)               # bootstrap: a line across every run
    N  = estimate_inverse_noise(d0, blocksize, lam)        # BlockLO(blocksize, bands, offdiag=True)
    gf = GapFiller(pix, N)                                 # index of the gaps, buffers, Jacobi vector
    d1, info = gf.fill(d)                                  # conditional mean of the gaps given the valid samples
    d2, info = gf.fill(d, sim=NoiseSimulator(...), realization=3)      # a constrained realisation
    b  = P.T * N * d1                                      # the gap-aware GLS right-hand side

**Flags.**  ``flags[i] < 0`` for an integer array (the ``pix`` array as ``SparseLO`` takes it), ``flags[i]``
true for a bool array; a NumPy array or a tensor.

**Constrained fill.**  With G the flagged samples, V the valid ones and Q = N^-1 (block-banded Toeplitz, the
blocks independent):

    n        = sim.draw(realization)             (0 when sim is None)
    u_i      = 0 where flagged, n_i - d_i elsewhere            (a select, never a product)
    b        = (N^-1 u)_G
    solve      Q_GG y = b,   Q_GG y := (N^-1 scatter(y))_G
    filled_i = d_i where valid (bit-equal), n_i + y_j at the j-th flagged sample

``sim=None`` gives the conditional mean ``x_G = -Q_GG^-1 Q_GV d_V``, and then ``(N^-1 filled)_V =
(Q_VV - Q_VG Q_GG^-1 Q_GV) d_V``: the Schur complement, the inverse covariance of the valid samples alone, so
``P.T * N * filled`` is the gap-aware right-hand side of the GLS map.  With a simulator the fill is a
constrained realisation (Hoffman-Ribak), which has the fluctuations a PSD estimate needs.  The solve is
:func:`cosmomap2_amd.cg` on compact vectors of ``ng`` values with the Jacobi preconditioner ``1 / a_0(block)``;
one iteration costs one time-order N^-1 plus ``ng``-sized traffic.  What ``d`` holds at a flagged sample never
reaches the output (a NaN there does no harm).  A stream without flagged samples comes back as it is, without
a solve; a wholly flagged block gets ``n`` (zeros without ``sim``).

**Linear fill.**  For each run ``[s, s + len)`` of flagged samples inside its noise block, ``L`` is the mean of the
valid samples among the ``nedge`` samples before ``s`` inside the block and ``R`` the same after the run; a side
without a valid sample takes the other side's level, both without: 0.  Sample ``s + k`` becomes
``L + (R - L) (k + 1) / (len + 1)``; valid samples are copied bit for bit.  A run that crosses a block boundary is
two runs.  ``nedge`` above the stream's length means the stream's length.

``d`` and ``out`` are float64 tensors in HBM or NumPy arrays.  Every argument is checked before the GPU is
touched (``ValueError``); without a GPU a valid call raises ``HipError`` like every operator constructor.  On
several GPUs each rank fills its own blocks (``sharding.shard_blocks``) with its own :class:`GapFiller` and a
simulator made with ``first_block = k0``: blocks are independent, so this is the same fill up to the solver's
tolerance (not bit for bit: cg's scalars span the blocks of a rank).
"""
import ctypes
import math

import numpy as np

from .. import _hip
from .. import device as D
from ._stream_args import _block_sizes, _check_flags, _check_out, _check_tod, _flags_to_dev, _int, _u64
from .noise_sim import NoiseSimulator

__all__ = ["GapFiller", "fill_gaps_linear"]


def _check_nedge(nedge):
    nedge = _int("nedge", nedge)
    if nedge < 1:
        raise ValueError("nedge=%d < 1" % nedge)
    return nedge


class _Gaps(_hip.Handle):
    """Owns a cm2_gaps handle and the device flags it reads."""

    def __init__(self, flags, sizes, a0=None):
        self.flags, kind = _flags_to_dev(flags)
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        pa = None
        if a0 is not None:
            a0 = np.ascontiguousarray(a0, dtype=np.float64)
            pa = a0.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        h = ctypes.c_void_p()
        _hip.call("cm2_gaps_create", ctypes.byref(h), D.ptr(self.flags), kind, int(sum(sizes)),
                  sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(sizes), pa, D.stream())
        _hip.Handle.__init__(self, "cm2_gaps_destroy", h)

    def info(self):
        info = (ctypes.c_int64 * 5)()
        _hip.call("cm2_gaps_info", self.h, info)
        return dict(zip(("nt", "ng", "runs", "longest_run", "buffer_bytes"), [int(v) for v in info]))

    def index(self):
        """(positions [ng] uint32, runs [nruns, 3] int64 = start, length, block) as NumPy arrays."""
        i = self.info()
        pos = np.empty(i["ng"], dtype=np.uint32)
        runs = np.empty((i["runs"], 3), dtype=np.int64)
        _hip.call("cm2_gaps_index", self.h, pos.ctypes.data, runs.ctypes.data, D.stream())
        return pos, runs

    def fill_linear(self, d, nedge, out):
        return _run_fill(d, out, lambda x, y: _hip.call("cm2_gaps_fill_linear", self.h, D.ptr(x), D.ptr(y), nedge,
                                                        D.stream()))


def _run_fill(d, out, run):
    """``run(x, y)`` from the device copy x of ``d`` into a device vector y, returned the way ``out`` asks:
    a new tensor (None), the tensor given, or the NumPy array given; a NumPy ``d`` without ``out`` gives NumPy."""
    x = D.f64(d)
    y = out if D.is_tensor(out) else D.empty(x.numel())
    run(x, y)
    if D.is_tensor(out):
        return out
    if out is not None:
        out[:] = D.to_host(y)
        return out
    return y if D.is_dev(d) else D.to_host(y)


def fill_gaps_linear(d, flags, blocksize, nedge=32, out=None):
    """
    ``d`` with every run of flagged samples replaced by a straight line between the mean levels of its two edges
    (the module's docstring has the definition): the bootstrap before any noise model exists.  ``blocksize``
    follows ``BlockLO`` (an int dividing ``len(d)``, or a list of block sizes).  Returns a new vector of ``d``'s
    kind, or ``out``.
    """
    nt = _check_flags(flags)
    _check_tod("d", d, nt)
    sizes = _block_sizes(blocksize, nt)
    nedge = min(_check_nedge(nedge), nt)            # no edge window reaches further; the C side takes an int64
    _check_out(out, nt)
    D.require_gpu()
    return _Gaps(flags, sizes).fill_linear(d, nedge, out)


class GapFiller(object):
    """
    Fills the flagged samples of time streams that share ``flags`` and the inverse noise ``N``, a Toeplitz
    ``BlockLO`` (``offdiag=True``).  The object owns the index of the gaps (``ng``, positions, runs cut at the
    block boundaries), the compact Jacobi vector and two buffers of ``nt`` doubles; a solve allocates nothing of
    TOD size.  After :meth:`fill`, ``iterations`` is cg's iteration count and ``relative_residual`` the final
    ``|b - Q_GG y| / |b|`` (one more application of the operator, made when the attribute is read).
    """

    def __init__(self, flags, N):
        from ..interfaces.linearoperators import BlockLO
        if not isinstance(N, BlockLO) or not N.isoffdiag:
            raise ValueError("N must be a Toeplitz BlockLO (offdiag=True), got %s%s"
                             % (type(N).__name__, " with offdiag=False" if isinstance(N, BlockLO) else ""))
        self.sizes, self.nt = list(N._sizes), int(N._nt)
        _check_flags(flags, self.nt)
        a0 = [float(np.atleast_1d(np.asarray(b, dtype=np.float64))[0]) for b in N.covnoise]
        if not all(np.isfinite(a) and a > 0 for a in a0):
            raise ValueError("every block's band must start with a positive a_0, got %r" % (a0,))
        self.N = N
        D.require_gpu()
        self._gaps = _Gaps(flags, self.sizes, a0)
        info = self._gaps.info()
        self.ng, self.runs, self.longest_run = info["ng"], info["runs"], info["longest_run"]
        self.iterations = 0
        self._n = None                 # the simulator's draw, kept between fills
        self._b = self._y = self._relres = None

    def info(self):
        return self._gaps.info()

    def index(self):
        """(positions of the flagged samples, runs as rows of start, length, block)."""
        return self._gaps.index()

    def normal_apply(self, y):
        """``Q_GG y`` for a compact float64 tensor of ``ng`` values in HBM."""
        out = D.empty(self.ng)
        _hip.call("cm2_gaps_normal_apply", self._gaps.h, self.N._noise.h, D.ptr(y), D.ptr(out), D.stream())
        return out

    def _precond(self, r):
        z = D.empty(self.ng)
        _hip.call("cm2_gaps_precond_apply", self._gaps.h, D.ptr(r), D.ptr(z), D.stream())
        return z

    @property
    def relative_residual(self):
        if self._relres is None:
            if self._b is None:
                return 0.0
            bb = D.dot(self._b, self._b)
            r = D.add_scaled(self._b, -1.0, self.normal_apply(self._y))
            self._relres = math.sqrt(D.dot(r, r) / bb) if bb > 0 else 0.0
        return self._relres

    def fill(self, d, sim=None, realization=0, rtol=1e-8, maxiter=None, out=None, callback=None):
        """
        ``(filled, info)``: ``d`` with its flagged samples replaced by the conditional mean given the valid ones
        (``sim=None``) or by realisation ``realization`` of ``sim`` constrained to them; ``info`` is cg's (0:
        converged to ``rtol |b|``, else ``maxiter``).  ``filled`` is a new vector of ``d``'s kind, or ``out``
        (which may be ``d`` itself).  ``callback`` is handed to cg (called with the compact iterate).
        """
        _check_tod("d", d, self.nt)
        if sim is not None:
            if not isinstance(sim, NoiseSimulator):
                raise ValueError("sim must be a NoiseSimulator or None, got %r" % (sim,))
            if sim.nt != self.nt or list(sim.sizes) != self.sizes:
                raise ValueError("the simulator draws blocks %r, N has %r" % (list(sim.sizes), self.sizes))
        realization = _u64("realization", realization)
        try:
            rtol = float(rtol)
        except (TypeError, ValueError):
            raise ValueError("rtol must be a positive number, got %r" % (rtol,))
        if not (np.isfinite(rtol) and rtol > 0):
            raise ValueError("rtol must be a positive number, got %r" % (rtol,))
        if maxiter is not None and _int("maxiter", maxiter) < 1:
            raise ValueError("maxiter=%d < 1" % maxiter)
        _check_out(out, self.nt)
        D.require_gpu()
        self.iterations, self._b, self._y, self._relres = 0, None, None, None
        return _run_fill(d, out, lambda x, y: self._fill_dev(x, y, sim, realization, rtol, maxiter, callback)), \
            self._info

    def _fill_dev(self, x, out, sim, realization, rtol, maxiter, callback):
        from ..solvers import cg
        g, st = self._gaps.h, D.stream
        self._info = 0
        if self.ng == 0:
            _hip.call("cm2_gaps_finish", g, D.ptr(x), None, None, D.ptr(out), st())
            return
        n = None
        if sim is not None:
            if self._n is None:
                self._n = D.empty(self.nt)
            n = sim.draw(realization, out=self._n)
        # `out` is free until the last step: it holds u, unless it is d itself
        u = out if out.data_ptr() != x.data_ptr() else D.empty(self.nt)
        b = D.empty(self.ng)
        _hip.call("cm2_gaps_rhs", g, self.N._noise.h, D.ptr(n), D.ptr(x), D.ptr(u), D.ptr(b), st())
        del u
        its = []

        def count(yk):
            its.append(1)
            if callback is not None:
                callback(yk)

        y, self._info = cg(self.normal_apply, b, M=self._precond, rtol=rtol, maxiter=maxiter, callback=count)
        self.iterations, self._b, self._y = len(its), b, y
        _hip.call("cm2_gaps_finish", g, D.ptr(x), D.ptr(n), D.ptr(y), D.ptr(out), st())
