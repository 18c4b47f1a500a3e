"""
The GLS map of a time stream with flagged samples (``pix = -1``): every flagged sample gets an unknown of its own.

    op = GapAwareNormalLO(P, N)                       # A_e on vectors [map (pol npix) ; g (ng)]
    z, info = cg(op, op.rhs(d), M=op.preconditioner(Mbd))
    m, g = op.split(z)
    r = op.residual(d, z)                             # d - P m on the valid samples, -g in the gaps

or in one call ``m, info, op = solve_gls_with_gaps(P, N, d, M=Mbd)``.

``P`` and ``P^T`` skip flagged samples while the Toeplitz ``N^-1`` sees zeros there, so ``P.T * N * P`` is
``P_V^T Q_VV P_V`` (Q = N^-1, V the valid samples, G the flagged ones): the operator of a stream whose flagged
samples were *measured as zero*, not of one without them.  The inverse covariance of the valid samples alone is the
Schur complement ``S = Q_VV - Q_VG Q_GG^-1 Q_GV``, and the GLS map solves ``(P^T S P) m = P^T S d_V``.  With ``E``
the nt x ng matrix holding a one at (position of the j-th flagged sample, j) and ``P_e = [P E]``,

    A_e = P_e^T N^-1 P_e = [ P^T Q P   P^T Q E ]        b_e = P_e^T N^-1 d0,   d0 = d on V, 0 on G
                           [ E^T Q P   Q_GG    ]

and eliminating the gap unknowns from ``A_e z = b_e`` gives exactly that system; its second row is
``g = Q_GG^-1 Q_GV (d_V - P m)``, so ``-g`` is the conditional mean of the noise residual in the gaps.  One
application is P, ``g`` written into the flagged samples, one time-order ``N^-1``, the flagged samples read back,
``P^T``.  On the tile-bucketed pointing (``set_pointing_mode``) the two middle steps are the plan's windowed
permutations with the flagged samples merged in (``cm2_PtNP_gaps_apply``, cm2_gaps.hip); in the exact mode the
chain is ``cm2_P_apply, cm2_gaps_scatter, cm2_noise_apply, cm2_gaps_gather, cm2_Pt_apply``.

Vectors are float64 tensors in HBM or NumPy arrays.  Every argument is checked before the GPU is touched
(``ValueError``); without a GPU a valid call raises ``HipError`` like every operator constructor.
"""
import ctypes

import numpy as np

from .. import _hip
from .. import device as D
from .. import linop as lp
from ..utilities._stream_args import _check_rtol, _check_tod, _int
from ..utilities.gap_fill import _Gaps
from . import linearoperators as L

__all__ = ["GapAwareNormalLO", "solve_gls_with_gaps"]


def _check_operators(P, N):
    """(block sizes, nt, a_0 of every block) of a valid pair, without touching the GPU."""
    if not isinstance(P, L.SparseLO):
        raise ValueError("P must be a SparseLO, got %s" % type(P).__name__)
    if not isinstance(N, L.BlockLO) or not N.isoffdiag:
        raise ValueError("N must be a Toeplitz BlockLO (offdiag=True), got %s%s"
                         % (type(N).__name__, " with offdiag=False" if isinstance(N, L.BlockLO) else ""))
    sizes, nt = list(N._sizes), int(N._nt)
    if int(P.nrows) != nt:
        raise ValueError("P has %d samples, N %d" % (P.nrows, nt))
    a0 = [float(np.atleast_1d(np.asarray(b, dtype=np.float64))[0]) for b in N.covnoise]
    if not all(np.isfinite(a) and a > 0 for a in a0):
        raise ValueError("every block's band must start with a positive a_0, got %r" % (a0,))
    return sizes, nt, a0


class GapAwareNormalLO(L._DeviceOp):
    """
    ``A_e = [P E]^T N^-1 [P E]`` (the module's docstring has the definitions): symmetric positive definite on
    ``pol * npix + ng`` values, the map followed by one value per flagged sample of ``P`` in time order.  ``N`` is
    a Toeplitz ``BlockLO`` on ``P.nrows`` samples.  The index of the flagged samples is built from ``P``'s own
    device pixel stream, so the pointing and the gaps cannot disagree.  The operator keeps three TOD-sized scratch
    vectors for its life; an application allocates its result only.  ``ng == 0`` gives ``P.T * N * P``.

    ``nmap``, ``ng``: sizes of the two parts; ``split(z)`` returns them as views.  After
    :func:`solve_gls_with_gaps`, ``iterations`` is cg's iteration count and ``gap_solution`` the ``g`` part.
    """

    def __init__(self, P, N):
        self.sizes, self.nt, a0 = _check_operators(P, N)
        self.P, self.N = P, N
        self.nmap = int(P.pol) * int(P.ncols)
        D.require_gpu()
        self._gaps = _Gaps(P._d_pix, self.sizes, a0)
        self.ng = self._gaps.info()["ng"]
        self.iterations, self.gap_solution = 0, None
        self._t1 = self._t2 = self._tb = None
        self._prepared_plan = None
        n = self.nmap + self.ng
        super(GapAwareNormalLO, self).__init__(n, n, self._mult, symmetric=True)

    # -- pieces ----------------------------------------------------------------------
    def split(self, z):
        """``(map, g)``: the first ``nmap`` and the last ``ng`` values of ``z``, as views."""
        if z.shape[0] != self.nmap + self.ng:
            raise lp.ShapeError("vector has %d entries, expected %d" % (z.shape[0], self.nmap + self.ng))
        return z[:self.nmap], z[self.nmap:]

    def _tail(self, v):
        """Device address of the gap part of a device vector."""
        return v.data_ptr() + 8 * self.nmap

    def _time_scratch(self):
        if self._t1 is None:
            self._t1, self._t2 = D.empty(self.nt), D.empty(self.nt)
        return self._t1, self._t2

    def _tiles(self):
        """The tile plan of P, the handle prepared for it, and the tile-order scratch."""
        T = L._sparse_tiles(self.P)
        if self._prepared_plan != T.plan_id:
            _hip.call("cm2_gaps_prepare_tiles", self._gaps.h, T.h, D.stream())
            self._prepared_plan = T.plan_id
        if self._tb is None or self._tb.numel() != max(T.nvalid, 1):
            self._tb = D.empty(max(T.nvalid, 1))
        return T

    def window_table(self):
        """``c_w`` of the tiled path: flagged samples before every permutation window of 8192 time samples
        (``nwin + 1`` values), or None when the stream is shorter than one window."""
        self._tiles()
        nwin = ctypes.c_int64(0)
        _hip.call("cm2_gaps_window_table", self._gaps.h, ctypes.byref(nwin), None, D.stream())
        if not nwin.value:
            return None
        table = np.empty(nwin.value + 1, dtype=np.uint32)
        _hip.call("cm2_gaps_window_table", self._gaps.h, ctypes.byref(nwin), table.ctypes.data, D.stream())
        return table

    def _back_project(self, tod, out):
        """``out = [P^T tod ; tod on G]`` for a time-order device vector (tod is not changed)."""
        st = D.stream()
        if L._use_tiles(self.P):
            T = self._tiles()
            _hip.call("cm2_gaps_time_to_tiles", self._gaps.h, T.h, D.ptr(tod), D.ptr(self._tb), self._tail(out), st)
            _hip.call("cm2_Pt_tiles_apply", T.h, D.ptr(self._tb), D.ptr(out), st)
        else:
            _hip.call("cm2_gaps_gather", self._gaps.h, D.ptr(tod), self._tail(out), st)
            _hip.call("cm2_Pt_apply", self.P._plan, D.ptr(tod), D.ptr(out), st)

    # -- A_e z -----------------------------------------------------------------------
    def _mult(self, v):
        x = D.f64(v)
        n = self.nmap + self.ng
        if x.numel() != n:
            raise lp.ShapeError("vector has %d entries, expected %d" % (x.numel(), n))
        out = D.empty(n)
        t1, t2 = self._time_scratch()
        st = D.stream()
        if L._use_tiles(self.P):
            T = self._tiles()
            _hip.call("cm2_PtNP_gaps_apply", T.h, self.N._noise.h, self._gaps.h, D.ptr(x), D.ptr(out),
                      D.ptr(self._tb), D.ptr(t1), D.ptr(t2), st)
        else:
            _hip.call("cm2_P_apply", self.P._plan, D.ptr(x), D.ptr(t1), st)
            _hip.call("cm2_gaps_scatter", self._gaps.h, self._tail(x), D.ptr(t1), st)
            _hip.call("cm2_noise_apply", self.N._noise.h, D.ptr(t1), D.ptr(t2), st)
            self._back_project(t2, out)
        return D.like_input(out, v)

    # -- b_e -------------------------------------------------------------------------
    def rhs(self, d):
        """``b_e = [P E]^T N^-1 d0`` with ``d0 = d`` on the valid samples and 0 on the flagged ones.  ``d0`` is a
        select (``cm2_gaps_masked_diff``: -d on V, 0 on G, the sign taken back at the end, which is exact), so
        what ``d`` holds at a flagged sample -- a NaN, say -- never enters arithmetic that is kept."""
        _check_tod("d", d, self.nt)
        D.require_gpu()
        x = D.f64(d)
        out = D.empty(self.nmap + self.ng)
        t1, t2 = self._time_scratch()
        st = D.stream()
        _hip.call("cm2_gaps_masked_diff", self._gaps.h, None, D.ptr(x), D.ptr(t1), st)
        _hip.call("cm2_noise_apply", self.N._noise.h, D.ptr(t1), D.ptr(t2), st)
        self._back_project(t2, out)
        _hip.call("cm2_scal", out.numel(), -1.0, D.ptr(out), st)
        return D.like_input(out, d)

    # -- M_e -------------------------------------------------------------------------
    def preconditioner(self, Mbd=None):
        """``blockdiag(Mbd, 1 / a_0(block))`` on the concatenated vector: ``Mbd`` (a map-domain operator such as
        ``BlockDiagonalPreconditionerLO``; None = identity) on the map part, Jacobi on the gap part."""
        if Mbd is not None and tuple(getattr(Mbd, "shape", ())) != (self.nmap, self.nmap):
            raise ValueError("Mbd must be an operator on the %d map values, got shape %r"
                             % (self.nmap, getattr(Mbd, "shape", None)))
        n = self.nmap + self.ng

        def mult(r):
            x = D.f64(r)
            if x.numel() != n:
                raise lp.ShapeError("vector has %d entries, expected %d" % (x.numel(), n))
            out = D.empty(n)
            st = D.stream()
            if isinstance(Mbd, L.BlockDiagonalPreconditionerLO):
                _hip.call("cm2_bdprecond_apply", int(Mbd.pol), Mbd._w.npix, *(Mbd._w.ptrs() + [
                    D.ptr(Mbd._d_det), D.ptr(Mbd._d_mask), D.ptr(x), D.ptr(out), st]))
            elif Mbd is None:
                out[:self.nmap].copy_(x[:self.nmap])
            else:
                from ..solvers import _apply
                out[:self.nmap].copy_(_apply(Mbd, x[:self.nmap]))
            _hip.call("cm2_gaps_precond_apply", self._gaps.h, self._tail(x), self._tail(out), st)
            return D.like_input(out, r)

        return L._DeviceOp(n, n, mult, symmetric=True)

    # -- residual --------------------------------------------------------------------
    def residual(self, d, z):
        """``d - P m`` on the valid samples and ``-g`` on the flagged ones for ``z = [m ; g]``: the noise residual
        with its gaps filled by their conditional mean, ``-g = -Q_GG^-1 Q_GV (d_V - P m)`` at the solution -- the
        stream a PSD estimate (``estimate_inverse_noise``) wants.  A new vector of ``d``'s kind."""
        _check_tod("d", d, self.nt)
        if np.ndim(z) != 1 or z.shape[0] != self.nmap + self.ng:
            raise ValueError("z must hold %d values (map and gaps), got shape %r"
                             % (self.nmap + self.ng, tuple(np.shape(z))))
        D.require_gpu()
        x, zd = D.f64(d), D.f64(z)
        t1, _ = self._time_scratch()
        out = D.empty(self.nt)
        st = D.stream()
        _hip.call("cm2_P_apply", self.P._plan, D.ptr(zd), D.ptr(t1), st)
        _hip.call("cm2_gaps_masked_diff", self._gaps.h, D.ptr(x), D.ptr(t1), D.ptr(out), st)
        if self.ng:
            y = D.scaled(-1.0, zd[self.nmap:])
            _hip.call("cm2_gaps_finish", self._gaps.h, D.ptr(out), None, D.ptr(y), D.ptr(out), st)
        return D.like_input(out, d)


def solve_gls_with_gaps(P, N, d, M=None, rtol=1e-6, maxiter=None, x0=None, callback=None):
    """
    ``(map, info, op)``: the GLS map of ``d`` given its valid samples alone, ``(P^T S P) m = P^T S d_V``, by
    :func:`cosmomap2_amd.cg` on the extended system ``A_e z = b_e`` of :class:`GapAwareNormalLO`.

    ``M`` is the map-domain preconditioner (``BlockDiagonalPreconditionerLO``, or None); the gap unknowns get the
    Jacobi ``1 / a_0(block)`` (``op.preconditioner(M)``).  ``x0`` starts the map (``pol * npix`` values, the gap
    unknowns from 0) or the whole vector (``pol * npix + ng``).  ``callback`` is handed to cg and receives the whole
    iterate.  ``info`` is cg's int (0: converged to ``rtol |b_e|``, else ``maxiter``).  The operator comes back as
    the third value: it carries ``iterations``, ``gap_solution`` (``g``, of ``d``'s kind) and ``residual(d, z)``,
    and can be kept for further solves with the same pointing and noise.  ``map`` is of ``d``'s kind.
    """
    from ..solvers import cg
    _, nt, _ = _check_operators(P, N)
    _check_tod("d", d, nt)
    rtol = _check_rtol(rtol)
    if maxiter is not None and _int("maxiter", maxiter) < 1:
        raise ValueError("maxiter=%d < 1" % maxiter)
    nmap = int(P.pol) * int(P.ncols)
    if M is not None and tuple(getattr(M, "shape", ())) != (nmap, nmap):
        raise ValueError("M must be an operator on the %d map values, got shape %r" % (nmap, getattr(M, "shape", None)))
    if x0 is not None and (np.ndim(x0) != 1 or np.shape(x0)[0] < nmap):
        raise ValueError("x0 must hold the %d map values (or the map and the gaps), got shape %r"
                         % (nmap, tuple(np.shape(x0))))
    if callback is not None and not callable(callback):
        raise ValueError("callback must be callable, got %r" % (callback,))
    op = GapAwareNormalLO(P, N)
    n = op.nmap + op.ng
    if x0 is not None:
        if np.shape(x0)[0] not in (nmap, n):
            raise ValueError("x0 has %d values, the map %d and the gaps %d" % (np.shape(x0)[0], nmap, op.ng))
        start = D.zeros(n)
        start[:np.shape(x0)[0]].copy_(D.f64(x0))
        x0 = start
    b = D.f64(op.rhs(D.f64(d)))
    its = []

    def count(zk):
        its.append(1)
        if callback is not None:
            callback(zk)

    z, info = cg(op, b, x0=x0, M=op.preconditioner(M), rtol=rtol, maxiter=maxiter, callback=count)
    m, g = op.split(z)
    op.iterations = len(its)
    op.gap_solution = D.like_input(g, d)
    return D.like_input(m, d), info, op
