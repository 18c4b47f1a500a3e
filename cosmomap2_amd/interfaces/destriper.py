"""
Destriping: the correlated noise of a time stream as one constant offset per baseline, solved for and removed.

    m, a, info, op = solve_destriped(P, blocksize, baseline_length, d, Mbd, weights=w)
    cleaned = op.cleaned(d, a)                       # d - F a on the valid samples, 0 on the flagged ones

or piece by piece

    F = OffsetsLO(P, blocksize, baseline_length, weights=w)        # nt x na
    op = DestriperNormalLO(P, F, Mbd, prior=None)                  # A on na values
    a, info = cg(op, op.rhs(d), M=op.preconditioner())
    m = op.map(d, a)

**Baselines.**  The stream has noise blocks as ``BlockLO`` takes them (``blocksize``: an int dividing ``nt`` or a
list); block ``b`` is the samples ``[o_b, o_b + n_b)``.  ``baseline_length = L >= 1`` cuts block ``b`` into
``K_b = ceil(n_b / L)`` baselines ``[o_b + k L, min(o_b + (k + 1) L, o_b + n_b))`` with the global index
``j = sum_{b' < b} K_b' + k``; ``na = sum K_b``.  Baselines never cross a block boundary.

**Weights.**  A sample is valid when ``pix >= 0`` in ``P``'s own device pixel stream.  ``weights`` is None (all 1) or
one positive finite ``w_b`` per block; ``w_t = w_b`` on the valid samples and 0 on the flagged ones, ``W = diag(w_t)``.
``nvalid_j`` counts the valid samples of baseline ``j`` and ``wsum_j = w_b nvalid_j``.

**Operators.**  ``(F a)_t = a_j(t)`` on the valid samples and 0 on the flagged ones, ``(F^T y)_j`` the sum of ``y_t``
over the valid samples of baseline ``j``.  With ``M = M_BD = (P^T W P)^-1`` (built by the caller from a
``ProcessTimeSamples`` with the same per-sample ``w``) and an optional symmetric prior ``C_a^-1`` on ``na`` values

    A a = wsum o a - F^T W P M P^T W F a (+ C_a^-1 a)      b = F^T W (d0 - P M P^T W d0),  d0 = d on valid, 0 on flagged
    m   = M P^T W (d0 - F a)

the Schur complement of ``[P F]^T W [P F] z = [P F]^T W d0``.  ``F^T W F = diag(wsum)`` is used as such.  A baseline
without a valid sample has the identity as its row and column and ``b_j = 0`` (with a prior: the prior's row).
Without a prior ``A`` is singular along the constant vector on the non-empty baselines for pol 1 and 3 (the map's
``I`` monopole); ``b`` is in its range and CG from 0 converges; ``d0 - F a - P m`` on the valid samples is unique.

On the tile-bucketed pointing (``set_pointing_mode``) one application is ``cm2_offsets_to_tiles ->
cm2_Pt_tiles_apply -> cm2_bdprecond_apply -> cm2_P_tiles_apply -> cm2_offsets_from_tiles``; in the exact mode the
time-order kernels stand around ``cm2_Pt_apply`` / ``cm2_P_apply``.

Vectors are float64 tensors in HBM or NumPy arrays.  Every argument is checked before the GPU is touched
(``ValueError``); without a GPU a valid call raises ``HipError``.
"""
import ctypes

import numpy as np

from .. import _hip
from .. import device as D
from .. import linop as lp
from ..utilities._stream_args import _block_sizes, _check_rtol, _check_tod, _int
from . import linearoperators as L

__all__ = ["OffsetsLO", "DestriperNormalLO", "solve_destriped"]

_I64P = ctypes.POINTER(ctypes.c_int64)
_DBLP = ctypes.POINTER(ctypes.c_double)


def _check_offsets_args(P, blocksize, baseline_length, weights):
    """(sizes, L, weights as an array or None, baselines per block) of valid arguments, without the GPU."""
    if not isinstance(P, L.SparseLO):
        raise ValueError("P must be a SparseLO, got %s" % type(P).__name__)
    nt = int(P.nrows)
    sizes = _block_sizes(blocksize, nt)
    Lb = _int("baseline_length", baseline_length)
    if Lb < 1:
        raise ValueError("baseline_length=%d < 1" % Lb)
    if nt >= 2 ** 32 - 1:
        raise ValueError("nt=%d does not fit the 32-bit sample index" % nt)
    per_block = [-(-n // Lb) for n in sizes]
    if sum(per_block) >= 2 ** 31:
        raise ValueError("%d baselines do not fit the 31-bit baseline index" % sum(per_block))
    w = None
    if weights is not None:
        try:
            w = np.ascontiguousarray(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("weights must be one positive number per block, got %r" % (weights,))
        if w.ndim != 1 or w.size != len(sizes):
            raise ValueError("weights must hold one value per block (%d), got shape %r" % (len(sizes), w.shape))
        if not np.all(np.isfinite(w) & (w > 0)):
            raise ValueError("weights must be positive and finite, got %r" % (w.tolist(),))
    return sizes, Lb, w, per_block


class _Offsets(_hip.Handle):
    """Owns a cm2_offsets handle and the device pixel stream it reads."""

    def __init__(self, d_pix, sizes, Lb, w):
        self.pix = d_pix
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        h = ctypes.c_void_p()
        _hip.call("cm2_offsets_create", ctypes.byref(h), D.ptr(d_pix), int(sz.sum()), sz.ctypes.data_as(_I64P),
                  len(sizes), int(Lb), None if w is None else w.ctypes.data_as(_DBLP), D.stream())
        _hip.Handle.__init__(self, "cm2_offsets_destroy", h)

    def info(self):
        info = (ctypes.c_int64 * 8)()
        _hip.call("cm2_offsets_info", self.h, info)
        return dict(zip(("nt", "nblocks", "baseline_length", "na", "nvalid", "windows", "tile_forms", "lds_bytes"),
                        [int(v) for v in info]))

    def counts(self, na):
        nvalid, wsum = np.empty(na, dtype=np.int64), np.empty(na, dtype=np.float64)
        _hip.call("cm2_offsets_counts", self.h, nvalid.ctypes.data, wsum.ctypes.data, D.stream())
        return nvalid, wsum


class OffsetsLO(L._DeviceOp):
    """
    ``F``, the ``nt x na`` baseline-offset template operator of the pointing ``P`` (the module's docstring has the
    definitions): ``F * a`` spreads every offset over the valid samples of its baseline, ``F.T * y`` sums the valid
    samples of every baseline, both unweighted.  The flags are ``P``'s own device pixel stream, so the pointing and
    the templates cannot disagree.

    ``na``, ``baselines_per_block`` (a list), ``nvalid`` (int64 array), ``wsum`` (``w_b nvalid_j``), ``sizes``,
    ``baseline_length``, ``weights`` (array or None).
    """

    def __init__(self, P, blocksize, baseline_length, weights=None):
        self.sizes, self.baseline_length, self.weights, self.baselines_per_block = \
            _check_offsets_args(P, blocksize, baseline_length, weights)
        self.P = P
        self.nt = int(P.nrows)
        self.na = int(sum(self.baselines_per_block))
        D.require_gpu()
        self._f = _Offsets(P._d_pix, self.sizes, self.baseline_length, self.weights)
        self.nvalid, self.wsum = self._f.counts(self.na)
        self._prepared_plan = None
        super(OffsetsLO, self).__init__(nargin=self.na, nargout=self.nt, matvec=self._expand, symmetric=False,
                                        rmatvec=self._sum)

    def _expand(self, a):
        x = D.f64(a)
        if x.numel() != self.na:
            raise lp.ShapeError("offset vector has %d entries, expected %d" % (x.numel(), self.na))
        out = D.empty(self.nt)
        _hip.call("cm2_offsets_expand", self._f.h, D.ptr(x), 0, D.ptr(out), D.stream())
        return D.like_input(out, a)

    def _sum(self, y):
        x = D.f64(y)
        if x.numel() != self.nt:
            raise lp.ShapeError("time-domain vector has %d entries, expected %d" % (x.numel(), self.nt))
        out = D.empty(self.na)
        _hip.call("cm2_offsets_sum", self._f.h, D.ptr(x), 0, D.ptr(out), D.stream())
        return D.like_input(out, y)

    def _tiles(self):
        """The tile plan of P, with the handle prepared for it."""
        T = L._sparse_tiles(self.P)
        if self._prepared_plan != T.plan_id:
            _hip.call("cm2_offsets_prepare_tiles", self._f.h, T.h, D.stream())
            self._prepared_plan = T.plan_id
        return T


def _check_normal_args(P, F, Mbd, prior):
    if not isinstance(P, L.SparseLO):
        raise ValueError("P must be a SparseLO, got %s" % type(P).__name__)
    if not isinstance(F, OffsetsLO):
        raise ValueError("F must be an OffsetsLO, got %s" % type(F).__name__)
    if F.P is not P:
        raise ValueError("F was built for another pointing operator than P")
    _check_mbd(P, Mbd)
    _check_prior(prior, F.na)


def _check_mbd(P, Mbd):
    nmap = int(P.pol) * int(P.ncols)
    if not isinstance(Mbd, L.BlockDiagonalPreconditionerLO):
        raise ValueError("Mbd must be a BlockDiagonalPreconditionerLO, got %s" % type(Mbd).__name__)
    if tuple(Mbd.shape) != (nmap, nmap) or int(Mbd.pol) != int(P.pol):
        raise ValueError("Mbd must act on the %d map values of P (pol %d), got shape %r, pol %r"
                         % (nmap, P.pol, tuple(Mbd.shape), Mbd.pol))


def _check_prior(prior, na):
    if prior is None:
        return
    shape = tuple(getattr(prior, "shape", ()))
    if shape != (na, na):
        raise ValueError("prior must be a symmetric operator on the %d offsets, got shape %r" % (na, shape or None))
    if getattr(prior, "symmetric", True) is False:
        raise ValueError("prior must be a symmetric operator, got one that says it is not")


def _prior_diagonal(prior, F):
    """c_0 of every baseline: the first band value of the prior's block when it is a Toeplitz BlockLO, else 0."""
    c0 = np.zeros(F.na)
    if isinstance(prior, L.BlockLO) and prior.isoffdiag:
        first = [float(np.atleast_1d(np.asarray(b, dtype=np.float64))[0]) for b in prior.covnoise]
        c0 = np.repeat(first, prior._sizes).astype(np.float64)
    return c0


class DestriperNormalLO(L._DeviceOp):
    """
    ``A = diag(wsum) - F^T W P M P^T W F (+ C_a^-1)`` on the ``na`` offsets (the module's docstring has the
    definitions): symmetric, positive semi-definite.  ``F`` is the :class:`OffsetsLO` of ``P``, ``Mbd`` the
    ``BlockDiagonalPreconditionerLO`` of the same weights, ``prior`` None or a symmetric operator on ``na`` values
    (typically ``BlockLO(F.baselines_per_block, bands, offdiag=True)``).  The operator keeps its scratch (a map pair,
    ``na`` values and a TOD-sized vector or two) for its life; an application allocates its result only.

    ``rhs(d)``, ``preconditioner()``, ``map(d, a)``, ``cleaned(d, a)``; after :func:`solve_destriped`,
    ``iterations`` is cg's iteration count.
    """

    def __init__(self, P, F, Mbd, prior=None):
        _check_normal_args(P, F, Mbd, prior)
        self.P, self.F, self.Mbd, self.prior = P, F, Mbd, prior
        self.nt, self.na = F.nt, F.na
        self.nmap = int(P.pol) * int(P.ncols)
        self.iterations = 0
        D.require_gpu()
        diag = F.wsum.copy()
        if prior is None:
            diag[F.nvalid == 0] = 1.0               # an empty baseline: the identity row
        self._diag = D.f64(diag)
        self._m1, self._m2 = D.empty(self.nmap), D.empty(self.nmap)
        self._s = D.empty(self.na)
        self._t1 = self._t2 = self._tb = None
        super(DestriperNormalLO, self).__init__(self.na, self.na, self._mult, symmetric=True)

    # -- scratch ---------------------------------------------------------------------
    def _time_scratch(self, two=False):
        if self._t1 is None:
            self._t1 = D.empty(self.nt)
        if two and self._t2 is None:
            self._t2 = D.empty(self.nt)
        return self._t1, self._t2

    def _tiles(self):
        T = self.F._tiles()
        if self._tb is None or self._tb.numel() != max(T.nvalid, 1):
            self._tb = D.empty(max(T.nvalid, 1))
        return T

    def _precond_map(self, src, dst):
        M = self.Mbd
        _hip.call("cm2_bdprecond_apply", int(M.pol), M._w.npix, *(M._w.ptrs() + [
            D.ptr(M._d_det), D.ptr(M._d_mask), D.ptr(src), D.ptr(dst), D.stream()]))

    def _binned(self, wtod, out):
        """``out = M P^T wtod`` for a weighted time-order device vector (the map scratch m1 is used)."""
        st = D.stream()
        if L._use_tiles(self.P):
            T = self._tiles()
            _hip.call("cm2_tod_time_to_tiles", T.h, D.ptr(wtod), D.ptr(self._tb), st)
            _hip.call("cm2_Pt_tiles_apply", T.h, D.ptr(self._tb), D.ptr(self._m1), st)
        else:
            _hip.call("cm2_Pt_apply", self.P._plan, D.ptr(wtod), D.ptr(self._m1), st)
        self._precond_map(self._m1, out)

    # -- A a -------------------------------------------------------------------------
    def _mult(self, v):
        x = D.f64(v)
        if x.numel() != self.na:
            raise lp.ShapeError("vector has %d entries, expected %d" % (x.numel(), self.na))
        st = D.stream()
        h = self.F._f.h
        if L._use_tiles(self.P):
            T = self._tiles()
            _hip.call("cm2_offsets_to_tiles", h, T.h, D.ptr(x), 1, D.ptr(self._tb), st)
            _hip.call("cm2_Pt_tiles_apply", T.h, D.ptr(self._tb), D.ptr(self._m1), st)
            self._precond_map(self._m1, self._m2)
            _hip.call("cm2_P_tiles_apply", T.h, D.ptr(self._m2), D.ptr(self._tb), st)
            _hip.call("cm2_offsets_from_tiles", h, T.h, D.ptr(self._tb), 1, D.ptr(self._s), st)
        else:
            t1, _ = self._time_scratch()
            _hip.call("cm2_offsets_expand", h, D.ptr(x), 1, D.ptr(t1), st)
            _hip.call("cm2_Pt_apply", self.P._plan, D.ptr(t1), D.ptr(self._m1), st)
            self._precond_map(self._m1, self._m2)
            _hip.call("cm2_P_apply", self.P._plan, D.ptr(self._m2), D.ptr(t1), st)
            _hip.call("cm2_offsets_sum", h, D.ptr(t1), 1, D.ptr(self._s), st)
        out = D.empty(self.na)
        _hip.call("cm2_xmy", self.na, D.ptr(self._diag), D.ptr(x), D.ptr(out), st)
        _hip.call("cm2_axpy", self.na, -1.0, D.ptr(self._s), D.ptr(out), st)
        if self.prior is not None:
            from ..solvers import _apply
            _hip.call("cm2_axpy", self.na, 1.0, D.ptr(_apply(self.prior, x)), D.ptr(out), st)
        return D.like_input(out, v)

    # -- b ---------------------------------------------------------------------------
    def rhs(self, d):
        """``b = F^T W (d0 - P M P^T W d0)``.  ``d0`` is a select (``cm2_offsets_residual``), so what ``d`` holds at
        a flagged sample -- a NaN, say -- never enters arithmetic that is kept."""
        _check_tod("d", d, self.nt)
        D.require_gpu()
        x = D.f64(d)
        st = D.stream()
        h = self.F._f.h
        t1, t2 = self._time_scratch(two=True)
        _hip.call("cm2_offsets_residual", h, D.ptr(x), None, 1, D.ptr(t1), st)          # W d0
        self._binned(t1, self._m2)                                                      # M P^T W d0
        _hip.call("cm2_P_apply", self.P._plan, D.ptr(self._m2), D.ptr(t2), st)
        _hip.call("cm2_offsets_residual", h, D.ptr(x), None, 0, D.ptr(t1), st)          # d0
        _hip.call("cm2_axpy", self.nt, -1.0, D.ptr(t2), D.ptr(t1), st)                  # d0 - P M P^T W d0
        out = D.empty(self.na)
        _hip.call("cm2_offsets_sum", h, D.ptr(t1), 1, D.ptr(out), st)
        return D.like_input(out, d)

    # -- Jacobi ----------------------------------------------------------------------
    def preconditioner(self):
        """Jacobi: ``1 / (wsum_j + c_0)``, ``c_0`` the first band value of the prior's block when the prior is a
        Toeplitz ``BlockLO`` and 0 otherwise; 1 where that sum is 0."""
        s = self.F.wsum + (_prior_diagonal(self.prior, self.F) if self.prior is not None else 0.0)
        jac = np.ones(self.na)
        np.divide(1.0, s, out=jac, where=s != 0)
        d_jac = D.f64(jac)
        na = self.na

        def mult(r):
            x = D.f64(r)
            if x.numel() != na:
                raise lp.ShapeError("vector has %d entries, expected %d" % (x.numel(), na))
            out = D.empty(na)
            _hip.call("cm2_xmy", na, D.ptr(d_jac), D.ptr(x), D.ptr(out), D.stream())
            return D.like_input(out, r)

        return L._DeviceOp(na, na, mult, symmetric=True)

    # -- the map and the cleaned stream ------------------------------------------------
    def _check_da(self, d, a):
        _check_tod("d", d, self.nt)
        if np.ndim(a) != 1 or np.shape(a)[0] != self.na:
            raise ValueError("a must hold the %d offsets, got shape %r" % (self.na, tuple(np.shape(a))))
        D.require_gpu()

    def map(self, d, a):
        """``m = M P^T W (d0 - F a)``: the binned map of the destriped stream, of ``d``'s kind."""
        self._check_da(d, a)
        x, ad = D.f64(d), D.f64(a)
        t1, _ = self._time_scratch()
        _hip.call("cm2_offsets_residual", self.F._f.h, D.ptr(x), D.ptr(ad), 1, D.ptr(t1), D.stream())
        out = D.empty(self.nmap)
        self._binned(t1, out)
        return D.like_input(out, d)

    def cleaned(self, d, a):
        """``d - F a`` on the valid samples and 0 on the flagged ones, of ``d``'s kind."""
        self._check_da(d, a)
        x, ad = D.f64(d), D.f64(a)
        out = D.empty(self.nt)
        _hip.call("cm2_offsets_residual", self.F._f.h, D.ptr(x), D.ptr(ad), 0, D.ptr(out), D.stream())
        return D.like_input(out, d)


def solve_destriped(P, blocksize, baseline_length, d, Mbd, weights=None, prior=None, rtol=1e-6, maxiter=None,
                    x0=None, callback=None):
    """
    ``(m, a, info, op)``: the destriped map of ``d``, the baseline offsets, cg's ``info`` (0: converged to
    ``rtol |b|``) and the :class:`DestriperNormalLO` that was solved, by :func:`cosmomap2_amd.cg` with the Jacobi
    preconditioner.  ``op.iterations`` is cg's iteration count, ``op.F`` the :class:`OffsetsLO`.  ``prior`` is any
    symmetric operator on the ``na`` offsets (checked against ``na`` once it is known), typically
    ``BlockLO(op.F.baselines_per_block, bands, offdiag=True)``.  ``x0`` starts the offsets; ``callback`` receives
    cg's iterate.  ``m`` and ``a`` are of ``d``'s kind.
    """
    from ..solvers import cg
    _, _, _, per_block = _check_offsets_args(P, blocksize, baseline_length, weights)
    na = int(sum(per_block))
    _check_tod("d", d, int(P.nrows))
    _check_mbd(P, Mbd)
    _check_prior(prior, na)
    rtol = _check_rtol(rtol)
    if maxiter is not None and _int("maxiter", maxiter) < 1:
        raise ValueError("maxiter=%d < 1" % maxiter)
    if x0 is not None and (np.ndim(x0) != 1 or np.shape(x0)[0] != na):
        raise ValueError("x0 must hold the %d offsets, got shape %r" % (na, tuple(np.shape(x0))))
    if callback is not None and not callable(callback):
        raise ValueError("callback must be callable, got %r" % (callback,))
    F = OffsetsLO(P, blocksize, baseline_length, weights)
    op = DestriperNormalLO(P, F, Mbd, prior)
    dd = D.f64(d)
    b = D.f64(op.rhs(dd))
    its = []

    def count(ak):
        its.append(1)
        if callback is not None:
            callback(ak)

    a, info = cg(op, b, x0=None if x0 is None else D.f64(x0), M=op.preconditioner(), rtol=rtol, maxiter=maxiter,
                 callback=count)
    op.iterations = len(its)
    m = op.map(dd, a)
    return D.like_input(m, d), D.like_input(a, d), info, op
