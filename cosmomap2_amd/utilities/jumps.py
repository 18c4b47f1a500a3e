"""
Baseline jumps of the time streams, found and removed on the GPU: a step in a detector's level (a flux jump of the
readout, a relock) that stays for the rest of the stream.  The glitch flagger cannot see one -- a running median keeps
an edge -- and a few of them put hundreds of times the clean stream's power into the lowest frequencies, so this
stage sits between the glitch flags and the filters (the reference has no counterpart).

    jc = JumpCorrector(blocksize, half_window=64)              # blocksize as BlockLO takes it
    d_out, jcls, info = jc.run(d, flags=pixs, classes=cls)     # corrected stream and class bytes, in HBM
    apply_flags(pixs, jcls)                                    # pixs[jcls != 0] = -1
    t, noeval = jc.statistic(d, flags=pixs)                    # the step statistic of every position
    sigma     = jc.scale(t, noeval)                            # its robust scale per block
    table     = jc.find(t, noeval, sigma, nsigma=6.0)          # positions, heights, accumulated offsets
    d_out, jcls, counts = jc.correct(d, table, radius=4)
    d_out, jcls, info = correct_jumps(d, blocksize, flags=pixs)   # the same as run, in one call

**Definition** (include/cosmomap2.h, f2f, has it in full).  Everything is cut at the block boundaries.  A sample is
*usable* when it is not flagged, finite, and has class 0 in ``classes``.  ``t_i`` is the mean of the usable samples
``i .. i+w-1`` minus the mean of the usable samples ``i-w .. i-1`` (``w = half_window``; sums in ascending order),
evaluable where both windows lie in the block and hold ``min_count`` usable samples.  ``sigma_b = 1.4826 x`` the lower
median of ``|t|`` over the evaluable positions of block ``b`` (``inf`` with fewer than 3).  A position with
``|t| > nsigma sigma_b`` that no evaluable position within ``w`` exceeds (or equals, further left) is a jump of height
``t``.  The stream loses the accumulated heights of the jumps of its block at or before each sample.  Classes, the
first that applies: the byte of ``classes`` if non-zero, ``jump``, ``near`` (a jump of the block within ``radius``),
``clean``.

**Iteration.**  A jump within ``w`` of a larger one shows only after the larger one is removed, so :meth:`run` repeats
the pass on its own output, with its own classes, until a pass finds no jump or ``iterations`` passes have run.

Arrays or tensors are taken as :func:`flag_glitches` takes them.  Every result has the bits the definition gives.
Every argument is checked before the GPU is touched (``ValueError``); without a GPU a valid call raises ``HipError``.
On several GPUs each rank corrects its own blocks: blocks are independent.
"""
import collections

import numpy as np

from .. import _hip
from .. import device as D
from ._stream_args import (_BlockStage, _StageHandle, _check_dev, _check_iterations, _check_nsigma, _check_out,
                           _check_sigma, _int)

__all__ = ["JumpCorrector", "correct_jumps", "JUMP_CLASSES"]

JUMP_CLASSES = ("clean", "jump", "near")
CLEAN, AT, NEAR = range(3)
MAX_WINDOW = 256               # CM2_JUMP_MAX_WINDOW
MAX_RADIUS = 256               # CM2_JUMP_MAX_RADIUS

JumpTable = collections.namedtuple("JumpTable", "positions heights offsets njumps total capacity counts_dev")
JumpTable.__doc__ = """What :meth:`JumpCorrector.find` returns: ``positions`` (int64), ``heights`` and ``offsets``
(the accumulated heights within the block) as tensors in HBM of ``capacity`` entries, the first ``total`` of them
valid; ``njumps`` the jumps per block (NumPy); ``counts_dev`` the same with ``total`` last, in HBM."""


def _check_window(w):
    w = _int("half_window", w)
    if not 1 <= w <= MAX_WINDOW:
        raise ValueError("half_window=%d outside [1, %d]" % (w, MAX_WINDOW))
    return w


def _check_min_count(min_count, w):
    if min_count is None:
        return (w + 1) // 2
    min_count = _int("min_count", min_count)
    if not 1 <= min_count <= w:
        raise ValueError("min_count=%d outside [1, half_window=%d]" % (min_count, w))
    return min_count


def _check_radius(radius):
    radius = _int("radius", radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError("radius=%d outside [0, %d]" % (radius, MAX_RADIUS))
    return radius


def _check_capacity(capacity):
    capacity = _int("capacity", capacity)
    if capacity < 1:
        raise ValueError("capacity=%d < 1" % capacity)
    return capacity


class _Jump(_StageHandle):
    """Owns a cm2_jump handle (block tables, mark bytes, the select's storage and the scale's cm2_glitch)."""
    prefix, info_names = "jump", ("nt", "nblocks", "half_window", "tile", "lds_bytes", "bytes")


class JumpCorrector(_BlockStage):
    """
    Finds and removes the baseline jumps of time streams cut into the noise blocks ``blocksize`` (BlockLO's
    convention: an int that divides the stream, or the list of block sizes), comparing the means of the
    ``half_window`` samples on either side of every position, ``1 <= half_window <= 256``.  The object owns, per
    stream length it has met, the block tables, one byte per sample and the scale's histograms (8 KB per block).
    """
    handle_class, window, prev_name = _Jump, "half_window", "classes"
    noun, histograms = "jump corrector", "the scale's histograms"

    def __init__(self, blocksize, half_window=64):
        self.half_window = _check_window(half_window)
        _BlockStage.__init__(self, blocksize)

    # ---- checks (no GPU) ----
    def _check_stat(self, t, noeval):
        if not D.is_tensor(t):
            raise ValueError("t must be the tensor that statistic() returned")
        nt = int(t.numel())
        if nt < 1:
            raise ValueError("t has no samples")
        _check_dev("t", t, nt, "float64")
        _check_dev("noeval", noeval, nt, "uint8")
        return nt, self._sizes(nt)

    # ---- device ----
    def info(self, nt):
        """The library's description of the handle for streams of ``nt`` samples (tile, LDS bytes, bytes owned)."""
        return _BlockStage.info(self, nt)

    def _stat(self, g, x, f, kind, prev, min_count, t, noeval):
        _hip.call("cm2_jump_stat", g.h, D.ptr(x), D.ptr(f), kind, D.ptr(prev), min_count, D.ptr(t), D.ptr(noeval),
                  D.stream())

    def _scale(self, g, t, noeval, nblocks):
        sigma = D.empty(nblocks)
        _hip.call("cm2_jump_scale", g.h, D.ptr(t), D.ptr(noeval), D.ptr(sigma), D.stream())
        return sigma

    def _find(self, g, t, noeval, sigma, nsigma, capacity, nblocks, bufs=None):
        tt = D.torch
        cap = min(capacity, int(t.numel()))                    # no stream has more jumps than samples
        pos, heights, offsets, njumps = bufs or (D.empty(cap, tt.int64), D.empty(cap), D.empty(cap),
                                                 D.empty(nblocks + 1, tt.int64))
        _hip.call("cm2_jump_find", g.h, D.ptr(t), D.ptr(noeval), D.ptr(sigma), nsigma, cap, D.ptr(pos),
                  D.ptr(heights), D.ptr(offsets), D.ptr(njumps), D.stream())
        counts = D.to_host(njumps)
        total = int(counts[-1])
        if total > cap:
            raise RuntimeError("%d jumps found, the table holds capacity=%d: raise nsigma or the capacity (jumps per "
                               "block: at most %d)" % (total, cap, int(counts[:-1].max())))
        return JumpTable(pos, heights, offsets, counts[:-1].copy(), total, cap, njumps)

    def _correct(self, g, x, prev, table, radius, out, cls, counts):
        _hip.call("cm2_jump_correct", g.h, D.ptr(x), D.ptr(prev), D.ptr(table.positions), D.ptr(table.offsets),
                  D.ptr(table.counts_dev), table.capacity, radius, D.ptr(out), D.ptr(cls), D.ptr(counts), D.stream())

    @staticmethod
    def _out(out, x, d):
        """the tensor the corrected stream is written to: ``out`` in HBM, the upload of a NumPy ``d``, or a new one"""
        if D.is_tensor(out):
            return out
        return x if not D.is_tensor(d) else D.empty(x.numel())

    def statistic(self, d, flags=None, classes=None, min_count=None):
        """``(t, noeval)``: the step statistic (float64) and its not-evaluable bytes (uint8), tensors in HBM."""
        nt, sizes = self._check_stream(d, flags, classes)
        min_count = _check_min_count(min_count, self.half_window)
        D.require_gpu()
        f, kind = self._dev_flags(flags)
        prev = None if classes is None else D.to_dev(classes)
        t, noeval = D.empty(nt), D.empty(nt, D.torch.uint8)
        self._stat(self._handle(nt, sizes), D.f64(d), f, kind, prev, min_count, t, noeval)
        return t, noeval

    def scale(self, t, noeval):
        """``sigma`` per block (a float64 tensor in HBM): the robust scale of ``t`` over the evaluable positions."""
        nt, sizes = self._check_stat(t, noeval)
        D.require_gpu()
        return self._scale(self._handle(nt, sizes), t, noeval, len(sizes))

    def find(self, t, noeval, sigma, nsigma=6.0, capacity=1 << 20):
        """The :class:`JumpTable` of the jumps of ``t``; ``sigma`` one number or one per block (array or tensor).
        Raises ``RuntimeError`` when there are more jumps than ``capacity``."""
        nt, sizes = self._check_stat(t, noeval)
        nsigma, capacity = _check_nsigma(nsigma), _check_capacity(capacity)
        if not (D.is_tensor(sigma) and sigma.is_cuda):
            sigma = _check_sigma(sigma, len(sizes))
            if sigma is None:
                raise ValueError("sigma must be given: one number, or one per block")
        else:
            _check_dev("sigma", sigma, len(sizes), "float64")
        D.require_gpu()
        return self._find(self._handle(nt, sizes), t, noeval, D.f64(sigma), nsigma, capacity, len(sizes))

    def correct(self, d, table, classes=None, radius=4, out=None):
        """``(d_out, jcls, counts)``: the stream without the jumps of ``table``, the class bytes (uint8, in HBM) and
        ``counts`` ([nblocks, 3] int64: clean, jump, near; samples with a class in ``classes`` are in none).  ``out``
        as :meth:`run` takes it."""
        nt, sizes = self._check_stream(d, None, classes)
        radius = _check_radius(radius)
        _check_out(out, nt)
        if not isinstance(table, JumpTable):
            raise ValueError("table must be what find() returned")
        if len(table.njumps) != len(sizes):
            raise ValueError("the table is of %d blocks, the stream has %d" % (len(table.njumps), len(sizes)))
        D.require_gpu()
        tt = D.torch
        x = D.f64(d)
        prev = None if classes is None else D.to_dev(classes)
        o = self._out(out, x, d)
        cls, counts = D.empty(nt, tt.uint8), D.empty(3 * len(sizes), tt.int64)
        self._correct(self._handle(nt, sizes), x, prev, table, radius, o, cls, counts)
        return self._result(o, out), cls, D.to_host(counts).reshape(len(sizes), 3)

    @staticmethod
    def _head(x, n, dtype):
        """the first n entries of a table in HBM, on the host"""
        return D.to_host(x[:n].contiguous()).copy() if n else np.zeros(0, dtype=dtype)

    @staticmethod
    def _result(o, out):
        if isinstance(out, np.ndarray):
            out[:] = D.to_host(o)
            return out
        return o

    def run(self, d, flags=None, classes=None, min_count=None, nsigma=6.0, radius=4, iterations=3, sigma=None,
            capacity=1 << 20, out=None):
        """
        ``(d_out, jcls, info)``.  ``d_out``: the corrected stream, a float64 tensor in HBM (``out`` if that is a
        tensor in HBM, which may be ``d`` itself; a NumPy ``out`` is filled and returned).  ``jcls``: a uint8 tensor in
        HBM, the byte of ``classes`` where that is non-zero and ``JUMP_CLASSES`` elsewhere.  ``info``: ``positions``,
        ``heights`` and ``found_in_pass`` of every jump in the order found, ``counts`` ([nblocks, 3] int64 of the last
        pass: clean, jump, near), ``sigma`` (one array per pass), ``short_blocks`` (fewer than 3 evaluable positions
        in the last pass) and ``passes``.  ``sigma`` (one number, or one per block) replaces the robust scale of
        ``t``.  Raises ``RuntimeError``, before anything is corrected in that pass, when a pass finds more than
        ``capacity`` jumps.
        """
        nt, sizes = self._check_stream(d, flags, classes)
        min_count = _check_min_count(min_count, self.half_window)
        nsigma, radius, iterations = _check_nsigma(nsigma), _check_radius(radius), _check_iterations(iterations)
        given, capacity = _check_sigma(sigma, len(sizes)), _check_capacity(capacity)
        _check_out(out, nt)
        D.require_gpu()
        tt = D.torch
        nb = len(sizes)
        g = self._handle(nt, sizes)
        x = D.f64(d)
        f, kind = self._dev_flags(flags)
        o = self._out(out, x, d)
        t, noeval = D.empty(nt), D.empty(nt, tt.uint8)
        cls = [D.empty(nt, tt.uint8), D.empty(nt, tt.uint8)]       # prev and the new classes change places
        counts_dev = D.empty(3 * nb, tt.int64)
        cap = min(capacity, nt)
        bufs = (D.empty(cap, tt.int64), D.empty(cap), D.empty(cap), D.empty(nb + 1, tt.int64))
        sig = D.to_dev(given) if given is not None else None
        prev = None if classes is None else D.to_dev(classes)
        positions, heights, found, sigmas = [], [], [], []
        for k in range(iterations):
            self._stat(g, x, f, kind, prev, min_count, t, noeval)
            if given is None:
                sig = self._scale(g, t, noeval, nb)
            table = self._find(g, t, noeval, sig, nsigma, capacity, nb, bufs)
            self._correct(g, x, prev, table, radius, o, cls[k & 1], counts_dev)
            positions.append(self._head(table.positions, table.total, np.int64))
            heights.append(self._head(table.heights, table.total, np.float64))
            found.append(np.full(table.total, k, dtype=np.int64))
            sigmas.append(D.to_host(sig).copy())
            x, prev = o, cls[k & 1]
            if table.total == 0:
                break
        # the evaluable positions per block of the last pass: a running count on the device, read at the block ends
        running = tt.cumsum(noeval == 0, 0, dtype=tt.int32 if nt < 2 ** 31 else tt.int64)
        ends = D.to_dev(np.cumsum(sizes) - 1, tt.int64)
        e_b = np.diff(np.concatenate([[0], D.to_host(running[ends]).astype(np.int64)]))
        del running
        info = dict(positions=np.concatenate(positions), heights=np.concatenate(heights),
                    found_in_pass=np.concatenate(found), counts=D.to_host(counts_dev).reshape(nb, 3).copy(),
                    sigma=sigmas, short_blocks=np.flatnonzero(e_b < 3), passes=len(sigmas))
        return self._result(o, out), prev, info


def correct_jumps(d, blocksize, flags=None, classes=None, half_window=64, min_count=None, nsigma=6.0, radius=4,
                  iterations=3, sigma=None, capacity=1 << 20, out=None):
    """``JumpCorrector(blocksize, half_window).run(d, ...)`` for a single stream."""
    return JumpCorrector(blocksize, half_window).run(d, flags=flags, classes=classes, min_count=min_count,
                                                     nsigma=nsigma, radius=radius, iterations=iterations, sigma=sigma,
                                                     capacity=capacity, out=out)
