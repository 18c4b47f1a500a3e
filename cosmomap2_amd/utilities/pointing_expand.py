"""
From telescope attitude to the solver's inputs, in HBM: one boresight quaternion per time sample and one offset
quaternion per detector are expanded to the HEALPix pixel and ``(cos 2 phi, sin 2 phi)`` of every detector sample
(``cm2_pointing_expand`` in ``include/cosmomap2.h`` has the definition, operation by operation).

    pixs, cos2, sin2 = expand_pointing(boresight, detquats, nside, hwp=chi)          # device tensors, detector-major
    ces = ProcessTimeSamples(pixs, 12 * nside**2, pol=3, cos_sin=(cos2, sin2), w=w)
    P = SparseLO(ces.get_new_pixel[0], pixs.numel(), pixs, pol=3, angle_processed=ces)

Conventions.  Quaternions are ``(x, y, z, w)``, scalar last, Hamilton product, and rotate vectors as
``v' = q v q*``.  ``q = q_frame q_bore[i] q_det[k]`` takes the detector frame to the sky: ``R(q) z^`` is the line of
sight and ``R(q) x^`` the polarisation-sensitive direction.  The angle ``psi`` is in the COSMO convention (from the
local meridian pointing south, toward east); with a half-wave plate at angle ``chi``, ``phi = psi + 2 chi``.
``quat_from_angles(theta, phi, psi)`` builds the quaternion that points at colatitude ``theta``, longitude ``phi`` with
that ``psi``.
"""
import ctypes

import numpy as np

from .. import _hip
from .. import device as D

torch = D.torch

__all__ = ["expand_pointing", "quat_mult", "quat_from_angles"]

_DBLP = ctypes.POINTER(ctypes.c_double)
_MAX_NSIDE = 8192                            # 12 nside^2 < 2^31: the pixel is an int32
_DBL_MIN = np.finfo(np.float64).tiny


def quat_mult(p, q):
    """Hamilton product ``p q`` of quaternions ``(x, y, z, w)`` (arrays ``[..., 4]``, broadcast against each other),
    each component summed left to right as the library does."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    px, py, pz, pw = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    qx, qy, qz, qw = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([((pw * qx + px * qw) + py * qz) - pz * qy,
                     ((pw * qy - px * qz) + py * qw) + pz * qx,
                     ((pw * qz + px * qy) - py * qx) + pz * qw,
                     ((pw * qw - px * qx) - py * qy) - pz * qz], axis=-1)


def quat_from_angles(theta, phi, psi):
    """``Rz(phi) Ry(theta) Rz(psi)`` as quaternions ``[..., 4]``: the line of sight ``R z^`` has colatitude
    ``theta`` and longitude ``phi``, and the sensitive direction ``R x^`` makes the angle ``psi`` with the local
    meridian (from south toward east), which is what :func:`expand_pointing` returns for it."""
    theta, phi, psi = np.broadcast_arrays(np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64),
                                          np.asarray(psi, dtype=np.float64))
    zero = np.zeros_like(theta)

    def rz(a):
        return np.stack([zero, zero, np.sin(0.5 * a), np.cos(0.5 * a)], axis=-1)

    ry = np.stack([zero, np.sin(0.5 * theta), zero, np.cos(0.5 * theta)], axis=-1)
    return quat_mult(quat_mult(rz(phi), ry), rz(psi))


def _int(name, v):
    try:
        i = int(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be an integer, got %r" % (name, v))
    if i != v:
        raise ValueError("%s must be an integer, got %r" % (name, v))
    return i


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _check_unit_able(name, q):
    """A host quaternion table whose rows the library could not normalise is refused here, with the row."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    bad = np.flatnonzero(~((n2 >= _DBL_MIN) & (n2 < np.inf)))
    if bad.size:
        raise ValueError("%s %d is %r: it cannot be normalised" % (name, int(bad[0]), q[bad[0]].tolist()))


def expand_pointing(boresight, detquats, nside, nest=False, hwp=None, flags=None, frame=None, pol=3, out=None):
    """
    ``(pixs, cos2phi, sin2phi)`` of every detector sample, in HBM: ``int32`` and two ``float64`` tensors of length
    ``ndet * ns``, detector-major (sample ``i`` of detector ``k`` at ``k * ns + i``).  The matching noise-block layout
    for ``BlockLO`` and ``solve_destriped`` is ``blocksize = [ns] * ndet``: one block per detector.

    ``boresight`` ``[ns, 4]`` and ``detquats`` ``[ndet, 4]`` (detector frame -> boresight frame) are quaternions
    ``(x, y, z, w)``; ``frame`` (4 numbers) is multiplied in front of every boresight quaternion, for a change of sky
    coordinates.  ``hwp`` ``[ns]`` is the plate angle in radians, ``flags`` ``[ns]`` marks samples to drop (non-zero).
    Inputs may be NumPy arrays or device tensors.  ``nside`` is a power of two up to 8192; ``nest`` selects NESTED
    ordering.  ``pol=1`` returns ``(pixs, None, None)``, allocates no angle arrays and does not read ``hwp``.  ``out=(pixs, cos2, sin2)``
    (``(pixs, None, None)`` for ``pol=1``) writes into given device tensors and returns them.

    A flagged sample, one whose boresight quaternion has a component that is not finite, or one whose quaternion is
    zero gets ``pix = -1, cos = 1, sin = 0``: the flag convention of ``SparseLO``, the tile plan and the gap index.
    Every argument is checked before the GPU is touched (``ValueError``); without a GPU a valid call raises
    ``HipError``.
    """
    n = _int("nside", nside)
    if n < 1 or n > _MAX_NSIDE or n & (n - 1):
        raise ValueError("nside=%d is not a power of two in [1, %d]" % (n, _MAX_NSIDE))
    if pol not in (1, 2, 3):
        raise ValueError("pol=%r is not 1, 2 or 3" % (pol,))
    bs, ds = _shape(boresight), _shape(detquats)
    if len(bs) != 2 or bs[1] != 4:
        raise ValueError("boresight must have shape [ns, 4], got %r" % (bs,))
    if len(ds) != 2 or ds[1] != 4 or ds[0] < 1:
        raise ValueError("detquats must have shape [ndet, 4] with ndet >= 1, got %r" % (ds,))
    ns, ndet = int(bs[0]), int(ds[0])
    for name, a in (("hwp", hwp), ("flags", flags)):
        if a is not None and _shape(a) != (ns,):
            raise ValueError("%s must have shape [ns] = [%d], got %r" % (name, ns, _shape(a)))
    h_frame = None
    if frame is not None:
        try:
            h_frame = np.ascontiguousarray(D.to_host(frame) if D.is_tensor(frame) else frame, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("frame must hold 4 numbers, got %r" % (frame,))
        if h_frame.shape != (4,):
            raise ValueError("frame must hold 4 numbers, got shape %r" % (h_frame.shape,))
        _check_unit_able("frame quaternion", h_frame)
    if not D.is_tensor(detquats):
        _check_unit_able("detector quaternion", detquats)
    want = (True, pol > 1, pol > 1)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise ValueError("out must be (pixs, cos2, sin2), got %r" % (type(out),))
        for name, t, dt, need in zip(("pixs", "cos2", "sin2"), out, ("int32", "float64", "float64"), want):
            if not need:
                if t is not None:
                    raise ValueError("out: %s must be None for pol=1" % name)
                continue
            if not D.is_dev(t) or str(t.dtype) != "torch." + dt or not t.is_contiguous() or \
                    t.numel() != ndet * ns:
                raise ValueError("out: %s must be a contiguous %s device tensor of %d elements, got %r"
                                 % (name, dt, ndet * ns, None if t is None else (type(t).__name__, _shape(t))))
    D.require_gpu()
    bore = D.f64(boresight)
    if bore.data_ptr() % 16:
        bore = bore.clone()
    det = D.f64(detquats)
    d_hwp = None if hwp is None or pol == 1 else D.f64(hwp)
    d_flags = None
    if flags is not None:
        d_flags = D.to_dev(flags)
        d_flags = (d_flags != 0).to(torch.uint8).contiguous()
    if out is not None:
        pixs, cos2, sin2 = out
    else:
        pixs = D.empty(ndet * ns, torch.int32)
        cos2, sin2 = (D.empty(ndet * ns), D.empty(ndet * ns)) if pol > 1 else (None, None)
    try:
        _hip.call("cm2_pointing_expand", ns, ndet, D.ptr(bore), D.ptr(det),
                  None if h_frame is None else h_frame.ctypes.data_as(_DBLP), D.ptr(d_hwp), D.ptr(d_flags), n,
                  1 if nest else 0, D.ptr(pixs), D.ptr(cos2), D.ptr(sin2), D.stream())
    except _hip.HipError as e:
        if e.status == _hip.ERR_ARGUMENT:              # the arguments were checked above: a detector table in HBM
            raise ValueError(str(e)) from None
        raise
    return pixs, cos2, sin2
