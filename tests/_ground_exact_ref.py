"""
The order-independent ground-bin sums of include/cosmomap2.h (f2b, cm2_ground_sums_apply) restated with NumPy and
Python integers, and the inputs the tests share.

A sample counts when 0 <= g < nbins.  M = the largest bit pattern of |v| over the counted samples;
e = (M >> 52) - 1023.  A sample is cut into three limbs of trunc(v 2^(95-e)) in float64 (limbs()); the limbs of a bin
are added as Python integers, S = L0 2^64 + L1 2^32 + L2, and S 2^(e-95) is rounded to float64 once, through
Fraction (int / int true division is correctly rounded, ties to even).
"""
import math
from fractions import Fraction

import numpy as np

KINDS = ("normal", "wide", "cancel", "big", "tiny", "zeros")
ABS_MASK = 0x7FFFFFFFFFFFFFFF
INF_BITS = 0x7FF0000000000000
LDS_BINS = 2048                      # gsum::kLdsBins of cm2_ground_exact_policy.h
SHAPES = ((1, 1), (255, 3), (16385, 257), (70000, 2048), (70000, 2049), (100001, 8192), (70000, 8193))


def counted(g, nbins):
    g = np.asarray(g)
    return (g >= 0) & (g < nbins)


def scale_word(g, v, nbins):
    """M: the largest bit pattern of |v| over the counted samples (0 when there is none)"""
    u = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)[counted(g, nbins)] & np.uint64(ABS_MASK)
    return int(u.max()) if u.size else 0


def exponent(M):
    return (M >> 52) - 1023


def limbs(v, e):
    """-> l0, l1, l2 (int64 arrays): the recipe of the device, every step exact in float64"""
    v = np.asarray(v, dtype=np.float64)
    y0 = np.ldexp(v, 31 - e)
    t0 = np.trunc(y0)
    y1 = np.ldexp(y0 - t0, 32)
    t1 = np.trunc(y1)
    t2 = np.trunc(np.ldexp(y1 - t1, 32))
    return t0.astype(np.int64), t1.astype(np.int64), t2.astype(np.int64)


def limbs_without_l2(v, e):
    """a deliberately wrong variant: the last 32 bits are dropped"""
    l0, l1, l2 = limbs(v, e)
    return l0, l1, np.zeros_like(l2)


def truncated(v, e):
    """trunc(v 2^(95-e)) of every sample as Python integers, in exact rational arithmetic"""
    s = Fraction(2) ** (95 - e)
    return [math.trunc(Fraction(float(x)) * s) for x in np.asarray(v, dtype=np.float64)]


def joined(l0, l1, l2):
    return [(a << 64) + (b << 32) + c for a, b, c in zip(l0.tolist(), l1.tolist(), l2.tolist())]


def integer_sums(g, v, nbins, split=limbs):
    """-> (M, [S_b]): the scale word and the integer of every bin (None where M is 0, Inf or NaN)"""
    g, v = np.asarray(g), np.asarray(v, dtype=np.float64)
    M = scale_word(g, v, nbins)
    if M == 0 or M >= INF_BITS:
        return M, None
    ok = counted(g, nbins)
    S = [0] * nbins
    for b, t in zip(g[ok].tolist(), joined(*split(v[ok], exponent(M)))):
        S[b] += t
    return M, S


def exact_sums(g, v, nbins, split=limbs):
    M, S = integer_sums(g, v, nbins, split)
    if S is None:
        return np.zeros(nbins) if M == 0 else np.full(nbins, np.nan)
    e = exponent(M)
    scale = Fraction(2) ** (e - 95)
    return np.array([float(s * scale) for s in S], dtype=np.float64)


# --------------------------------------------------------------------- inputs ----
def labels(rng, nt, nbins, beyond=False):
    """labels in [-1, nbins), the last bin hit by the last sample; beyond: also labels a caller of the C ABI may
    pass and the kernels must skip (nbins, nbins + 5, the largest int32, -7)"""
    g = rng.integers(-1, nbins, size=nt).astype(np.int32)
    if beyond and nt >= 16:
        g[rng.choice(nt - 1, size=4, replace=False)] = (nbins, nbins + 5, 2 ** 31 - 1, -7)
    g[-1] = nbins - 1
    return g


def case(kind, nt, nbins, beyond=False):
    """-> g (int32), v (float64) of one of KINDS; the same arrays for the same arguments"""
    rng = np.random.default_rng([KINDS.index(kind), nt, nbins, int(beyond)])
    g = labels(rng, nt, nbins, beyond)
    x = rng.standard_normal(nt) + 0.5
    if kind == "normal":
        v = x
    elif kind == "wide":             # every sample scaled by 2^-k, k in 0..129: all three limbs and the truncation
        v = np.ldexp(x, -rng.integers(0, 130, size=nt))
    elif kind == "cancel":           # +x, -x and 2^-70 z in the same bins
        n = nt // 3
        v = np.concatenate([x[:n], -x[:n], np.ldexp(x[2 * n:], -70)])
        g[n:2 * n] = g[:n]
        g[2 * n:3 * n] = g[:n]
        p = rng.permutation(nt)
        g, v = g[p], v[p]
        g[-1] = nbins - 1
    elif kind == "big":
        v = np.ldexp(x, 600)
    elif kind == "tiny":
        v = np.ldexp(x, -700)
    elif kind == "zeros":
        v = np.where(rng.random(nt) < 0.5, 0.0, -0.0)
    else:
        raise ValueError(kind)
    return g, np.ascontiguousarray(v, dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
