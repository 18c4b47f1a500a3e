"""
The demodulator restated in NumPy from its definition (include/cosmomap2.h, f2h), rule by rule and without the
kernel's method: the loop runs over the taps k in ascending order and NumPy over the outputs of a block, so every
output still adds its own included terms one after the other, each product and each addition rounded once, and an
excluded term is skipped (np.where keeps the chain as it was), not added as a zero.  Also the shared cases of
tests/test_demod_cpu.py and tests/test_gpu_demod.py, and the default taps restated.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import _glitch_ref as G

FULL, PARTIAL, REJECTED = range(3)
CLASSES = ("full", "partial", "rejected")
MAX_FACTOR, MAX_TAPS = 64, 1025
# the layout constants of cm2_demod_policy.h
MAX_UNIT, THREADS, ROUNDS = 2048, 256, 8
TWO53 = 9007199254740992.0                     # 2^53: TWO53 + 1 == TWO53

bits, flagged, edges = G.bits, G.flagged, G.edges


def per_unit(D):
    return MAX_UNIT // D


def unit_len(D):
    return per_unit(D) * D


def rounds(D):
    return -(-per_unit(D) // THREADS)


def slots(n):
    return (n - 1) + ((n - 1) >> 5) + 1


def lds_bytes(D, L, carrier=True):
    n = slots((per_unit(D) - 1) * D + L)
    return n * 8 * (3 if carrier else 1) + (n + 7) // 8 * 8


def same_bits(a, b):
    """bit for bit; positions where both sides are NaN count as equal (the sign of a generated NaN differs between
    hosts)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------ the restatement ----
def default_taps(D, L=None, cutoff=None):
    """lowpass_taps restated: a sinc under a Hamming window, symmetrised, divided by its fsum"""
    L = 16 * D + 1 if L is None else L
    fc = 0.4 / D if cutoff is None else cutoff
    c = (L - 1) // 2
    k = np.arange(L, dtype=np.float64) - c
    h = 2.0 * fc * np.sinc(2.0 * fc * k) * (0.54 + 0.46 * np.cos(np.pi * k / (c + 1)))
    h = 0.5 * (h + h[::-1])
    return h / math.fsum(h)


def tap_sum(h):
    w = 0.0
    for x in h:
        w = w + float(x)
    return w


def usable(d, flags=None):
    """rule 1"""
    return ~flagged(flags, d.size) & np.isfinite(d)


def out_sizes(sizes, D):
    return [-(-int(s) // D) for s in sizes]


def run(d, sizes, D, h, flags=None, cosv=None, sinv=None, min_weight=0.5):
    """rules 1-6: SimpleNamespace(T, Q, U, cls, counts, W, n); Q and U None without a carrier.  W and n (the included
    terms) are kept for the tests of the cases."""
    d, h = np.asarray(d, dtype=np.float64), np.asarray(h, dtype=np.float64)
    L = h.size
    c = (L - 1) // 2
    carrier = cosv is not None
    use, e = usable(d, flags), edges(sizes)
    wfull = tap_sum(h)
    thr = float(min_weight) * wfull
    M = sum(out_sizes(sizes, D))
    T, Q, U, W = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
    cls, nin = np.zeros(M, dtype=np.uint8), np.zeros(M, dtype=np.int64)
    counts = np.zeros((len(sizes), 3), dtype=np.int64)
    o0 = 0
    with np.errstate(all="ignore"):
        for b, (b0, b1) in enumerate(zip(e[:-1], e[1:])):
            n = int(b1 - b0)
            m = -(-n // D)
            x, u = d[b0:b1], use[b0:b1]
            if carrier:                                            # the carrier is used only at usable samples
                xc = np.where(u, x * np.where(u, cosv[b0:b1], 0.0), 0.0)
                xs = np.where(u, x * np.where(u, sinv[b0:b1], 0.0), 0.0)
            j = np.arange(m, dtype=np.int64)
            sT, sQ, sU, w, cnt = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.int64)
            for k in range(L):                                     # rule 3: ascending k, one chain per sum
                i = j * D - c + k
                ii = np.clip(i, 0, n - 1)
                inc = (i >= 0) & (i < n) & u[ii]
                sT = np.where(inc, sT + h[k] * x[ii], sT)
                if carrier:
                    sQ = np.where(inc, sQ + h[k] * xc[ii], sQ)
                    sU = np.where(inc, sU + h[k] * xs[ii], sU)
                w = np.where(inc, w + h[k], w)
                cnt += inc
            ok = w >= thr                                          # rule 4 (False for a NaN)
            T[o0:o0 + m] = np.where(ok, sT / w, 0.0)
            if carrier:
                Q[o0:o0 + m] = np.where(ok, 2.0 * (sQ / w), 0.0)
                U[o0:o0 + m] = np.where(ok, 2.0 * (sU / w), 0.0)
            k_ = np.where(cnt == L, FULL, np.where(ok, PARTIAL, REJECTED)).astype(np.uint8)      # rule 5
            cls[o0:o0 + m], W[o0:o0 + m], nin[o0:o0 + m] = k_, w, cnt
            counts[b] = np.bincount(k_, minlength=3)
            o0 += m
    return SimpleNamespace(T=T, Q=Q if carrier else None, U=U if carrier else None, cls=cls, counts=counts, W=W,
                           n=nin, wfull=wfull, M=M)


def pick(pix, cls, sizes, D, drop_from):
    e, out = edges(sizes), []
    for b0, b1 in zip(e[:-1], e[1:]):
        out.append(np.asarray(pix[b0:b1:D], dtype=np.int32))
    p = np.concatenate(out)
    return np.where((cls >= drop_from) | (p < 0), -1, p).astype(np.int32)


def response(h, f):
    """|H(f)|, the DFT of the taps at f cycles per sample"""
    k = np.arange(h.size) - (h.size - 1) // 2
    return abs(np.sum(h * np.exp(-2j * np.pi * f * k)))


# ----------------------------------------------------------------------- the shared cases ----
def _case(name, sizes, D, h, d, flags=None, cosv=None, sinv=None, min_weight=0.5):
    sizes = [int(s) for s in sizes]
    assert sum(sizes) == d.size and (flags is None or flags.size == d.size)
    return SimpleNamespace(name=name, sizes=sizes, D=D, h=np.asarray(h, dtype=np.float64), d=d, flags=flags, cosv=cosv,
                           sinv=sinv, min_weight=min_weight)


def _stream(rng, nt, flag_share=0.03):
    d = rng.standard_normal(nt) + 3.0
    ph = 2.0 * np.pi * 0.1371 * np.arange(nt) + rng.uniform(0, 6.0)
    pix = rng.integers(0, 1000, nt).astype(np.int32)
    pix[rng.random(nt) < flag_share] = -1
    return d, pix, np.cos(ph), np.sin(ph)


# (D, L): D = 1 (a plain FIR), 2, 8, 64; L = 1 (a plain pick), 3, 2 D + 1, 1025; L = 1025 at D = 1 and at D = 64;
# 3 and 7: factors that do not divide 2048
SIZE_SHAPES = [(1, 1), (1, 3), (2, 1), (2, 3), (2, 5), (8, 1), (8, 3), (8, 17), (64, 1), (64, 3), (64, 129), (1, 1025),
               (64, 1025), (2, 1025), (8, 1025), (3, 7), (7, 15), (4, 65)]


def size_list(D, L):
    """blocks of 1, c, c + 1, D - 1, D, D + 1, unit - 1, unit, unit + 1 and unit + c samples (those of them >= 1), and
    one of two units and a bit that D does not divide where it can"""
    c, unit = (L - 1) // 2, unit_len(D)
    return [s for s in (1, c, c + 1, D - 1, D, D + 1, unit - 1, unit, unit + 1, unit + c, 2 * unit + D // 2 + 1)
            if s >= 1]


def positive_taps(L, seed):
    """taps of one sign, not symmetric: an order of the sum other than the ascending one shows"""
    return np.random.default_rng(seed).uniform(0.2, 1.0, L)


def _sizes_case(D, L):
    rng = np.random.default_rng(1000 * D + L)
    sizes = size_list(D, L)
    d, pix, co, si = _stream(rng, sum(sizes))
    h = default_taps(D, L) if L > 1 and (D, L) not in ((3, 7), (7, 15), (8, 17)) else positive_taps(L, L + D)
    return _case("sizes_D%d_L%d" % (D, L), sizes, D, h, d, pix, co, si)


def _special_cases():
    out = {}
    rng = np.random.default_rng(77)
    # a flagged run longer than L: class 2 and 0.0; shorter ones: partial
    D, L = 4, 9
    sizes = [3000, 1000]
    d, pix, co, si = _stream(rng, 4000, 0.0)
    pix[500:530] = -1
    pix[1197:1199] = -1
    pix[2990:3010] = -1                                            # across the block edge
    out["flag_run"] = _case("flag_run", sizes, D, default_taps(D, L), d, pix, co, si)
    # W exactly on min_weight Wfull, and one tap below: taps that add exactly, Wfull = 3
    h = np.array([0.25, 0.25, 0.5, 1.0, 0.5, 0.25, 0.25])
    d, pix, co, si = _stream(rng, 400, 0.0)
    f = np.zeros(400, dtype=bool)
    f[[97, 98, 99, 102, 103]] = True                               # output 25 (centre 100) keeps 1 + 0.5: W = 1.5
    f[[197, 198, 199, 201, 202]] = True                            # output 50 keeps 1 + 0.25: W = 1.25
    f[[297, 298, 299, 301]] = True                                 # output 75 keeps 1 + 0.25 + 0.25 = 1.5 again
    out["weight_edge"] = _case("weight_edge", [400], 4, h, d, f, co, si, 0.5)
    # min_weight = 1: one missing term rejects
    f = np.zeros(400, dtype=np.uint8)
    f[[50, 203]] = 7
    out["min_weight_1"] = _case("min_weight_1", [200, 200], 4, h, d.copy(), f, co, si, 1.0)
    # negative lobes: the partial W is <= 0
    h = np.array([-1.0, 0.5, 2.0, 0.5, -1.0])
    f = np.zeros(400, dtype=bool)
    f[100] = True                                                  # output 50 (D = 2): W = -1
    f[[199, 201]] = True                                           # output 100: W = 0
    f[[298, 302]] = True                                           # output 150: W = 3 > Wfull = 1
    out["negative_lobes"] = _case("negative_lobes", [400], 2, h, d.copy(), f, co, si, 0.5)
    # NaN and +-inf at block ends and at unit edges, a NaN carrier under a flagged sample and under a usable one
    D, L = 2, 5
    unit = unit_len(D)
    sizes = [unit + 50, 2 * unit + 1, 30]
    nt = sum(sizes)
    d, pix, co, si = _stream(rng, nt, 0.02)
    e = edges(sizes)
    for b0, b1 in zip(e[:-1], e[1:]):
        d[b0], d[b1 - 1] = np.nan, np.inf
    d[[unit - 1, unit, unit + 1]] = [np.inf, np.nan, -np.inf]
    d[e[1] + unit] = -np.inf
    d[e[1] + 2 * unit - 1] = np.nan
    pix[[300, 301]] = -1
    co[300], si[301] = np.nan, np.nan                              # under flagged samples: never read
    pix[600], co[600] = 5, np.nan                                  # under a usable one: Q is NaN there
    d[600] = 1.0
    out["nonfinite"] = _case("nonfinite", sizes, D, default_taps(D, L), d, pix, co, si)
    # +-1e308 pairs (a chain that overflows and one that cancels first) and subnormals
    d = np.ones(600)
    d[100:104] = [1e308, 1e308, -1e308, -1e308]
    d[300:304] = [1e308, -1e308, 1e308, -1e308]
    out["huge_pairs"] = _case("huge_pairs", [600], 1, np.ones(5), d, None, np.ones(600), -np.ones(600))
    d = rng.integers(-2000, 2000, 600).astype(np.float64) * 5e-324
    out["subnormals"] = _case("subnormals", [600], 2, [0.25, 0.5, 0.25], d, None, np.full(600, 0.5), np.full(600, -0.5))
    # 2^53, 1, -2^53 inside one window: ascending 0, descending 1
    d = np.zeros(200)
    d[99:102] = [TWO53, 1.0, -TWO53]
    d[149:152] = [-TWO53, TWO53, 1.0]
    out["chain_order"] = _case("chain_order", [200], 1, np.ones(3), d, None, np.ones(200), np.ones(200))
    # a unit with no unusable sample (W = Wfull from the create) next to units with a single one
    D, L = 8, 33
    unit = unit_len(D)
    sizes = [4 * unit + 5]
    d, pix, co, si = _stream(rng, sizes[0], 0.0)
    pix[unit // 2] = -1                                            # unit 0 (which also has its block edge)
    pix[2 * unit + 700] = -1                                       # unit 2; unit 1 stages nothing unusable
    d[3 * unit + 16 + 100] = np.nan                                # unit 3, beyond the reach of unit 2's windows
    out["shortcut"] = _case("shortcut", sizes, D, default_taps(D, L) + 1e-3, d, pix, co, si)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for D, L in SIZE_SHAPES:
        c = _sizes_case(D, L)
        out[c.name] = c
    out.update(_special_cases())
    return out


SIZE_CASES = ["sizes_D%d_L%d" % s for s in SIZE_SHAPES]
SPECIAL_CASES = ["flag_run", "weight_edge", "min_weight_1", "negative_lobes", "nonfinite", "huge_pairs", "subnormals",
                 "chain_order", "shortcut"]
CASES = SIZE_CASES + SPECIAL_CASES


def case(name):
    return cases()[name]


def variant(c, carrier=True, flags="own"):
    """the case with or without its carrier, and its flags as they are ("own"), as bool, as uint8 bytes, or none"""
    f = c.flags
    if flags == "none" or f is None:
        f = None
    elif flags == "bool":
        f = flagged(f, f.size)
    elif flags == "uint8":
        f = flagged(f, f.size).astype(np.uint8) * 3
    return SimpleNamespace(name=c.name, sizes=c.sizes, D=c.D, h=c.h, d=c.d, flags=f, min_weight=c.min_weight,
                           cosv=c.cosv if carrier else None, sinv=c.sinv if carrier else None)


@functools.lru_cache(maxsize=None)
def expected(name, carrier=True, flags="own"):
    c = variant(case(name), carrier, flags)
    return run(c.d, c.sizes, c.D, c.h, c.flags, c.cosv, c.sinv, c.min_weight)


# --------------------------------------------------------------------- detection quality ----
QUALITY = [(8, 0.13), (4, 0.21), (16, 0.08), (8, 0.07)]            # (D, f_m)
QUALITY_IQU = (1.0, 0.1, -0.05)
QUALITY_N = 4000


def quality_stream(fm, n=QUALITY_N, phase=0.3):
    I, Q, U = QUALITY_IQU
    ph = 2.0 * np.pi * fm * np.arange(n) + phase
    co, si = np.cos(ph), np.sin(ph)
    return I + Q * co + U * si, co, si


def quality_bounds(h, fm):
    """(bound on |T - I|, bound on |Q^ - Q| and |U^ - U|) for outputs whose window lies inside the block"""
    I, Q, U = QUALITY_IQU
    H1, H2 = response(h, fm), response(h, 2.0 * fm)
    return (abs(Q) + abs(U)) * H1 + 1e-12, 2.0 * abs(I) * H1 + (abs(Q) + abs(U)) * H2 + 1e-12
