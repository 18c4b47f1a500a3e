"""
References, restatements and error bounds for the time-stream filter kernels
(csrc/cm2_filter.hip), and the cases the CPU and the GPU tests share.

Plain NumPy, no GPU, in the manner of tests/_vector_ref.py:

  * ``mean_ref``, ``poly_noflag_ref``, ``poly_flagged_ref`` -> ``(ref, S)`` per chunk in
    np.longdouble.  S is the same formula with every operand replaced by its absolute value and
    every subtraction by an addition:  |d_i| + sum_k |q_k(i)| sum_j |q_k(j)| |d_j|.
  * ``mean_f64``, ``poly_noflag_f64``, ``poly_flagged_f64``: float64 restatements in the kernel's
    order.  Lane l sums its samples j = l, l + 64, ... in sequence, the 64 lane sums go through
    the xor butterfly 32, 16, ..., 1, then come the Stieltjes recurrence of k_filter_setup,
    ortho_eval and the write pass of poly_body.  The library is built with -ffp-contract=off and
    the three chunk carriers (RegChunk<8>, RegChunk<32>, MemChunk) and LdsChunk visit a lane's
    samples in the same order, so these match the GPU bit for bit.
  * ``stream_ref`` / ``stream_f64``: the whole stream, zeros in every gap.
  * ``windows_plan`` / ``windows_f64``: the window planner of filter_windows_build, the
    workgroup -> window map of k_filter_windows, and the filter through them.

Acceptance, element by element: bit-equal to the restatement, or |got - ref| <= c 2^-53 S;
where S = 0 (gaps, kind-0 chunks, flagged samples of the fit) the result must be exactly 0.

The constants c.  Mean and no-flag fit, counted from the kernel source: a coefficient is
ceil(n / 64) lane terms (1 product or load + the adds) and 6 butterfly stages; the projection
adds K products; one final subtraction; + 2 for the second-order terms and the reference's own
roundings:  c = ceil(n / 64) + 6 + K + 1 + 2  (K = 1 for the mean: the division).
Flagged chunks: the loss of orthonormality of the float64 recurrence enters, which no operation
count gives.  It is measured: WORST_FLAGGED[order] is the largest |restatement - ref| / (2^-53 S)
over every flagged chunk of the cases below (tests/test_filter_ref_cpu.py re-measures it), and
c = that times 8 (the headroom between NumPy and the device that the vector-kernel tests showed
to be enough for equal formulas in a different rounding order), rounded up to a power of two.
"""
from types import SimpleNamespace

import numpy as np

import _vector_ref as V

LD, U53, _ld = V.LD, V.U53, V._ld
bits, assert_bit_equal = V.bits, V.assert_bit_equal

KWAVE = 64
WIN_LEN = 8192                       # kPermWin of cm2_tiles.h
REG_SMALL, REG_LARGE = 512, 2048     # kWave * kRegSmall, kWave * kRegLarge

MUTATIONS = ("drop_last", "j_le_n", "skip_stage", "kind_threshold", "table_neighbour",
             "flagged_written", "gap_not_zeroed", "beta_prev", "drop_window", "trailing_gap")


def _ceil(a, b):
    return -(-int(a) // int(b))


def pow2_at_least(r):
    p = 1
    while p < r:
        p <<= 1
    return p


# ----------------------------------------------------------------- acceptance ----
def excess(got, ref, S, c):
    """max over ALL elements of |got - ref| / (c 2^-53 S), c a number or one per element"""
    return V.excess(got, ref, _ld(S) * _ld(c), 1)


def assert_within(got, ref, S, c, what=""):
    e = excess(got, ref, S, c)
    assert e <= 1.0, "%s: |got - ref| is %.3g x the bound c 2^-53 S" % (what, e)
    return e


def c_mean(n):
    # ceil(n / 64) lane terms, 6 butterfly stages, sum / cnt, d - mean, + 2
    return _ceil(n, KWAVE) + 6 + 1 + 1 + 2


def c_noflag(n, K):
    # ceil(n / 64) lane terms (product + adds), 6 butterfly stages, K terms of the projection,
    # d - p, + 2
    return _ceil(n, KWAVE) + 6 + K + 1 + 2


# largest |poly_flagged_f64 - poly_flagged_ref| / (2^-53 S) over the flagged chunks of
# time_case(order) (both inputs) and of the tile layouts run at that order, rounded up to one
# decimal; test_filter_ref_cpu.py::test_flagged_constant_is_the_measured_one keeps it honest
#
# The large entries come from two kinds of chunk: unflagged samples in two clusters at the chunk's
# ends, and exactly K unflagged samples of a long chunk some of which lie close together (there
# the exact result is 0 and the kernel leaves up to 5e-14 S).  Two independent extended-precision
# routes to Q (the one below, and a Chebyshev basis with repeated Gram-Schmidt) agree to 0.02 on
# such chunks: the loss is the float64 three-term recurrence's own, not the reference's.
WORST_FLAGGED = {1: 2.4, 2: 65.2, 3: 42.8, 4: 37.7, 5: 46.7, 6: 463.7, 7: 219.0}


def c_flagged(order):
    return pow2_at_least(8.0 * WORST_FLAGGED[order])


# ------------------------------------------------- lane sums and the butterfly ----
def lane_allsum(terms, mut=None):
    """terms (n,) or (n, m), zero where a sample does not enter.  -> (64,) or (64, m): what each
    lane holds after wave_allsum (all the same, unless a stage is skipped)."""
    t = np.asarray(terms, dtype=np.float64)
    one = t.ndim == 1
    if one:
        t = t[:, None]
    n, m = t.shape
    U = _ceil(n, KWAVE)
    pad = np.zeros((U * KWAVE, m))
    pad[:n] = t
    pad = pad.reshape(U, KWAVE, m)
    acc = np.zeros((KWAVE, m))
    for u in range(U):                               # sum += term, j = lane + 64 u
        acc = acc + pad[u]
    lanes = np.arange(KWAVE)
    for off in (32, 16, 8, 4, 2, 1):                 # v += __shfl_xor(v, off)
        if mut == "skip_stage" and off == 4:
            continue
        acc = acc + acc[lanes ^ off]
    return acc[:, 0] if one else acc


def _sum_domain(d, valid, mut, tail):
    """(d, valid) as the reduction loops see them: the chunk, one sample less (drop_last) or one
    sample more (j_le_n: the sample that follows the chunk in the stream)"""
    d, valid = np.asarray(d, dtype=np.float64), np.asarray(valid, dtype=bool)
    if mut == "drop_last":
        valid = valid.copy()
        valid[-1] = False
    if mut == "j_le_n" and tail is not None:
        d, valid = np.append(d, tail[0]), np.append(valid, bool(tail[1]))
    return d, valid


# ------------------------------------------------------------------- the mean ----
def mean_ref(d, valid):
    d, valid = _ld(d), np.asarray(valid, dtype=bool)
    cnt = int(valid.sum())
    if cnt == 0:
        return np.zeros(d.size, dtype=LD), np.zeros(d.size, dtype=LD)
    return d - d[valid].sum() / LD(cnt), np.abs(d) + np.abs(d[valid]).sum() / LD(cnt)


def mean_f64(d, valid, mut=None, tail=None):
    d = np.asarray(d, dtype=np.float64)
    n = d.size
    if n == 0:
        return np.zeros(0)
    ds, vs = _sum_domain(d, valid, mut, tail)
    lane = np.arange(n) % KWAVE
    s = lane_allsum(np.where(vs, ds, 0.0), mut)
    cnt = lane_allsum(vs.astype(np.float64), mut)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (s / cnt)[lane]
    if not np.isfinite(mean).all():
        return np.zeros(n)
    return d - mean


# ---------------------------------------------------------- no flag: d - T T^T d ----
def poly_noflag_ref(d, T):
    d, T = _ld(d), _ld(T)
    return d - T @ (T.T @ d), np.abs(d) + np.abs(T) @ (np.abs(T).T @ np.abs(d))


def poly_noflag_f64(d, T, mut=None):
    d = np.asarray(d, dtype=np.float64)
    n, K = T.shape
    ds, vs = _sum_domain(d, np.ones(n, dtype=bool), mut, None)
    lane = np.arange(n) % KWAVE
    c = lane_allsum(np.where(vs[:, None], T * ds[:, None], 0.0), mut)          # (64, K)
    p = np.zeros(n)
    for k in range(K):
        p = p + c[lane, k] * T[:, k]
    return d - p


# ------------------------------------------------- some flags: d - Q Q^T d ----------
def ortho_basis_ld(pos, K):
    """Orthonormal basis of the polynomials of degree < K on the integer positions `pos`, in
    extended precision: q_0 = const, q_k = x q_{k-1} orthogonalised against ALL earlier columns
    (three Gram-Schmidt passes) on the support rescaled to [-1, 1].  No Vandermonde or Legendre
    block is ever formed, so no ill-conditioned basis stands between the positions and Q."""
    pos = _ld(pos)
    m = pos.size
    x = (LD(2) * pos - (pos[0] + pos[-1])) / (pos[-1] - pos[0]) if m > 1 else np.zeros(1, dtype=LD)
    Q = np.zeros((m, K), dtype=LD)
    Q[:, 0] = LD(1) / np.sqrt(LD(m))
    for k in range(1, K):
        v = x * Q[:, k - 1]
        for _ in range(3):
            v = v - Q[:, :k] @ (Q[:, :k].T @ v)
        Q[:, k] = v / np.sqrt(v @ v)
    return Q


def poly_flagged_ref(d, valid, K):
    d, valid = _ld(d), np.asarray(valid, dtype=bool)
    ref, S = np.zeros(d.size, dtype=LD), np.zeros(d.size, dtype=LD)
    Q = ortho_basis_ld(np.flatnonzero(valid), K)
    dv = d[valid]
    ref[valid] = dv - Q @ (Q.T @ dv)
    S[valid] = np.abs(dv) + np.abs(Q) @ (np.abs(Q).T @ np.abs(dv))
    return ref, S


def poly_flagged_f64(d, valid, K, mut=None, tail=None):
    d, valid = np.asarray(d, dtype=np.float64), np.asarray(valid, dtype=bool)
    n = d.size
    ds, vs = _sum_domain(d, valid, mut, tail)
    ns = ds.size
    idx = np.flatnonzero(vs)
    jmin, jmax = int(idx[0]), int(idx[-1])
    xc, xs = np.float64(0.5) * np.float64(jmin + jmax), np.float64(2.0) / np.float64(jmax - jmin)
    x = (np.arange(ns, dtype=np.float64) - xc) * xs
    alpha, beta, nrm = np.zeros(K), np.zeros(K), np.zeros(K)

    def ortho_eval(upto):
        p = [np.ones(ns)]
        if upto >= 1:
            p.append(x - alpha[0])
        for k in range(1, upto):
            bk = beta[k - 1] if mut == "beta_prev" else beta[k]
            p.append((x - alpha[k]) * p[k] - bk * p[k - 1])
        return p

    with np.errstate(divide="ignore", invalid="ignore"):
        for level in range(K):                                           # StieltjesStep<K, level>
            pl = ortho_eval(level)[level]
            pp = pl * pl
            s0 = lane_allsum(np.where(vs, pp, 0.0))[0]
            s1 = lane_allsum(np.where(vs, x * pp, 0.0))[0]
            nrm[level] = s0
            alpha[level] = s1 / s0
            beta[level] = s0 / nrm[level - 1] if level > 0 else 0.0
        inorm = 1.0 / np.sqrt(nrm)
    p = ortho_eval(K - 1)
    q = [p[k] * inorm[k] for k in range(K)]
    c = [lane_allsum(np.where(vs, q[k] * ds, 0.0))[0] for k in range(K)]
    proj = np.zeros(ns)
    for k in range(K):
        proj = proj + c[k] * q[k]
    o = (ds - proj)[:n]
    return o if mut == "flagged_written" else np.where(valid, o, 0.0)


# ------------------------------------------------------------------ one chunk ----
def chunk_kind(order, pix, mut=None):
    """'mean' for order 0, else 0 (too few unflagged samples), 1 (no flag), 2 (some flags)"""
    if order == 0:
        return "mean"
    cnt, K = int((np.asarray(pix) >= 0).sum()), order + 1
    if cnt <= (K if mut == "kind_threshold" else K - 1):
        return 0
    return 1 if cnt == len(pix) else 2


def chunk_ref(order, pix, d, T):
    kind = chunk_kind(order, pix)
    n = len(pix)
    if kind == "mean":
        return mean_ref(d, np.asarray(pix) != -1) + (kind,)
    if kind == 0:
        return np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), kind
    if kind == 1:
        return poly_noflag_ref(d, T) + (kind,)
    return poly_flagged_ref(d, np.asarray(pix) >= 0, order + 1) + (kind,)


def chunk_f64(order, pix, d, T, mut=None, tail=None):
    kind = chunk_kind(order, pix, mut)
    if kind == "mean":
        tl = None if tail is None else (tail[0], tail[1] != -1)
        return mean_f64(d, np.asarray(pix) != -1, mut, tl)
    if kind == 0:
        return np.zeros(len(pix))
    if kind == 1:
        return poly_noflag_f64(d, T, mut)
    tl = None if tail is None else (tail[0], tail[1] >= 0)
    return poly_flagged_f64(d, np.asarray(pix) >= 0, order + 1, mut, tl)


# ----------------------------------------------------------- the whole stream ----
def filter_segments(subscans, tstart, nsamples, nbolos):
    """(start, length) of every chunk, CES -> detector pair -> sub-scan, then ascending"""
    starts, lens, offset = [], [], 0
    for sub, ts, ns, nb in zip(subscans, tstart, nsamples, nbolos):
        for b in range(int(nb)):
            for n, t0 in zip(sub, ts):
                starts.append(int(t0) + int(ns) * b + offset)
                lens.append(int(n))
        offset += int(nb) * int(ns)
    starts, lens = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    o = np.argsort(starts, kind="stable")
    return starts[o], lens[o]


def _table(legendres, order, n, mut=None):
    if order == 0 or n == 0:
        return None
    if mut == "table_neighbour":         # toff of the next longer chunk length: its first n K words
        other = min(m for m in legendres if m > n)
        return np.asarray(legendres[other]).reshape(-1)[:n * (order + 1)].reshape(n, order + 1)
    return np.asarray(legendres[n], dtype=np.float64)


def stream_ref(order, starts, lens, pix, d, legendres):
    """-> (ref, S, c per element, kind per chunk)"""
    nt = len(d)
    ref, S, c = np.zeros(nt, dtype=LD), np.zeros(nt, dtype=LD), np.ones(nt)
    kinds = []
    for a, n in zip(starts, lens):
        a, n = int(a), int(n)
        r, s, kind = chunk_ref(order, pix[a:a + n], d[a:a + n], _table(legendres, order, n))
        ref[a:a + n], S[a:a + n] = r, s
        c[a:a + n] = {"mean": c_mean(n), 0: 1, 1: c_noflag(n, order + 1)}.get(kind) or c_flagged(order)
        kinds.append(kind)
    return ref, S, c, kinds


def stream_f64(order, starts, lens, pix, d, legendres, mut=None, only=None):
    """k_filter_mean / k_filter_poly on a NaN-filled output.  `only`: the chunk a mutation hits
    (default: every chunk it can apply to)."""
    nt = len(d)
    out = np.full(nt, np.nan)
    end = 0
    for s, (a, n) in enumerate(zip(starts, lens)):
        a, n = int(a), int(n)
        m = mut if (only is None or only == s) else None
        if not (m == "gap_not_zeroed"):
            out[end:a] = 0.0
        tail = (d[a + n], pix[a + n]) if a + n < nt else None
        if m == "table_neighbour" and (chunk_kind(order, pix[a:a + n]) != 1 or
                                       not any(k > n for k in legendres)):
            m = None
        if m in ("drop_last", "j_le_n") and n == 0:
            m = None
        out[a:a + n] = chunk_f64(order, pix[a:a + n], d[a:a + n], _table(legendres, order, n, m), m, tail)
        end = a + n
    out[end:] = 0.0
    return out


# ------------------------------------------------------------- the tile order ----
def windows_plan(starts, lens, nt):
    """filter_windows_build: -> wins [(t0, span, s0, s1)], ok, memset, and block_map(nwin)"""
    S, L = [int(v) for v in starts], [int(v) for v in lens]
    nseg = len(S)
    wins, memset = [], (nseg == 0 or S[0] > 0)
    s0 = 0
    while s0 < nseg:
        t0, s1 = S[s0], s0
        while s1 < nseg and S[s1] + L[s1] - t0 <= WIN_LEN and s1 - s0 < (1 << 20):
            s1 += 1
        if s1 == s0:                                   # a chunk longer than a window
            return SimpleNamespace(wins=[], ok=False, memset=memset, nwin=0)
        t1 = S[s1 - 1] + L[s1 - 1]
        nxt = S[s1] if s1 < nseg else int(nt)
        if nxt - t0 <= WIN_LEN:
            t1 = nxt                                   # the trailing gap rides along
        else:
            memset = True
        wins.append((t0, t1 - t0, s0, s1))
        s0 = s1
    return SimpleNamespace(wins=wins, ok=True, memset=memset, nwin=len(wins))


def block_map(nwin, mut=None):
    """blockIdx.x -> wid of k_filter_windows for the grid launch_windows gives it; wid >= nwin
    means the workgroup exits"""
    per_xcd = (nwin + 7) // 8
    grid = per_xcd * 8
    if mut == "drop_window":                           # a grid of nwin workgroups, not rounded up
        grid = nwin
    return [(b & 7) * per_xcd + (b >> 3) for b in range(grid)]


def windows_f64(order, starts, lens, pix, d, legendres, mut=None):
    """cm2_filter_apply_tiles on a NaN-filled tile-order buffer, brought back to the time order
    (flagged samples 0, as cm2_tod_tiles_to_time leaves them).  None if the plan is not tileable."""
    nt = len(d)
    plan = windows_plan(starts, lens, nt)
    if not plan.ok:
        return None
    valid = np.asarray(pix) >= 0
    out = np.zeros(nt) if plan.memset else np.full(nt, np.nan)
    for wid in block_map(plan.nwin, mut):
        if wid >= plan.nwin:
            continue
        t0, span, s0, s1 = plan.wins[wid]
        data = np.array(d[t0:t0 + span], dtype=np.float64)
        prev = 0
        for s in range(s0, s1):
            a, n = int(starts[s]) - t0, int(lens[s])
            data[prev:a] = 0.0
            data[a:a + n] = chunk_f64(order, pix[t0 + a:t0 + a + n], d[t0 + a:t0 + a + n],
                                      _table(legendres, order, n))
            prev = a + n
        if mut != "trailing_gap":
            data[prev:span] = 0.0
        seg = out[t0:t0 + span]
        seg[valid[t0:t0 + span]] = data[valid[t0:t0 + span]]
    out[~valid] = 0.0
    return out


# ---------------------------------------------------------------------- cases ----
NPIX_TILES = 640
TILE_ORDERS_ALL = tuple(range(8))
TILE_ORDERS_FEW = (0, 2, 7)


def _dedupe(seq):
    out = []
    for v in seq:
        if v > 0 and v not in out:
            out.append(v)
    return out


def _pattern(rng, which, n, K):
    """detector 2's flags of one chunk -> boolean `unflagged`"""
    ok = np.zeros(n, dtype=bool)
    if which == 0:                                     # all flagged
        pass
    elif which in (1, 2):                              # exactly K - 1 / exactly K unflagged
        ok[rng.choice(n, size=min(n, K - 2 + which), replace=False)] = True
    elif which == 3:                                   # first and last sample flagged
        ok[1:n - 1] = True
    elif which == 4:                                   # only a run of 3 K samples at the start
        ok[:3 * K] = True
    else:                                              # K unflagged at each end only
        ok[:K] = True
        ok[max(0, n - K):] = True
    return ok


def time_case(order):
    """One CES of 4 detectors whose sub-scans have every size at which the kernels change path,
    followed by a one-detector CES of one sub-scan (4 detectors x sub-scans is a multiple of 4;
    the extra chunk makes nseg % 4 == 1)."""
    K = order + 1
    rng = np.random.default_rng(7000 + order)
    sizes = _dedupe([1, 2, K - 1, K, K + 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4100])
    sizes.insert(len(sizes) // 2, 0)                   # one zero-length sub-scan
    gaps = (0, 1, 63, 64, 65)
    tstart, at = [], 3                                 # the first chunk starts at sample 3
    for i, n in enumerate(sizes):
        tstart.append(at)
        at += n + gaps[i % len(gaps)]
    ns = tstart[-1] + sizes[-1] + 70                   # 70 samples follow the last chunk
    sub2, ts2, ns2 = [130], [2], 140
    subscans, tstarts = [np.array(sizes), np.array(sub2)], [np.array(tstart), np.array(ts2)]
    nsamples, nbolos = [ns, ns2], [4, 1]
    nt = 4 * ns + ns2
    pix = rng.integers(0, 1000, size=nt).astype(np.int32)
    det = lambda b: slice(b * ns, (b + 1) * ns)
    f1 = rng.random(ns) < 0.10                         # detector 1: 10 % random, some as -2
    p1 = pix[det(1)]
    p1[f1] = np.where(rng.random(int(f1.sum())) < 0.3, -2, -1)
    # detector 2: six patterns in rotation, started so that 513, 2047, 2048 | 2049, 4100 get
    # patterns 4, 5, 0 | 1, 2: the only phase that gives a skipped chunk (kind 0) to RegChunk<32>
    # and to MemChunk as well; the 11 shorter chunks see all six
    phase = 4 - sizes.index(513)
    p2 = pix[det(2)]
    for i, (t0, n) in enumerate(zip(tstart, sizes)):
        p2[t0:t0 + n][~_pattern(rng, (i + phase) % 6, n, K)] = -1
    pix[det(3)][rng.random(ns) < 0.50] = -1            # detector 3: 50 % random
    pix[4 * ns:][rng.random(ns2) < 0.10] = -1
    d = rng.standard_normal(nt) + 3.0 + 1e-3 * np.arange(nt)
    starts, lens = filter_segments(subscans, tstarts, nsamples, nbolos)
    assert len(starts) % 4 == 1 and starts[0] == 3
    return SimpleNamespace(order=order, nt=nt, args=([subscans, tstarts], nsamples, nbolos), pix=pix,
                           d=d, starts=starts, lens=lens, sizes=sizes)


def _abs_chunks(windows):
    """[(t0, [(offset, length), ...]), ...] -> starts, lens"""
    starts, lens = [], []
    for t0, chunks in windows:
        for off, n in chunks:
            starts.append(t0 + off)
            lens.append(n)
    return np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)


def _tile_layout(name):
    """-> starts, lens, nt, chunks per window (None: not tileable), memset, special chunks"""
    if name == "a":
        t3 = 16384 + 6013
        t4, t5 = t3 + 8150, t3 + 8150 + 8120
        t6 = t5 + 8000
        t7 = t6 + 8192
        t8 = t7 + 8192
        wins = [(0, [(0, 8192)]),                                            # exactly one window
                (8192, [(0, 3000), (3005, 3000), (6012, 2180)]),             # ends on offset 8192
                (16384, [(0, 3000), (3005, 3000)]),                          # the same, one sample later:
                (t3, [(0, 2180), (2200, 1000), (3300, 1500), (4800, 64), (4900, 3000)]),   # opens the next
                (t4, [(90 * i, 89) for i in range(90)]),
                (t5, [(0, 700), (700, 700), (1400, 700)]),                   # kinds 0, 1, 2 side by side
                (t6, [(0, 1000), (1000, 2000)]),                             # every sample flagged; usual
                (t7, [(0, 8191)]),
                (t8, [(0, 513), (600, 2049), (3000, 4100)])]
        s, l = _abs_chunks(wins)
        special = {"few": 90 + 11, "none": 90 + 12, "all": 90 + 14, "none2": 9}
        return s, l, t8 + 8000, [1, 3, 2, 5, 90, 3, 2, 1, 3], False, special
    if name.startswith("b"):
        nwin = int(name[1:])
        wins = [(8192 * w, [(0, 3000), (3050, 2000 + w)]) for w in range(nwin)]
        s, l = _abs_chunks(wins)
        return s, l, 8192 * nwin, [2] * nwin, False, {}
    if name.startswith("c"):
        s, l, nt, per, memset = {
            "c0": ([0, 2100], [2000, 2900], 8000, [2], False),       # the trailing gap fits
            "c1": ([0, 2100], [2000, 2900], 9000, [2], True),        # it does not
            "c2": ([3, 2103], [2000, 2900], 8000, [2], True),        # S[0] > 0
            "c3": ([0, 9000], [3000, 3000], 12500, [1, 1], True),    # samples between two windows
        }[name]
        return np.array(s, dtype=np.int64), np.array(l, dtype=np.int64), nt, per, memset, {}
    assert name == "d"
    return np.array([0, 200], dtype=np.int64), np.array([100, 8193], dtype=np.int64), 9000, None, False, {}


TILE_LAYOUTS = {"a": TILE_ORDERS_ALL, "b1": TILE_ORDERS_FEW, "b7": TILE_ORDERS_FEW, "b8": TILE_ORDERS_FEW,
                "c0": TILE_ORDERS_FEW, "c1": TILE_ORDERS_FEW, "c2": TILE_ORDERS_FEW, "c3": TILE_ORDERS_FEW,
                "d": TILE_ORDERS_FEW}
TILE_LAYOUT_E = "b7"                 # layout (e): this one on a second tile plan and back


def tile_case(name, order):
    """One detector, chunks given by their starts; pixels in [0, 640), 10 % flagged (-1)."""
    K = order + 1
    starts, lens, nt, per_window, memset, special = _tile_layout(name)
    rng = np.random.default_rng(9000 + 17 * order + sum(map(ord, name)))
    pix = rng.integers(0, NPIX_TILES, size=nt).astype(np.int32)
    flagged = rng.random(nt) < 0.10
    for key, s in special.items():
        a, n = int(starts[s]), int(lens[s])
        if key == "all":
            flagged[a:a + n] = True
        elif key == "few":                             # K - 1 unflagged: kind 0
            flagged[a:a + n] = True
            flagged[a + rng.choice(n, size=K - 1, replace=False)] = False
        else:
            flagged[a:a + n] = False
    pix[flagged] = -1
    d = rng.standard_normal(nt) + 3.0 + 1e-3 * np.arange(nt)
    return SimpleNamespace(name=name, order=order, nt=nt, args=([lens, starts], nt, 1), pix=pix, d=d,
                           starts=starts, lens=lens, per_window=per_window, memset=memset)


def flagged_ratio(order, case, scale=1.0):
    """largest |restatement - ref| / (2^-53 S) over the flagged (kind 2) chunks of a case"""
    worst = 0.0
    d = case.d * scale
    for a, n in zip(case.starts, case.lens):
        a, n = int(a), int(n)
        px = case.pix[a:a + n]
        if chunk_kind(order, px) != 2:
            continue
        ref, S = poly_flagged_ref(d[a:a + n], px >= 0, order + 1)
        worst = max(worst, excess(poly_flagged_f64(d[a:a + n], px >= 0, order + 1), ref, S, 1))
    return worst


def measure_flagged(order):
    worst = max(flagged_ratio(order, time_case(order)), flagged_ratio(order, time_case(order), 2.0 ** 20))
    for name, orders in TILE_LAYOUTS.items():
        if order in orders:
            worst = max(worst, flagged_ratio(order, tile_case(name, order)))
    return worst


# --------------------------------------------------------------- ground filter ----
GROUND_SHAPES = ((1, 1), (255, 3), (16384, 256), (16385, 257), (100001, 8192))


def ground_case(nt, nbins):
    """labels in [-1, nbins) with one empty bin (where there is room for one) and the last bin hit"""
    rng = np.random.default_rng(500 + nt + nbins)
    g = rng.integers(-1, nbins, size=nt).astype(np.int32)
    if nbins >= 3:
        g[g == 1] = 2                                  # bin 1 stays empty
    g[-1] = nbins - 1
    return g, rng.standard_normal(nt) + 0.5


def ground_ref(g, v, nbins):
    """-> sums, sum |v|, hits per bin; filtered stream and its magnitude per sample"""
    g, vl = np.asarray(g), _ld(v)
    ok = g >= 0
    hits = np.bincount(g[ok], minlength=nbins)
    sums, mags = np.zeros(nbins, dtype=LD), np.zeros(nbins, dtype=LD)
    np.add.at(sums, g[ok], vl[ok])
    np.add.at(mags, g[ok], np.abs(vl[ok]))
    gi = np.where(ok, g, 0)
    h = np.maximum(hits, 1).astype(LD)
    out = np.where(ok, vl - (sums / h)[gi], vl)
    S = np.where(ok, np.abs(vl) + (mags / h)[gi], np.abs(vl))
    return sums, mags, hits, out, S, np.where(ok, hits[gi], 0)


def c_ground_sums(hits):
    # hits terms in any order: at most hits roundings on a sum, + 2
    return np.asarray(hits) + 2


def c_ground_filtered(hits_of_sample):
    # the bin sum (hits), times 1 / hits or divided by it (2 at most), v - binned (1), + 2;
    # a sample with label -1 is copied: S = |v| and any c demands the exact value only if got == v,
    # which the test asserts bit for bit
    return np.asarray(hits_of_sample) + 3 + 2
