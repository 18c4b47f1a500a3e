"""
References and error bounds for the map-domain vector kernels (csrc/cm2_vector.hip).

Plain NumPy, no GPU.  Every operation comes as

  * ``*_ref(...) -> (ref, S)``: the value in extended precision (np.longdouble, 64-bit
    mantissa) and its magnitude S, the same formula with every operand replaced by its
    absolute value and every subtraction by an addition.  S is a componentwise running
    error bound: a float64 evaluation whose longest chain of rounded operations has
    length d is off by at most  d * 2^-53 * S  to first order, whatever the order of
    the terms.  The acceptance rule is  |got - ref| <= c * 2^-53 * S  element by
    element with  c = d + 2  (the 2 pays for the second-order terms and for the
    reference's own 2^-64 roundings).  The c_* functions below return c, counted from
    the kernel source; the count is written next to each.
  * ``*_f64(...)``: where the kernel promises a term order, a float64 restatement in
    exactly that order.  The library is built with -ffp-contract=off and NumPy's
    elementwise loops do not fuse, so these match the GPU bit for bit.

The launch arithmetic of the entry points (workgroups, rows per workgroup) is restated
here because the chain lengths depend on it.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit mantissa on this platform"

U53 = LD(2.0) ** -53


def _ld(a):
    return np.asarray(a, dtype=LD)


def _ceil(a, b):
    return -(-int(a) // int(b))


# ----------------------------------------------------------------- acceptance ----
def excess(got, ref, S, c):
    """max over ALL elements of |got - ref| / (c 2^-53 S); <= 1 passes.  Where S = 0 the result
    must be exact (ratio 0 or inf).  NaN anywhere gives inf."""
    got, ref, S = _ld(got).reshape(-1), _ld(ref).reshape(-1), _ld(S).reshape(-1)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    bound = LD(c) * U53 * S
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, LD(0), LD(np.inf)))
    ratio = np.where(np.isnan(ratio), LD(np.inf), ratio)
    return float(ratio.max())


def assert_within(got, ref, S, c, what=""):
    e = excess(got, ref, S, c)
    assert e <= 1.0, "%s: |got - ref| is %.3g x the bound c 2^-53 S (c = %d)" % (what, e, c)
    return e


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def assert_bit_equal(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %r != %r" % (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %r (%s) != %r (%s)" % (
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], float(got.reshape(-1)[bad[0]]).hex(),
        want.reshape(-1)[bad[0]], float(want.reshape(-1)[bad[0]]).hex())


# --------------------------------------------------------------------- inputs ----
def normals(seed, *shape):
    """(a) standard normals"""
    return np.random.default_rng(seed).standard_normal(shape)


def cancelling(seed, n, ra=None, rb=None):
    """(b) A (n[, ra]) and B (n[, rb]) whose row-wise products cancel: rows come in pairs
    (+v, w), (-v (1 + 2^-30), w), shuffled, plus a tail of at most 5 rows 1e-6 small.  Every
    sum_i A[i, a] B[i, b] is ~1e-9 of sum_i |A[i, a] B[i, b]|."""
    rng = np.random.default_rng(seed)
    sa = (ra,) if ra is not None else ()
    sb = (rb,) if rb is not None else ()
    m = max(0, (n - 3) // 2)
    t = n - 2 * m
    va, vb = rng.standard_normal((m,) + sa), rng.standard_normal((m,) + sb)
    A = np.concatenate([va, -va * (1.0 + 2.0 ** -30), 1e-6 * rng.standard_normal((t,) + sa)])
    B = np.concatenate([vb, vb, rng.standard_normal((t,) + sb)])
    perm = rng.permutation(n)
    return np.ascontiguousarray(A[perm]), np.ascontiguousarray(B[perm])


HITS = (40, 0, 1, 2)


def pixel_weights(seed, npix, shift=0):
    """(c) per-pixel sums from k random-angle hits, k = HITS[(npix - 1 - j + shift) % 4]: counted
    from the END of the map, so that with shift = 0 the last pixel has 40 hits (regular for every
    pol) and the one before it none (singular for every pol) -- both in the last partial block of
    any blocking that leaves two pixels there; shift = 1 makes the last pixel the empty one."""
    rng = np.random.default_rng(seed)
    k = np.array([HITS[(npix - 1 - j + shift) % 4] for j in range(npix)], dtype=np.int64)
    W = {f: np.zeros(npix) for f in ("counts", "cosine", "sine", "cos2", "sin2", "sincos")}
    for j in range(npix):
        phi = rng.uniform(0.0, np.pi, k[j])
        c, s = np.cos(2.0 * phi), np.sin(2.0 * phi)
        W["counts"][j] = float(k[j])
        W["cosine"][j], W["sine"][j] = c.sum(), s.sum()
        W["cos2"][j], W["sin2"][j], W["sincos"][j] = (c * c).sum(), (s * s).sum(), (c * s).sum()
    return W


def det_mask_f64(pol, W):
    """cm2_bd_det_mask (cm2_pixel.hip) in its operation order -> (det, mask uint8)."""
    n, c, s = W["counts"], W["cosine"], W["sine"]
    c2, s2, cs = W["cos2"], W["sin2"], W["sincos"]
    if pol == 1:
        return n.copy(), (n > 0.0).astype(np.uint8)
    if pol == 2:
        d = (c2 * s2) - (cs * cs)
    else:
        d = (((n * (c2 * s2 - cs * cs)) - (c * c) * s2) - (s * s) * c2) + ((2.0 * c) * s) * cs
    return d, (np.abs(d) > 1e-5).astype(np.uint8)


# ---------------------------------------------------- launch arithmetic restated ---
K_BLOCK, K_RED_BLOCKS, K_GEMM_BLOCKS, K_NUM_CU = 256, 1024, 128, 256
ELEMENTWISE_THREADS = K_NUM_CU * 8 * K_BLOCK          # grid_for(): 2048 workgroups of 256


def red_blocks(n):
    return min(max(_ceil(n, K_BLOCK), 1), K_RED_BLOCKS)


def pow2_at_least(r):
    p = 1
    while p < r:
        p <<= 1
    return p


def zt_plan(n, r, aligned):
    """(wide?, rstep, rows per workgroup, workgroups) of cm2_Zt_apply"""
    if r in (16, 32, 64) and n >= 4096 and aligned:
        rstep = 4 * (128 // r)
        rows = _ceil(_ceil(n, K_RED_BLOCKS), rstep) * rstep
        return True, rstep, rows, _ceil(n, rows)
    rstep = 256 // pow2_at_least(r)
    rows = max(_ceil(_ceil(n, red_blocks(n)), rstep) * rstep, rstep)
    return False, rstep, rows, max(_ceil(n, rows), 1)


def gemm_tn_plan(n, r1, r2, aligned):
    """(kernel, rows per wave or workgroup) of cm2_gemm_tn"""
    mfma = r1 % 16 == 0 and r2 % 16 == 0 and r1 <= 64 and r2 <= 64 and r1 == r2
    if mfma and aligned and r1 in (32, 64):
        return "pairs", (_ceil(n, 4 * K_GEMM_BLOCKS * 4) + 3) // 4 * 4      # 512 workgroups x 4 waves
    if mfma:
        return "mfma", (_ceil(n, K_GEMM_BLOCKS * 4) + 3) // 4 * 4
    return "scalar", _ceil(n, K_GEMM_BLOCKS * 4)


def m2_is_wide(npix, r, aligned):
    return r in (16, 32, 64) and aligned and npix >= 64


# -------------------------------------------------------------- the constants c ---
def c_dot(n):
    # k_dot_partial: a thread takes T = ceil(n / (g 256)) terms: 1 product + (T - 1) adds (0 + p is
    # exact) = T; block_sum_256: 6 wave steps + 3 adds of the 4 wave sums; k_reduce_final: a thread
    # takes F = ceil(g / 256) partials, F - 1 adds, then 6 + 3 again.
    g = red_blocks(n)
    T, F = _ceil(n, g * K_BLOCK), _ceil(g, K_BLOCK)
    return T + 6 + 3 + (F - 1) + 6 + 3 + 2


def c_update_xr_rr(n):
    # rr = sum rn^2, rn = r - alpha q, alpha = rho / pq: the division, the product and the
    # subtraction put 3 roundings on rn relative to |r| + |alpha| |q|, the square doubles them (6),
    # then the chain of c_dot (the rounded square is its "product")
    return c_dot(n) + 6


def c_zt(n, r, aligned):
    # k_Zt_partial and k_Zt_partial_wide alike: a thread takes T = rows / rstep rows of its
    # workgroup (1 product + T - 1 adds = T); one thread per column then adds the workgroup's rstep
    # sums from LDS (rstep - 1; wide: 4 waves x 64 / LPR row groups = rstep as well);
    # k_Zt_final: a thread adds ceil(nblk / qn) partials (that - 1), qn = 1024 / rp, then one thread
    # per column adds qn sums (qn - 1)
    _, rstep, rows, nblk = zt_plan(n, r, aligned)
    qn = 1024 // pow2_at_least(r)
    return rows // rstep + (rstep - 1) + (_ceil(nblk, qn) - 1) + (qn - 1) + 2


def c_serial(terms):
    # acc = 0; acc += a_k b_k for k < terms: 1 product + (terms - 1) adds
    return terms + 2


def c_z_axpy(r, wide):
    # narrow: the r-term chain, alpha * acc, w + .        wide: 2 products + 1 add inside a lane is a
    # chain of 2, log2(r / 2) butterfly adds, alpha * p, w + .
    return (r + 2 if not wide else 2 + int(np.log2(r // 2)) + 2) + 2


def c_gemm_tn(n, r1, r2, aligned):
    # mfma: a wave's accumulator takes its `chunk` rows one after the other, 4 per instruction:
    #   at most 1 rounding for the product and 1 per add, chunk + 1 (an MFMA that fuses does fewer);
    #   pairs kernel: + 3 adds of the four waves' accumulators through LDS
    # scalar: 1 product + (chunk - 1) adds = chunk
    # k_gemm_tn_final (512 partials): a thread adds 32 of them (31), then 16 sums in order (15)
    kind, chunk = gemm_tn_plan(n, r1, r2, aligned)
    body = {"pairs": chunk + 1 + 3, "mfma": chunk + 1, "scalar": chunk}[kind]
    return body + 31 + 15 + 2


def c_panel_gemm(rin, mfma):
    # scalar: acc = out or 0, then rin times acc += P W: rin products feeding rin adds: rin + 1
    # mfma (rin = 32): 8 instructions of 4 terms on one accumulator, the same rin + 1 at most
    return rin + 1 + 2


def c_m2(pol, r, wide):
    # Z y and AZ y: narrow r (serial chain), wide 2 + log2(r / 2) as in c_z_axpy
    # t = res - AZ y: 1
    # block, pol 3: cofactor (a b - c d) 2, times t 1, two adds of the three terms 2, / det 1 = 6;
    #        pol 2: the cofactor is an input, times t 1, one add 1, / det 1 = 3;  pol 1: / hits = 1
    # + Z y: 1
    zy = r if not wide else 2 + int(np.log2(r // 2))
    block = {1: 1, 2: 3, 3: 6}[pol]
    return zy + 1 + block + 1 + 2


# ------------------------------------------------------- elementwise restatements ---
def axpy_f64(a, x, y):
    return y + a * x


def scal_f64(a, x):
    return a * x


def xmy_f64(x, y):
    return x * y


def update_p_f64(rho, rho_prev, z, p):
    beta = np.float64(rho) / np.float64(rho_prev)
    return p * beta + z


def update_xr_f64(rho, pq, p, q, x, r):
    alpha = np.float64(rho) / np.float64(pq)
    return x + alpha * p, r - alpha * q


# the same in extended precision, with c: one rounding per operation of the expression
C_AXPY, C_SCAL, C_XMY = 2 + 2, 1 + 2, 1 + 2        # a x, y + . | a x | x y
C_UPDATE_P = 3 + 2                                 # rho / rho_prev, p beta, . + z
C_UPDATE_XR = 3 + 2                                # rho / pq, alpha p, x + .  (r alike)


def axpy_ref(a, x, y):
    return _ld(y) + LD(a) * _ld(x), np.abs(_ld(y)) + abs(LD(a)) * np.abs(_ld(x))


def scal_ref(a, x):
    return LD(a) * _ld(x), abs(LD(a)) * np.abs(_ld(x))


def xmy_ref(x, y):
    return _ld(x) * _ld(y), np.abs(_ld(x) * _ld(y))


def update_p_ref(rho, rho_prev, z, p):
    beta = LD(rho) / LD(rho_prev)
    return _ld(p) * beta + _ld(z), np.abs(_ld(p)) * abs(beta) + np.abs(_ld(z))


def update_xr_ref(rho, pq, p, q, x, r):
    """-> (x', Sx), (r', Sr)"""
    alpha = LD(rho) / LD(pq)
    return ((_ld(x) + alpha * _ld(p), np.abs(_ld(x)) + abs(alpha) * np.abs(_ld(p))),
            (_ld(r) - alpha * _ld(q), np.abs(_ld(r)) + abs(alpha) * np.abs(_ld(q))))


# ----------------------------------------------------------- reductions, extended ---
def dot_ref(x, y):
    x, y = _ld(x), _ld(y)
    return np.array([(x * y).sum()], dtype=LD), np.array([(np.abs(x) * np.abs(y)).sum()], dtype=LD)


def update_xr_rr_ref(rho, pq, q, r):
    alpha = LD(rho) / LD(pq)
    rn = _ld(r) - alpha * _ld(q)
    mag = np.abs(_ld(r)) + np.abs(alpha) * np.abs(_ld(q))
    return np.array([(rn * rn).sum()], dtype=LD), np.array([(mag * mag).sum()], dtype=LD)


def _rows_chunked(n, chunk=32768):
    for lo in range(0, n, chunk):
        yield lo, min(n, lo + chunk)


def zt_ref(Z, x):
    """Z^T x"""
    n, r = Z.shape
    ref, S = np.zeros(r, dtype=LD), np.zeros(r, dtype=LD)
    for lo, hi in _rows_chunked(n):
        z, v = _ld(Z[lo:hi]), _ld(x[lo:hi])[:, None]
        ref += (z * v).sum(axis=0)
        S += (np.abs(z) * np.abs(v)).sum(axis=0)
    return ref, S


def z_apply_ref(Z, y):
    """Z y, in row chunks"""
    n, r = Z.shape
    ref, S = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    yl = _ld(y)
    for lo, hi in _rows_chunked(n):
        z = _ld(Z[lo:hi])
        ref[lo:hi] = (z * yl).sum(axis=1)
        S[lo:hi] = (np.abs(z) * np.abs(yl)).sum(axis=1)
    return ref, S


def z_apply_f64(Z, y):
    """((0 + Z_i0 y0) + Z_i1 y1) + ..."""
    acc = np.zeros(Z.shape[0])
    for k in range(Z.shape[1]):
        acc = acc + Z[:, k] * y[k]
    return acc


def z_axpy_ref(Z, y, alpha, w):
    zy, szy = z_apply_ref(Z, y)
    return _ld(w) + LD(alpha) * zy, np.abs(_ld(w)) + abs(LD(alpha)) * szy


def z_axpy_f64(Z, y, alpha, w):
    return w + alpha * z_apply_f64(Z, y)


def matmul_ref(A, B):
    """A B for small inner dimension or few rows, extended"""
    A, B = _ld(A), _ld(B)
    return A @ B, np.abs(A) @ np.abs(B)


def gemm_tn_ref(Z1, Z2):
    """Z1^T Z2, row-major (r1, r2)"""
    n = Z1.shape[0]
    ref = np.zeros((Z1.shape[1], Z2.shape[1]), dtype=LD)
    S = ref.copy()
    for lo, hi in _rows_chunked(n, 4096):
        a, b = _ld(Z1[lo:hi]), _ld(Z2[lo:hi])
        ref += np.einsum("ia,ib->ab", a, b)            # (several times faster than a.T @ b here)
        S += np.einsum("ia,ib->ab", np.abs(a), np.abs(b))
    return ref, S


def panel_gemm_ref(P, W, out0=None):
    ref, S = matmul_ref(P, W)
    if out0 is not None:
        ref, S = ref + _ld(out0), S + np.abs(_ld(out0))
    return ref, S


def gemm_atbt_ref(A, B):
    """C = A^T B^T, A (k, m), B (n, k)"""
    return matmul_ref(A.T, B.T)


# ------------------------------------------------------------------- M_BD, M2 ----
def bd_inverse_f64(pol, W, det, mask, t):
    """bd_inverse_block of cm2_blocks.h, float64, its operation order; t and result (npix, pol)"""
    m = mask.astype(bool)
    n, c, s = W["counts"], W["cosine"], W["sine"]
    c2, s2, cs = W["cos2"], W["sin2"], W["sincos"]
    o = np.zeros_like(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        if pol == 1:
            o[:, 0] = t[:, 0] / n
        elif pol == 2:
            x0, x1 = t[:, 0], t[:, 1]
            o[:, 0] = (s2 * x0 - cs * x1) / det
            o[:, 1] = ((-cs) * x0 + c2 * x1) / det
        else:
            x0, x1, x2 = t[:, 0], t[:, 1], t[:, 2]
            o[:, 0] = (((c2 * s2 - cs * cs) * x0 + (s * cs - c * s2) * x1) + (c * cs - s * c2) * x2) / det
            o[:, 1] = (((s * cs - c * s2) * x0 + (n * s2 - s * s) * x1) + (s * c - n * cs) * x2) / det
            o[:, 2] = (((c * cs - s * c2) * x0 + ((-n) * cs + c * s) * x1) + (n * c2 - c * c) * x2) / det
    o[~m] = 0.0
    return o


def bd_inverse_ref(pol, W, det, mask, t, tmag):
    """-> (M_BD t, magnitude) with t of magnitude tmag, both (npix, pol) extended; det is data"""
    m = mask.astype(bool)
    n, c, s = [_ld(W[k]) for k in ("counts", "cosine", "sine")]
    c2, s2, cs = [_ld(W[k]) for k in ("cos2", "sin2", "sincos")]
    d = _ld(det)
    A = np.abs
    o, S = np.zeros_like(t), np.zeros_like(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        if pol == 1:
            o[:, 0], S[:, 0] = t[:, 0] / n, tmag[:, 0] / A(n)
        elif pol == 2:
            cof = [[s2, -cs], [-cs, c2]]
            for a in range(2):
                o[:, a] = (cof[a][0] * t[:, 0] + cof[a][1] * t[:, 1]) / d
                S[:, a] = (A(cof[a][0]) * tmag[:, 0] + A(cof[a][1]) * tmag[:, 1]) / A(d)
        else:
            # (p, q, u, v): cofactor p q - u v, magnitude |p q| + |u v|
            cof = [[(c2, s2, cs, cs), (s, cs, c, s2), (c, cs, s, c2)],
                   [(s, cs, c, s2), (n, s2, s, s), (s, c, n, cs)],
                   [(c, cs, s, c2), (c, s, n, cs), (n, c2, c, c)]]
            for a in range(3):
                acc, mag = 0, 0
                for b in range(3):
                    p, q, u, v = cof[a][b]
                    acc = acc + (p * q - u * v) * t[:, b]
                    mag = mag + (A(p * q) + A(u * v)) * tmag[:, b]
                o[:, a], S[:, a] = acc / d, mag / A(d)
    o[~m], S[~m] = 0, 0
    return o, S


def m2_finish_f64(pol, Z, AZ, y, res, W, det, mask):
    """k_m2_finish (thread per pixel), float64, its operation order"""
    zy, azy = z_apply_f64(Z, y), z_apply_f64(AZ, y)
    t = (res - azy).reshape(-1, pol)
    return (bd_inverse_f64(pol, W, det, mask, t) + zy.reshape(-1, pol)).reshape(-1)


def m2_finish_ref(pol, Z, AZ, y, res, W, det, mask, ymag=None):
    """M_BD (res - AZ y) + Z y, extended.  ymag: magnitude of y when y itself carries an error
    bound worth of uncertainty (the whole-operator test); defaults to |y|."""
    yl = _ld(y)
    ym = np.abs(yl) if ymag is None else _ld(ymag)
    zy, _ = z_apply_ref(Z, yl)
    azy, _ = z_apply_ref(AZ, yl)
    _, szy = z_apply_ref(np.abs(Z), ym)
    _, sazy = z_apply_ref(np.abs(AZ), ym)
    t = (_ld(res) - azy).reshape(-1, pol)
    tmag = (np.abs(_ld(res)) + sazy).reshape(-1, pol)
    o, So = bd_inverse_ref(pol, W, det, mask, t, tmag)
    return (o + zy.reshape(-1, pol)).reshape(-1), (So + szy.reshape(-1, pol)).reshape(-1)


def m2_apply_abs(pol, Z, AZ, W, det, mask, dy):
    """|M_BD| |AZ| dy + |Z| dy: how far an error dy >= 0 of y moves the output of M2, at most"""
    _, a = z_apply_ref(np.abs(AZ), dy)
    _, z = z_apply_ref(np.abs(Z), dy)
    zero = np.zeros((a.size // pol, pol), dtype=LD)
    _, So = bd_inverse_ref(pol, W, det, mask, zero, a.reshape(-1, pol))
    return (So + z.reshape(-1, pol)).reshape(-1)
