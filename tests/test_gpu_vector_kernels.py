"""
Every branch of the map-domain vector kernels (csrc/cm2_vector.hip) against the references of
tests/_vector_ref.py, through _hip.call on torch tensors.

Conventions of every case: each output (and the reduction scratch) is the middle of a larger
buffer pre-filled with a sentinel whose bits must be unchanged after the call; an even guard
keeps the 16-byte alignment (the wide / paired kernels), a guard of one double takes it away
(the fallbacks); scratch and outputs are NaN before each call unless the operation accumulates
into them, so a reduction that read a partial nobody wrote returns NaN; every reduction and
contraction is called twice and must return the same bits.  A result is accepted when it is
bit-equal to the float64 restatement, or when |got - ref| <= c 2^-53 S for ALL elements with
c counted from the kernel source (_vector_ref.c_*).

Kernels launched by the 17 ABI entry points of cm2_vector.hip and the case that reaches them
(to be kept in step with the dispatch code by hand):

  cm2_dot            k_dot_partial, k_reduce_final        test_dot (n = 0 .. 786437: 1 .. 1024
                                                          workgroups, 3 grid-stride trips)
  cm2_axpy           k_axpy                               test_elementwise[axpy]
  cm2_scal           k_scal                               test_elementwise[scal]
  cm2_xmy            k_xmy                                test_elementwise[xmy]
  cm2_pcg_update_p   k_pcg_update_p                       test_elementwise[update_p]
  cm2_pcg_update_xr  k_pcg_update_xr, k_reduce_final      test_pcg_update_xr
  cm2_Zt_apply       k_Zt_partial                         test_Zt_apply[r], every r at n < 4096, r not
                                                          in (16, 32, 64) at any n, r in (16, 32, 64)
                                                          unaligned at n >= 4096
                     k_Zt_partial_wide<8|16|32>           test_Zt_apply[16|32|64], aligned, n = 4096,
                                                          4097, 5003 (tail loop only) and n = 2^18 + 37,
                                                          2^17 + 37, 2^16 + 37 (unrolled body and tail)
                     k_Zt_final                           both of the above
  cm2_Z_apply        k_Z_apply                            test_Z_apply[r]
  cm2_Z_axpy         k_Z_axpy                             test_Z_axpy[5], test_Z_axpy[16|32|64] unaligned
                     k_Z_axpy_wide<8|16|32>               test_Z_axpy[16|32|64] aligned;
                                                          test_Z_axpy_grid_stride (<32>, 4097 blocks of
                                                          work on 4096 workgroups)
  cm2_gemm_tn        k_gemm_tn_mfma<1,1>                  test_gemm_tn[16-16-*]
                     k_gemm_tn_mfma<3,3>                  test_gemm_tn[48-48-*]
                     k_gemm_tn_mfma<2,2>, <4,4>           test_gemm_tn[32-32-unaligned], [64-64-unaligned]
                     k_gemm_tn_mfma_pairs<1>, <2>         test_gemm_tn[32-32-aligned], [64-64-aligned]
                                                          (n = 24581: 16-row body and tail)
                     k_gemm_tn_scalar                     test_gemm_tn[5-5|3-7|16-32|64-16]
                     k_gemm_tn_final                      all of the above
  cm2_panel_gemm     k_panel_gemm_mfma<1>, <2>            test_panel_gemm[32-16-aligned], [32-32-aligned]
                     k_panel_gemm_scalar                  test_panel_gemm[32-16|32-32-unaligned], [5-3]
  cm2_small_matvec   k_small_matvec                       test_small_matvec
  cm2_m2_finish      k_m2_finish<1|2|3>                   test_m2_finish[pol-5], [pol-16|32|64] unaligned
                                                          or npix < 64
                     k_m2_finish_wide<1|2|3, 8|16|32>     test_m2_finish[pol-16|32|64] aligned, npix >= 64;
                                                          test_m2_finish_grid_stride (<1, 8>, 4098 blocks
                                                          on 4096 workgroups); test_two_level_operator
                                                          (<3, 16>)
  cm2_gemm_atbt      k_gemm_atbt                          test_gemm_atbt
  cm2_transpose      k_transpose                          test_transpose
  not reached here:  cm2_pcg / cm2_pcg_sharded (pcg_run) and cm2_arnoldi, drivers over the kernels above
                     (tests/test_gpu_parity.py, test_gpu_sharded.py, test_gpu_round4.py), and
                     cm2_cos_sin_2phi / k_trig2 (tests/test_gpu_parity.py).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vector_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF8DEAD0000BEEF        # a NaN with a payload: no kernel produces these bits
TAIL = 8                             # sentinels after the data
ALIGNED, ODD = 2, 1                  # guard lengths (doubles) in front of the data


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device
    from types import SimpleNamespace
    return SimpleNamespace(I=I, U=U, D=device, hip=_hip, torch=torch)


class Guarded(object):
    """n elements in the middle of a sentinel-filled buffer.  data=None: NaN (an output or scratch
    that the call has to write), else the array's values."""

    def __init__(self, cm, n, data=None, guard=ALIGNED, u8=False):
        torch = cm.torch
        self.cm, self.n, self.g, self.u8 = cm, int(n), int(guard), u8
        total = self.g + self.n + TAIL
        if u8:
            self.buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=cm.D.dev())
        else:
            self.buf = torch.full((total,), SENTINEL, dtype=torch.int64, device=cm.D.dev()).view(torch.float64)
        self.v = self.buf[self.g:self.g + self.n]
        if not u8 and self.n:
            assert (self.v.data_ptr() & 15 == 0) == (self.g % 2 == 0)
        self.set(data)

    def set(self, data=None):
        if data is None:
            self.v.fill_(0 if self.u8 else float("nan"))
        elif self.cm.D.is_tensor(data):
            self.v.copy_(data.reshape(-1))
        else:
            self.v.copy_(self.cm.D.to_dev(np.ascontiguousarray(data).reshape(-1)))
        return self

    @property
    def ptr(self):
        return self.v.data_ptr()

    def get(self):
        self.cm.torch.cuda.synchronize()
        return self.v.cpu().numpy().copy()

    def intact(self, what):
        raw = self.buf if self.u8 else self.buf.view(self.cm.torch.int64)
        want = 0xA5 if self.u8 else SENTINEL
        front, back = raw[:self.g], raw[self.g + self.n:]
        assert bool((front == want).all().item()) and bool((back == want).all().item()), \
            "%s: wrote outside its %d elements" % (what, self.n)


def call(cm, name, *args):
    cm.hip.call(name, *(list(args) + [cm.D.stream()]))


def all_intact(what, *bufs):
    for b in bufs:
        b.intact(what)


def reduce_work(cm):
    return Guarded(cm, int(cm.hip.load().cm2_reduce_work_doubles()))


@functools.lru_cache(maxsize=None)
def vec_pair(family, n, seed=0):
    if family == "a":
        return R.normals(1000 + seed + n, n), R.normals(2000 + seed + n, n)
    return R.cancelling(3000 + seed + n, n)


@functools.lru_cache(maxsize=None)
def mat_vec(family, n, r):
    """Z (n, r), x (n) with cancelling column sums for family b"""
    if family == "a":
        return R.normals(4000 + n + r, n, r), R.normals(5000 + n + r, n)
    x, Z = R.cancelling(6000 + n + r, n, None, r)
    return Z, x


# ======================================================================= elementwise ===
N_ELEMENTWISE = (1, 255, 256, 257, 524287, 524288, 524289, 1048579)
assert R.ELEMENTWISE_THREADS == 524288      # the last three sizes take the grid-stride trip


@pytest.mark.parametrize("op", ["axpy", "scal", "xmy", "update_p"])
def test_elementwise(cm, op):
    a = -0.625 + 2.0 ** -40
    for n in N_ELEMENTWISE:
        x, y = vec_pair("a", n)
        for guard in (ALIGNED, ODD):
            what = "%s n=%d guard=%d" % (op, n, guard)
            gx, gy = Guarded(cm, n, x, guard), Guarded(cm, n, y, guard)
            if op == "axpy":
                call(cm, "cm2_axpy", n, a, gx.ptr, gy.ptr)
                got, want = gy.get(), R.axpy_f64(a, x, y)
            elif op == "scal":
                call(cm, "cm2_scal", n, a, gx.ptr)
                got, want = gx.get(), R.scal_f64(a, x)
            elif op == "xmy":
                out = Guarded(cm, n, None, guard)
                call(cm, "cm2_xmy", n, gx.ptr, gy.ptr, out.ptr)
                got, want = out.get(), R.xmy_f64(x, y)
                out.intact(what)
            else:
                rho, rho_prev = Guarded(cm, 1, [0.7], guard), Guarded(cm, 1, [1.9], guard)
                call(cm, "cm2_pcg_update_p", n, rho.ptr, rho_prev.ptr, gx.ptr, gy.ptr)
                got, want = gy.get(), R.update_p_f64(0.7, 1.9, x, y)
                all_intact(what, rho, rho_prev)
            R.assert_bit_equal(got, want, what)
            all_intact(what, gx, gy)


# ================================================================ dot, pcg_update_xr ===
N_REDUCE = (1, 255, 256, 257, 262143, 262144, 262145, 786437)     # 1024 partials of 256 threads


@pytest.mark.parametrize("family", ["a", "b"])
def test_dot(cm, family):
    work, out = reduce_work(cm), Guarded(cm, 1)
    for n in (0,) + N_REDUCE:
        x, y = vec_pair(family, n) if n else (np.zeros(0), np.zeros(0))
        ref, S = R.dot_ref(x, y)
        for guard in (ALIGNED, ODD):
            what = "dot n=%d guard=%d" % (n, guard)
            gx, gy = Guarded(cm, n, x, guard), Guarded(cm, n, y, guard)
            got = []
            for _ in range(2):
                work.set()
                out.set()
                call(cm, "cm2_dot", n, gx.ptr, gy.ptr, out.ptr, work.ptr)
                got.append(out.get())
            R.assert_bit_equal(got[0], got[1], what + " repeated")
            e = R.assert_within(got[0], ref, S, R.c_dot(n), what)
            print("%s: %.3f of the bound (c = %d)" % (what, e, R.c_dot(n)))
            all_intact(what, gx, gy, out, work)


@pytest.mark.parametrize("family", ["a", "b"])
def test_pcg_update_xr(cm, family):
    work, rr = reduce_work(cm), Guarded(cm, 1)
    rho_v, pq_v = 0.7, -1.9
    for n in N_REDUCE:
        p, q = vec_pair(family, n)
        x, r = vec_pair(family, n, seed=7)
        want_x, want_r = R.update_xr_f64(rho_v, pq_v, p, q, x, r)
        ref, S = R.update_xr_rr_ref(rho_v, pq_v, q, r)
        for guard in (ALIGNED, ODD):
            what = "update_xr n=%d guard=%d" % (n, guard)
            rho, pq = Guarded(cm, 1, [rho_v], guard), Guarded(cm, 1, [pq_v], guard)
            gp, gq = Guarded(cm, n, p, guard), Guarded(cm, n, q, guard)
            gx, gr = Guarded(cm, n, x, guard), Guarded(cm, n, r, guard)
            got = []
            for _ in range(2):
                work.set()
                rr.set()
                gx.set(x)
                gr.set(r)
                call(cm, "cm2_pcg_update_xr", n, rho.ptr, pq.ptr, gp.ptr, gq.ptr, gx.ptr, gr.ptr,
                     rr.ptr, work.ptr)
                got.append(rr.get())
                R.assert_bit_equal(gx.get(), want_x, what + " x")
                R.assert_bit_equal(gr.get(), want_r, what + " r")
            R.assert_bit_equal(got[0], got[1], what + " repeated")
            R.assert_within(got[0], ref, S, R.c_update_xr_rr(n), what + " rr")
            all_intact(what, rho, pq, gp, gq, gx, gr, rr, work)


# ================================================================== Z^T x, Z y, axpy ===
R_DEFLATION = (1, 5, 16, 17, 32, 48, 64, 200, 256)
N_ZT = (1, 3, 4095, 4096, 4097, 5003)
N_ZT_BODY_AND_TAIL = {16: 262144 + 37, 32: 131072 + 37, 64: 65536 + 37}


@pytest.mark.parametrize("r", R_DEFLATION)
def test_Zt_apply(cm, r):
    work, out = reduce_work(cm), Guarded(cm, r)
    sizes = N_ZT + ((N_ZT_BODY_AND_TAIL[r],) if r in N_ZT_BODY_AND_TAIL else ())
    for n in sizes:
        if r in N_ZT_BODY_AND_TAIL and n == N_ZT_BODY_AND_TAIL[r]:
            wide, rstep, rows, nblk = R.zt_plan(n, r, True)
            assert wide and rows >= 8 * rstep and rows % (8 * rstep) != 0 and n % rows % rstep != 0
        for family in ("a", "b"):
            Z, x = mat_vec(family, n, r)
            ref, S = R.zt_ref(Z, x)
            for guard in (ALIGNED, ODD):
                aligned = guard == ALIGNED
                what = "Zt r=%d n=%d family=%s guard=%d" % (r, n, family, guard)
                gZ, gx = Guarded(cm, n * r, Z, guard), Guarded(cm, n, x, guard)
                got = []
                for _ in range(2):
                    work.set()
                    out.set()
                    call(cm, "cm2_Zt_apply", n, r, gZ.ptr, gx.ptr, out.ptr, work.ptr)
                    got.append(out.get())
                R.assert_bit_equal(got[0], got[1], what + " repeated")
                R.assert_within(got[0], ref, S, R.c_zt(n, r, aligned), what)
                all_intact(what, gZ, gx, out, work)


@pytest.mark.parametrize("r", R_DEFLATION)
def test_Z_apply(cm, r):
    y = R.normals(77 + r, r)
    for n in N_ZT:
        Z, _ = mat_vec("a", n, r)
        want = R.z_apply_f64(Z, y)
        for guard in (ALIGNED, ODD):
            what = "Z_apply r=%d n=%d guard=%d" % (r, n, guard)
            gZ, gy, out = Guarded(cm, n * r, Z, guard), Guarded(cm, r, y, guard), Guarded(cm, n, None, guard)
            call(cm, "cm2_Z_apply", n, r, gZ.ptr, gy.ptr, out.ptr)
            R.assert_bit_equal(out.get(), want, what)
            all_intact(what, gZ, gy, out)


@pytest.mark.parametrize("r", [5, 16, 32, 64])
def test_Z_axpy(cm, r):
    y, alpha = R.normals(78 + r, r), -0.375 - 2.0 ** -33
    for n in (1, 3, 63, 64, 65, 4099):
        Z, w = mat_vec("a", n, r)
        ref, S = R.z_axpy_ref(Z, y, alpha, w)
        want = R.z_axpy_f64(Z, y, alpha, w)
        for guard in (ALIGNED, ODD):
            wide = guard == ALIGNED and r in (16, 32, 64)
            what = "Z_axpy r=%d n=%d guard=%d" % (r, n, guard)
            gZ, gy, gw = Guarded(cm, n * r, Z, guard), Guarded(cm, r, y, guard), Guarded(cm, n, w, guard)
            got = []
            for _ in range(2):
                gw.set(w)
                call(cm, "cm2_Z_axpy", n, r, gZ.ptr, gy.ptr, alpha, gw.ptr)
                got.append(gw.get())
            R.assert_bit_equal(got[0], got[1], what + " repeated")
            if wide:
                R.assert_within(got[0], ref, S, R.c_z_axpy(r, True), what)
            else:
                R.assert_bit_equal(got[0], want, what)
            all_intact(what, gZ, gy, gw)


def test_Z_axpy_grid_stride(cm):
    """the wide kernel has 16 x 256 workgroups at most; one more block of 64 rows than that"""
    torch = cm.torch
    r, n = 64, 4096 * 64 + 5
    gen = torch.Generator(device=cm.D.dev()).manual_seed(1234)
    gZ = Guarded(cm, n * r, torch.randn(n * r, generator=gen, dtype=torch.float64, device=cm.D.dev()))
    w0 = torch.randn(n, generator=gen, dtype=torch.float64, device=cm.D.dev())
    gw, y, alpha = Guarded(cm, n, w0), R.normals(79, r), 1.25
    gy = Guarded(cm, r, y)
    call(cm, "cm2_Z_axpy", n, r, gZ.ptr, gy.ptr, alpha, gw.ptr)
    ref, S = R.z_axpy_ref(gZ.get().reshape(n, r), y, alpha, w0.cpu().numpy())
    R.assert_within(gw.get(), ref, S, R.c_z_axpy(r, True), "Z_axpy grid stride")      # all n rows
    all_intact("Z_axpy grid stride", gZ, gy, gw)


# ===================================================================== E = Z1^T Z2 ===
N_GEMM = (1, 3, 4, 5, 2047, 2048, 2049, 24581)


@functools.lru_cache(maxsize=None)
def gemm_case(family, n, r1, r2):
    if family == "a":
        Z1, Z2 = R.normals(7000 + n + r1, n, r1), R.normals(8000 + n + r2, n, r2)
    else:
        Z1, Z2 = R.cancelling(9000 + n + r1 + r2, n, r1, r2)
    return (Z1, Z2) + R.gemm_tn_ref(Z1, Z2)


def _gemm_work(cm, r1, r2):
    return Guarded(cm, int(cm.hip.load().cm2_gemm_tn_work_doubles(r1, r2)))


@pytest.mark.parametrize("r1,r2,guard", [
    (16, 16, ALIGNED), (16, 16, ODD), (48, 48, ALIGNED), (48, 48, ODD),
    (32, 32, ALIGNED), (32, 32, ODD), (64, 64, ALIGNED), (64, 64, ODD),
    (5, 5, ALIGNED), (3, 7, ODD), (16, 32, ALIGNED), (64, 16, ALIGNED)],
    ids=lambda v: {ALIGNED: "aligned", ODD: "unaligned"}.get(v, str(v)))
def test_gemm_tn(cm, r1, r2, guard):
    work, E = _gemm_work(cm, r1, r2), Guarded(cm, r1 * r2)
    kinds = set()
    for n in N_GEMM:
        kind, chunk = R.gemm_tn_plan(n, r1, r2, guard == ALIGNED)
        kinds.add(kind)
        if kind == "pairs" and n == 24581:
            assert chunk == 16 and n % chunk == 5             # 1536 waves: unrolled body; one: tail, twice
        for family in ("a", "b"):
            Z1, Z2, ref, S = gemm_case(family, n, r1, r2)
            what = "gemm_tn %dx%d n=%d family=%s guard=%d (%s)" % (r1, r2, n, family, guard, kind)
            g1, g2 = Guarded(cm, n * r1, Z1, guard), Guarded(cm, n * r2, Z2, guard)
            got = []
            for _ in range(2):
                work.set()
                E.set()
                call(cm, "cm2_gemm_tn", n, r1, r2, g1.ptr, g2.ptr, E.ptr, work.ptr)
                got.append(E.get())
            R.assert_bit_equal(got[0], got[1], what + " repeated")
            R.assert_within(got[0], ref.reshape(-1), S.reshape(-1), R.c_gemm_tn(n, r1, r2, guard == ALIGNED), what)
            all_intact(what, g1, g2, E, work)
    assert len(kinds) == 1
    if r1 == r2:                                              # the same contraction through the class
        n = 2049
        Z1, Z2, ref, S = gemm_case("a", n, r1, r2)
        g1, g2 = Guarded(cm, n * r1, Z1, guard), Guarded(cm, n * r2, Z2, guard)
        co = cm.I.CoarseLO(g1.v.view(n, r1), g2.v.view(n, r2), r1)
        R.assert_within(co.E.reshape(-1), ref.reshape(-1), S.reshape(-1),
                        R.c_gemm_tn(n, r1, r2, guard == ALIGNED), "CoarseLO.E r=%d guard=%d" % (r1, guard))


# ================================================ panel gemm, small matvec, atbt, transpose ===
@pytest.mark.parametrize("rin,rout,guard", [(32, 16, ALIGNED), (32, 16, ODD), (32, 32, ALIGNED),
                                            (32, 32, ODD), (5, 3, ALIGNED)],
                         ids=lambda v: {ALIGNED: "aligned", ODD: "unaligned"}.get(v, str(v)))
def test_panel_gemm(cm, rin, rout, guard):
    mfma = rin == 32 and guard == ALIGNED
    W = R.normals(81, rin, rout)
    gW = Guarded(cm, rin * rout, W, guard)
    for n in (1, 15, 16, 17, 1000):
        P, out0 = R.normals(82 + n, n, rin), R.normals(83 + n, n, rout)
        gP = Guarded(cm, n * rin, P, guard)
        for accumulate in (0, 1):
            ref, S = R.panel_gemm_ref(P, W, out0 if accumulate else None)
            what = "panel_gemm %dx%d n=%d accumulate=%d guard=%d" % (rin, rout, n, accumulate, guard)
            out = Guarded(cm, n * rout, None, guard)
            got = []
            for _ in range(2):
                out.set(out0 if accumulate else None)
                call(cm, "cm2_panel_gemm", n, rin, rout, gP.ptr, gW.ptr, out.ptr, accumulate)
                got.append(out.get())
            R.assert_bit_equal(got[0], got[1], what + " repeated")
            R.assert_within(got[0], ref.reshape(-1), S.reshape(-1), R.c_panel_gemm(rin, mfma), what)
            all_intact(what, gP, gW, out)


@pytest.mark.parametrize("r", [1, 5, 32, 255, 256])
def test_small_matvec(cm, r):
    M, v = R.normals(84 + r, r, r), R.normals(85 + r, r)
    ref, S = R.matmul_ref(M, v)
    for guard in (ALIGNED, ODD):
        gM, gv, out = Guarded(cm, r * r, M, guard), Guarded(cm, r, v, guard), Guarded(cm, r, None, guard)
        got = []
        for _ in range(2):
            out.set()
            call(cm, "cm2_small_matvec", r, gM.ptr, gv.ptr, out.ptr)
            got.append(out.get())
        R.assert_bit_equal(got[0], got[1], "small_matvec repeated")
        R.assert_within(got[0], ref, S, R.c_serial(r), "small_matvec r=%d" % r)
        all_intact("small_matvec r=%d" % r, gM, gv, out)


@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (5, 7, 3), (32, 32, 40), (300, 4, 2)])
def test_gemm_atbt(cm, m, n, k):
    A, B = R.normals(86 + m, k, m), R.normals(87 + n, n, k)
    ref, S = R.gemm_atbt_ref(A, B)
    for guard in (ALIGNED, ODD):
        gA, gB, out = Guarded(cm, k * m, A, guard), Guarded(cm, n * k, B, guard), Guarded(cm, m * n, None, guard)
        got = []
        for _ in range(2):
            out.set()
            call(cm, "cm2_gemm_atbt", m, n, k, gA.ptr, gB.ptr, out.ptr)
            got.append(out.get())
        R.assert_bit_equal(got[0], got[1], "gemm_atbt repeated")
        R.assert_within(got[0], ref.reshape(-1), S.reshape(-1), R.c_serial(k), "gemm_atbt %r" % ((m, n, k),))
        all_intact("gemm_atbt", gA, gB, out)


@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (33, 31), (1000, 32), (32, 1000), (4099, 5)])
def test_transpose(cm, rows, cols):
    A = R.normals(88 + rows, rows, cols)
    for guard in (ALIGNED, ODD):
        gA, out = Guarded(cm, rows * cols, A, guard), Guarded(cm, rows * cols, None, guard)
        call(cm, "cm2_transpose", rows, cols, gA.ptr, out.ptr)
        R.assert_bit_equal(out.get().reshape(cols, rows), np.ascontiguousarray(A.T), "transpose %dx%d" % (rows, cols))
        all_intact("transpose", gA, out)


# ======================================================================== M2 tail ===
FIELDS = ("counts", "cosine", "sine", "cos2", "sin2", "sincos")


@functools.lru_cache(maxsize=None)
def weights(npix, shift):
    return R.pixel_weights(90 + npix, npix, shift)


def _device_weights(cm, W, guard=ALIGNED):
    return [Guarded(cm, W[f].size, W[f], guard) for f in FIELDS]


def _det_mask(cm, pol, npix, gW, W, what):
    """cm2_bd_det_mask on the device, compared bitwise with the restatement's rule before use"""
    det, mask = Guarded(cm, npix), Guarded(cm, npix, u8=True)
    call(cm, "cm2_bd_det_mask", pol, npix, *([g.ptr for g in gW] + [det.ptr, mask.ptr]))
    want_det, want_mask = R.det_mask_f64(pol, W)
    R.assert_bit_equal(det.get(), want_det, what + " det")
    assert (mask.get() == want_mask).all(), what + " mask"
    all_intact(what, det, mask)
    return det, mask, want_det, want_mask


@pytest.mark.parametrize("r", [5, 16, 32, 64])
@pytest.mark.parametrize("pol", [1, 2, 3])
def test_m2_finish(cm, pol, r):
    y = R.normals(91 + r, r)
    for npix in (1, 63, 64, 65, 127, 200, 4099):
        # a last partial block of one pixel cannot hold a masked and an unmasked one: both in turn
        for shift in ((0, 1) if npix % 64 == 1 else (0,)):
            W = weights(npix, shift)
            gW = _device_weights(cm, W)
            what0 = "m2_finish pol=%d r=%d npix=%d shift=%d" % (pol, r, npix, shift)
            det, mask, det_h, mask_h = _det_mask(cm, pol, npix, gW, W, what0)
            last = mask_h[(npix - 1) // 64 * 64:]
            assert npix % 64 == 1 or (last.min() == 0 and last.max() == 1)
            n = pol * npix
            Z, res = mat_vec("a", n, r)
            AZ = R.normals(92 + n + r, n, r)
            ref, S = R.m2_finish_ref(pol, Z, AZ, y, res, W, det_h, mask_h)
            want = R.m2_finish_f64(pol, Z, AZ, y, res, W, det_h, mask_h)
            masked = np.repeat(mask_h == 0, pol)
            R.assert_bit_equal(want[masked], 0.0 + R.z_apply_f64(Z, y)[masked], what0 + " restatement")
            for guard in (ALIGNED, ODD):
                wide = R.m2_is_wide(npix, r, guard == ALIGNED)
                what = what0 + " guard=%d" % guard
                gZ, gAZ = Guarded(cm, n * r, Z, guard), Guarded(cm, n * r, AZ, guard)
                gy, gres, out = Guarded(cm, r, y, guard), Guarded(cm, n, res, guard), Guarded(cm, n, None, guard)
                got = []
                for _ in range(2):
                    out.set()
                    call(cm, "cm2_m2_finish", pol, npix, r, gZ.ptr, gAZ.ptr, gy.ptr, gres.ptr,
                         *([g.ptr for g in gW] + [det.ptr, mask.ptr, out.ptr]))
                    got.append(out.get())
                R.assert_bit_equal(got[0], got[1], what + " repeated")
                if wide:
                    # (S of a masked pixel is that of Z y alone: nothing of res may show there)
                    R.assert_within(got[0], ref, S, R.c_m2(pol, r, True), what)
                else:
                    R.assert_bit_equal(got[0], want, what)
                all_intact(what, gZ, gAZ, gy, gres, out, det, mask, *gW)


def test_m2_finish_grid_stride(cm):
    """the wide kernel has 16 x 256 workgroups at most; two more 64-pixel blocks than that, the
    last of them partial"""
    torch = cm.torch
    pol, r, npix = 1, 16, 4096 * 64 + 70
    dev = cm.D.dev()
    gen = torch.Generator(device=dev).manual_seed(4321)
    gZ = Guarded(cm, npix * r, torch.randn(npix * r, generator=gen, dtype=torch.float64, device=dev))
    gAZ = Guarded(cm, npix * r, torch.randn(npix * r, generator=gen, dtype=torch.float64, device=dev))
    gres = Guarded(cm, npix, torch.randn(npix, generator=gen, dtype=torch.float64, device=dev))
    hits = torch.randint(0, 4, (npix,), generator=gen, device=dev).to(torch.float64)
    hits[-1], hits[-2] = 3.0, 0.0
    W = {f: (hits.cpu().numpy() if f == "counts" else np.zeros(npix)) for f in FIELDS}
    gW = [Guarded(cm, npix, hits)] + [Guarded(cm, npix, W[f]) for f in FIELDS[1:]]
    det, mask, det_h, mask_h = _det_mask(cm, pol, npix, gW, W, "m2 grid stride")
    y = R.normals(93, r)
    gy, out = Guarded(cm, r, y), Guarded(cm, npix)
    call(cm, "cm2_m2_finish", pol, npix, r, gZ.ptr, gAZ.ptr, gy.ptr, gres.ptr,
         *([g.ptr for g in gW] + [det.ptr, mask.ptr, out.ptr]))
    ref, S = R.m2_finish_ref(pol, gZ.get().reshape(npix, r), gAZ.get().reshape(npix, r), y, gres.get(), W,
                             det_h, mask_h)
    R.assert_within(out.get(), ref, S, R.c_m2(pol, r, True), "m2_finish grid stride")
    all_intact("m2_finish grid stride", gZ, gAZ, gres, gy, out, det, mask, *gW)


# ================================================ the whole operator, Python views ===
def test_two_level_operator(cm):
    """TwoLevelPreconditionerLO against M_BD (res - AZ y) + Z y, y = invE Z^T res in extended
    precision, within the sum of the three stages' bounds; once from aligned tensors (wide tail)
    and once from contiguous views at an odd element offset (the fallbacks)."""
    torch, I = cm.torch, cm.I
    pol, r, npix = 3, 32, 200
    n = pol * npix
    rng = np.random.default_rng(95)
    pix = np.tile(np.arange(npix), 16)
    phi = rng.uniform(0.0, np.pi, pix.size)
    ces = cm.U.ProcessTimeSamples(pix, npix, pol=pol, phi=phi)
    assert ces.get_new_pixel[0] == npix
    M = I.BlockDiagonalPreconditionerLO(ces, npix, pol=pol)
    W = {f: M._w.d[f].cpu().numpy() for f in FIELDS}
    det_h, mask_h = M._d_det.cpu().numpy(), M._d_mask.cpu().numpy()
    want_det, want_mask = R.det_mask_f64(pol, W)
    R.assert_bit_equal(det_h, want_det, "det")
    assert (mask_h == want_mask).all() and mask_h.all()
    Z, res = mat_vec("a", n, r)
    AZ = R.normals(96, n, r)
    y_in = R.normals(97, r)

    def tensors(odd):
        out = []
        for A in (Z, AZ):
            buf = torch.empty(n * r + 2, dtype=torch.float64, device=cm.D.dev())
            v = buf[1:1 + n * r].view(n, r) if odd else buf[:n * r].view(n, r)
            v.copy_(cm.D.f64(A))
            assert v.is_contiguous() and (v.data_ptr() & 15 != 0) == odd
            out.append(v)
        return out

    ref1, S1 = R.zt_ref(Z, res)
    refE, SE = R.gemm_tn_ref(Z, AZ)
    for odd in (False, True):
        what = "views at an odd offset" if odd else "aligned tensors"
        tZ, tAZ = tensors(odd)
        Zd, AZd = I.DeflationLO(tZ), I.DeflationLO(tAZ)
        assert Zd._d_Z.data_ptr() == tZ.data_ptr() and AZd._d_Z.data_ptr() == tAZ.data_ptr()
        E = I.CoarseLO(tZ, tAZ, r)
        R.assert_within(E.E.reshape(-1), refE.reshape(-1), SE.reshape(-1), R.c_gemm_tn(n, r, r, not odd),
                        what + ": CoarseLO.E")
        R.assert_bit_equal(Zd.mult(y_in), R.z_apply_f64(Z, y_in), what + ": DeflationLO.mult")
        R.assert_within(Zd.rmult(res), ref1, S1, R.c_zt(n, r, not odd), what + ": DeflationLO.rmult")
        # stage 1: y0 = Z^T res;  stage 2: y = invE y0 (invE is data: what the class holds);
        # stage 3: the tail.  An error dy of y moves the result by |M_BD| |AZ| dy + |Z| dy at most.
        invE = R._ld(E._d_inv.cpu().numpy().reshape(r, r))
        b1 = R.LD(R.c_zt(n, r, not odd)) * R.U53 * S1
        y_ref, S2 = invE @ ref1, np.abs(invE) @ S1
        dy = np.abs(invE) @ b1 + R.LD(R.c_serial(r)) * R.U53 * S2
        ref3, S3 = R.m2_finish_ref(pol, Z, AZ, y_ref, res, W, det_h, mask_h, ymag=S2)
        wide = R.m2_is_wide(npix, r, not odd)
        bound = R.LD(R.c_m2(pol, r, wide)) * R.U53 * S3 + R.m2_apply_abs(pol, Z, AZ, W, det_h, mask_h, dy)
        M2 = I.TwoLevelPreconditionerLO(M, Zd, AZd, E)
        got = M2.mult(cm.D.f64(res)).cpu().numpy()
        e = R.assert_within(got, ref3, bound / R.U53, 1, what + ": TwoLevelPreconditionerLO")
        print("%s: %.3f of the three stages' bound" % (what, e))
        R.assert_bit_equal(M2.mult(res), got, what + ": host vector in, host vector out")
