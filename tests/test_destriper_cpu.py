"""
Destriping without a GPU: the algebra of the baseline-offset system restated densely (_destriper_ref.py, whose
docstring has the definitions), the device-free arithmetic of cosmomap2_amd/csrc/cm2_offsets_policy.h compiled with
the host compiler, the argument checks of cosmomap2_amd.interfaces.destriper (which come before the device is
touched), and the new names in the C ABI and in the kernel resource table.

The common case: nt = 34002 = 4 * 8192 + 1234 in blocks of 14000 and 20002 samples with weights 1.0 and 2.5, nside 4
(192 pixels), uniformly random pixels and angles; flagged: 40 samples from every 400th starting at 123, all of window
3 and [13990, 14010) across the block boundary.  L = 37 / 1000 / 10000 gives 920 / 35 / 5 baselines of which
229 / 7 / 0 are empty.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as sla

import _destriper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
NPIX = 192

_cases = {}


def dense_case(L, pol, prior):
    key = (L, pol, prior)
    if key not in _cases:
        mask = R.common_flags()
        pix, phi = R.scan(R.NT, NPIX, mask, 11)
        rng = np.random.default_rng(12)
        sky = rng.standard_normal(pol * NPIX)
        B = R.baselines(R.SIZES, L)
        walk = np.cumsum(0.5 * rng.standard_normal(B.na))
        d = R.pointing(pix, phi, NPIX, pol) @ sky + walk[B.j_of_t] + rng.standard_normal(R.NT)
        d[mask] = 1e3                                        # what a flagged sample holds must not matter
        _cases[key] = R.system(R.SIZES, R.WEIGHTS, L, pix, phi, NPIX, pol, d, prior=prior)
    return _cases[key]


def test_the_common_case_has_the_stated_baselines():
    valid = ~R.common_flags()
    for L, na, empty in zip(R.LENGTHS, (920, 35, 5), (229, 7, 0)):
        B = R.baselines(R.SIZES, L)
        nvalid, wsum = R.counts(B, valid, R.WEIGHTS)
        assert (B.na, int((nvalid == 0).sum())) == (na, empty)
        assert nvalid.sum() == valid.sum() and B.per_block == [-(-n // L) for n in R.SIZES]


@pytest.mark.parametrize("pol", [1, 3])
@pytest.mark.parametrize("L", [37, 1000])
def test_schur_system_equals_the_joint_normal_equations(L, pol):
    s = dense_case(L, pol, True)
    m_j, a_j = R.joint_solve(s)
    a = np.linalg.solve(s.A, s.b)
    m = R.map_of(s, a)
    ea = np.linalg.norm(a - a_j) / np.linalg.norm(a_j)
    em = np.linalg.norm(m - m_j) / np.linalg.norm(m_j)
    print("\nL %d pol %d: Schur against joint, offsets %.3g, map %.3g" % (L, pol, ea, em))
    assert ea <= 1e-10 and em <= 1e-10, (ea, em)
    assert np.linalg.eigvalsh(s.A).min() > 0


@pytest.mark.parametrize("pol", [1, 3])
@pytest.mark.parametrize("L", R.LENGTHS)
def test_without_a_prior_the_constant_is_the_null_vector_and_the_residual_is_unique(L, pol):
    s = dense_case(L, pol, False)
    one = np.where(s.empty, 0.0, 1.0)
    assert np.linalg.norm(s.A @ one) <= 1e-12 * np.linalg.norm(s.wsum)
    assert np.all(s.b[s.empty] == 0.0)
    its = []
    a, info = sla.cg(s.A, s.b, M=np.diag(s.jac), rtol=1e-10, atol=0.0, callback=lambda xk: its.append(1))
    assert info == 0
    r_cg = (s.d0 - s.F @ a - s.P @ R.map_of(s, a))[s.valid]
    r_ls, _, _ = R.lstsq_residual(s)
    e = np.linalg.norm(r_cg - r_ls) / np.linalg.norm(r_ls)
    print("\nL %d pol %d: %d iterations, residual against lstsq %.3g" % (L, pol, len(its), e))
    assert e <= 1e-8, e
    assert np.all(a[s.empty] == 0.0)


# --------------------------------------------------------------------------- the policy header ------
DRIVER = r"""
#include "cm2_offsets_policy.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace cm2::offsets;
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "geometry")) {
        printf("%d %d %d %d\n", kWin, kChunk, kChunks, kWinPadded);
        for (int q = 0; q < kWin; ++q) printf("%d\n", pad(q));
        return 0;
    }
    // <what> L size0 size1 ...
    const int64_t L = atoll(argv[2]);
    std::vector<int64_t> off(1, 0), j0(1, 0);
    for (int i = 3; i < argc; ++i) {
        off.push_back(off.back() + atoll(argv[i]));
        j0.push_back(j0.back() + baselines_in(atoll(argv[i]), L));
    }
    const int64_t nb = (int64_t)off.size() - 1, nt = off.back(), nwin = (nt + kWin - 1) / kWin;
    if (!strcmp(argv[1], "samples")) {
        printf("%lld\n", (long long)j0.back());
        Baseline walk = baseline_of(off.data(), j0.data(), nb, L, 0);
        for (int64_t t = 0; t < nt; ++t) {
            const Baseline s = baseline_of(off.data(), j0.data(), nb, L, t);
            if (t >= walk.end) walk = next_baseline(off.data(), j0.data(), L, walk);
            if (walk.j != s.j || walk.start != s.start || walk.end != s.end || walk.b != s.b) return 3;
            if (block_of_baseline(j0.data(), nb, s.j) != s.b) return 4;
            printf("%lld %lld %lld %lld\n", (long long)s.j, (long long)s.start, (long long)s.end, (long long)s.b);
        }
    } else if (!strcmp(argv[1], "windows")) {
        printf("%lld %lld\n", (long long)nwin, (long long)side_slots(nwin));
        for (int64_t w = 0; w < nwin; ++w) {
            int64_t first, last;
            window_baselines(off.data(), j0.data(), nb, L, nt, w, &first, &last);
            Baseline s;
            const int comb = w >= 1 ? (combines_at(off.data(), j0.data(), nb, L, w, &s) ? 1 : 0) : 0;
            printf("%lld %lld %d %lld\n", (long long)first, (long long)last, comb, comb ? (long long)s.j : -1LL);
            Baseline g = baseline_of(off.data(), j0.data(), nb, L, w * kWin);
            for (int64_t j = first; j <= last; ++j) {
                const Target tg = segment_target(g.start, g.end, w * kWin);
                printf("%d %lld\n", (int)tg, tg == kDirect ? -1LL : (long long)side_slot(w, tg));
                if (j < last) g = next_baseline(off.data(), j0.data(), L, g);
            }
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("offsets_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]


def test_policy_geometry(driver):
    out = _run(driver, "geometry")
    assert out[0] == [8192, 32, 256, 8192 + 256]
    pad = np.array([r[0] for r in out[1:]])
    assert np.array_equal(pad, np.arange(8192) + np.arange(8192) // 32)
    assert len(set(pad.tolist())) == 8192 and pad.max() < 8192 + 256
    # the first samples of a wave's 64 chunks fall into 32 different pairs of 4-byte banks (an 8-byte access of 64
    # lanes takes two passes of 32)
    assert len({(2 * int(pad[32 * c])) % 64 for c in range(64)}) == 32


@pytest.mark.parametrize("name", sorted(R.LAYOUTS))
def test_policy_baseline_of_every_sample(driver, name):
    nt, sizes, _, L, _ = R.LAYOUTS[name]
    B = R.baselines(sizes, L)
    out = _run(driver, "samples", L, *sizes)
    assert out[0] == [B.na]
    got = np.array(out[1:])
    assert got.shape == (nt, 4)
    assert np.array_equal(got[:, 0], B.j_of_t)
    assert np.array_equal(got[:, 1], B.start[B.j_of_t]) and np.array_equal(got[:, 2], B.end[B.j_of_t])
    assert np.array_equal(got[:, 3], B.block[B.j_of_t])


@pytest.mark.parametrize("name", sorted(R.LAYOUTS))
def test_policy_windows_and_side_slots(driver, name):
    nt, sizes, _, L, _ = R.LAYOUTS[name]
    B = R.baselines(sizes, L)
    out = _run(driver, "windows", L, *sizes)
    nwin = -(-nt // R.WIN)
    assert out[0] == [nwin, 2 * nwin]
    at = 1
    finished = np.zeros(B.na, dtype=int)                     # every baseline is finished exactly once
    written, read = set(), []
    for w in range(nwin):
        first, last = R.window_baselines(B, nt, w)
        f, l, comb, cj = out[at]
        at += 1
        assert (f, l) == (first, last)
        crossing = w >= 1 and B.j_of_t[w * R.WIN] == B.j_of_t[w * R.WIN - 1]
        j = int(B.j_of_t[w * R.WIN])
        assert comb == (1 if crossing and B.start[j] >= (w - 1) * R.WIN else 0)
        if comb:
            assert cj == j
            finished[j] += 1
            read.append(2 * (w - 1) + 1)                     # the tail slot of the window it began in,
            v = w
            while v * R.WIN < B.end[j]:
                read.append(2 * v)                           # then the head slots in ascending window order
                v += 1
        for j in range(first, last + 1):
            tg, slot = out[at]
            at += 1
            want = R.segment_target(B.start[j], B.end[j], w * R.WIN)
            assert tg == want and slot == (-1 if want == 0 else 2 * w + (want - 1))
            if want == 0:
                finished[j] += 1
            else:
                assert slot not in written
                written.add(slot)
    assert at == len(out)
    assert np.all(finished == 1)
    assert sorted(read) == sorted(written) and len(set(read)) == len(read)      # every slot written is read once
    if name == "windows":
        assert not written                                   # baselines equal windows: nothing crosses
    if name == "common10000":
        assert written


# -------------------------------------------------------------------------- argument checks ------
ASIZES = [1000, 2000]
ANT = sum(ASIZES)


@pytest.fixture
def ds():
    from cosmomap2_amd.interfaces import destriper
    return destriper


@pytest.fixture
def no_gpu(monkeypatch):
    """As on a machine without a GPU, whether or not this one has one."""
    from cosmomap2_amd import device as D
    monkeypatch.setattr(D, "gpu_available", lambda: False)


def sparse_lo(nt=ANT, npix=48, pol=3):
    """A SparseLO as far as the argument checks look at it."""
    from cosmomap2_amd.interfaces.linearoperators import SparseLO
    P = SparseLO.__new__(SparseLO)
    P.nrows, P.ncols, P.pol = nt, npix, pol
    return P


def mbd(npix=48, pol=3):
    """A BlockDiagonalPreconditionerLO as far as the argument checks look at it."""
    from cosmomap2_amd import linop as lp
    from cosmomap2_amd.interfaces.linearoperators import BlockDiagonalPreconditionerLO
    M = BlockDiagonalPreconditionerLO.__new__(BlockDiagonalPreconditionerLO)
    lp.LinearOperator.__init__(M, pol * npix, pol * npix, lambda x: x, symmetric=True)
    M.pol = pol
    return M


def offsets_lo(ds, P, na=90):
    F = ds.OffsetsLO.__new__(ds.OffsetsLO)
    F.P, F.na, F.nt = P, na, P.nrows
    return F


def test_exported_from_interfaces():
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd.interfaces import destriper
    for name in ("OffsetsLO", "DestriperNormalLO", "solve_destriped"):
        assert getattr(I, name) is getattr(destriper, name)


def test_offsets_arguments(ds, no_gpu):
    P = sparse_lo()
    for bad in (None, np.eye(3)):
        with pytest.raises(ValueError, match="SparseLO"):
            ds.OffsetsLO(bad, ASIZES, 100)
    for blocksize in (7, [1000, 1999], [1000, -5, 2005], [], 0, 2.5):
        with pytest.raises(ValueError, match="blocksize"):
            ds.OffsetsLO(P, blocksize, 100)
    for L in (0, -3, 2.5, "10", None, True):
        with pytest.raises(ValueError, match="baseline_length"):
            ds.OffsetsLO(P, ASIZES, L)
    for w in ([1.0], [1.0, 2.0, 3.0], [1.0, 0.0], [1.0, -2.0], [1.0, np.nan], [np.inf, 1.0], [[1.0, 2.0]], "ab"):
        with pytest.raises(ValueError, match="weights"):
            ds.OffsetsLO(P, ASIZES, 100, weights=w)
    with pytest.raises(ValueError, match="32-bit"):
        ds.OffsetsLO(sparse_lo(nt=2 ** 32 - 1), 2 ** 32 - 1, 100)
    with pytest.raises(ValueError, match="31-bit"):
        ds.OffsetsLO(sparse_lo(nt=2 ** 31), 2 ** 31, 1)


def test_normal_operator_arguments(ds, no_gpu):
    P = sparse_lo()
    F = offsets_lo(ds, P)
    with pytest.raises(ValueError, match="SparseLO"):
        ds.DestriperNormalLO(None, F, mbd())
    with pytest.raises(ValueError, match="OffsetsLO"):
        ds.DestriperNormalLO(P, np.eye(3), mbd())
    with pytest.raises(ValueError, match="another pointing"):
        ds.DestriperNormalLO(sparse_lo(), F, mbd())
    for M in (None, np.eye(144), mbd(npix=47), mbd(pol=1)):
        with pytest.raises(ValueError, match="Mbd"):
            ds.DestriperNormalLO(P, F, M)
    for prior in (np.eye(89), 3.0, mbd()):
        with pytest.raises(ValueError, match="prior"):
            ds.DestriperNormalLO(P, F, mbd(), prior=prior)


def test_solve_arguments(ds, no_gpu):
    P, M, d = sparse_lo(), mbd(), np.zeros(ANT)
    na = 10 + 20                                             # L = 100
    for bad in (np.zeros(ANT - 1), np.zeros((ANT, 1)), np.zeros(ANT, dtype=complex)):
        with pytest.raises(ValueError, match="samples|TOD"):
            ds.solve_destriped(P, ASIZES, 100, bad, M)
    with pytest.raises(ValueError, match="Mbd"):
        ds.solve_destriped(P, ASIZES, 100, d, None)
    with pytest.raises(ValueError, match="baseline_length"):
        ds.solve_destriped(P, ASIZES, 0, d, M)
    with pytest.raises(ValueError, match="weights"):
        ds.solve_destriped(P, ASIZES, 100, d, M, weights=[1.0])
    with pytest.raises(ValueError, match="prior"):
        ds.solve_destriped(P, ASIZES, 100, d, M, prior=np.eye(na + 1))
    for rtol in (0.0, -1e-8, np.nan, np.inf, "x", None):
        with pytest.raises(ValueError, match="rtol"):
            ds.solve_destriped(P, ASIZES, 100, d, M, rtol=rtol)
    for maxiter in (0, -3, 2.5, "10"):
        with pytest.raises(ValueError, match="maxiter"):
            ds.solve_destriped(P, ASIZES, 100, d, M, maxiter=maxiter)
    for x0 in (np.zeros(na - 1), np.zeros((na, 1)), 1.0):
        with pytest.raises(ValueError, match="x0"):
            ds.solve_destriped(P, ASIZES, 100, d, M, x0=x0)
    with pytest.raises(ValueError, match="callback"):
        ds.solve_destriped(P, ASIZES, 100, d, M, callback=3)


def test_valid_calls_raise_hip_error_without_a_gpu(ds, no_gpu):
    from cosmomap2_amd import _hip
    P, M, d = sparse_lo(), mbd(), np.zeros(ANT)
    for call in (lambda: ds.OffsetsLO(P, ASIZES, 100),
                 lambda: ds.OffsetsLO(P, 1500, 1, weights=[1.0, 2.5]),
                 lambda: ds.DestriperNormalLO(P, offsets_lo(ds, P), M, prior=np.eye(90)),
                 lambda: ds.solve_destriped(P, ASIZES, 100, d, M),
                 lambda: ds.solve_destriped(P, ASIZES, 100, d, M, weights=[1.0, 2.5], prior=np.eye(30), rtol=1e-10,
                                            maxiter=50, x0=np.zeros(30), callback=lambda a: None)):
        with pytest.raises(_hip.HipError):
            call()


# ------------------------------------------------------------------------------ the C ABI ------
NEW = ("cm2_offsets_create", "cm2_offsets_destroy", "cm2_offsets_info", "cm2_offsets_counts", "cm2_offsets_expand",
       "cm2_offsets_residual", "cm2_offsets_sum", "cm2_offsets_prepare_tiles", "cm2_offsets_to_tiles",
       "cm2_offsets_from_tiles")
NOT_RESTARTABLE = ("cm2_offsets_destroy", "cm2_offsets_info", "cm2_offsets_counts")
KERNELS = ("k_offsets_expand", "k_offsets_residual", "k_offsets_sum", "k_offsets_to_tiles", "k_offsets_from_tiles",
           "k_offsets_combine", "k_offsets_count", "k_offsets_wsum", "k_offsets_compare")


def test_abi_lists_name_the_new_entry_points():
    from cosmomap2_amd import _hip, kernel_resources as KR
    text = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    assert re.search(r"#define CM2_ABI_VERSION 2\b", text)
    for name in NEW:
        assert name in _hip.PROTOTYPES, name
        m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_hip.PROTOTYPES[name]), name
        assert (name in _hip.RESTARTABLE) == (name not in NOT_RESTARTABLE), name
    for kernel in KERNELS:
        assert any(re.search(p, kernel) for p in KR.NO_SPILL), kernel


def test_new_entry_points_refuse_null_arguments():
    """Their argument checks come before the first HIP call: no GPU is needed to meet them."""
    import ctypes
    from cosmomap2_amd import _hip
    lib = _hip.load()
    nargs = {name: len(_hip.PROTOTYPES[name]) for name in NEW}
    for name in NEW:
        if name == "cm2_offsets_destroy":
            assert lib.cm2_offsets_destroy(None) == 0
            continue
        args = [0 if a in (ctypes.c_int, ctypes.c_int64) else None for a in _hip.PROTOTYPES[name]]
        assert len(args) == nargs[name]
        assert getattr(lib, name)(*args) == _hip.ERR_ARGUMENT, name
        assert name.encode() in lib.cm2_last_error(), (name, lib.cm2_last_error())


def test_create_refuses_bad_arguments_before_the_device():
    import ctypes
    from cosmomap2_amd import _hip
    lib = _hip.load()
    h = ctypes.c_void_p()
    pix = ctypes.c_void_p(4096)                              # never read: every call below is refused first

    def create(nt, sizes, L, w=None):
        sz = (ctypes.c_int64 * len(sizes))(*sizes)
        pw = None if w is None else (ctypes.c_double * len(w))(*w)
        rc = lib.cm2_offsets_create(ctypes.byref(h), pix, nt, sz, len(sizes), L, pw, None)
        return rc, lib.cm2_last_error()

    for args, word in (((2 ** 32 - 1, [2 ** 32 - 1], 10), b"32-bit"), ((2 ** 31, [2 ** 31], 1), b"31-bit"),
                       ((100, [100], 0), b"baseline_length"), ((100, [60, 30], 10), b"add up"),
                       ((100, [60, 50], 10), b"add up"), ((100, [100, 0], 10), b"non-positive"),
                       ((0, [1], 10), b"nt="), ((100, [60, 40], 10, [1.0, 0.0]), b"weight"),
                       ((100, [60, 40], 10, [float("nan"), 1.0]), b"weight")):
        rc, msg = create(*args)
        assert rc == _hip.ERR_ARGUMENT and b"cm2_offsets_create" in msg and word in msg, (args, rc, msg)
        assert not h.value


def test_new_kernels_use_no_scratch():
    """The resource table of the shipped objects lists the new kernels without scratch or spilled registers; the
    window kernels hold the padded window and the 256 partial sums and flags of the scan in dynamic LDS."""
    from cosmomap2_amd import build as B, kernel_resources as KR
    B.build(verbose=False)
    rows = {r["kernel"]: r for r in KR.load_all()}
    for kernel in KERNELS:
        assert kernel in rows, sorted(rows)
        assert rows[kernel].get("scratch_bytes_per_lane", 0) == 0, rows[kernel]
        assert rows[kernel].get("vgpr_spill", 0) == 0, rows[kernel]
    assert not KR.offenders(list(rows.values()))
    table = open(os.path.join(ROOT, "profiles", "kernel_resources.md")).read()
    for kernel in KERNELS:
        assert "`%s`" % kernel in table, kernel
