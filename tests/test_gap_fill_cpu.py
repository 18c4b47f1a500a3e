"""
cosmomap2_amd.utilities.gap_fill without a GPU: every bad argument is refused with ValueError before the
device is touched, a valid call raises HipError when there is no GPU, and the new entry points and kernels are
listed where the build and the binding look for them.
"""
import os
import re
import shutil

import numpy as np
import pytest

SIZES = [1000, 2000]
NT = sum(SIZES)
BANDS = [np.array([2.0, -0.5, 0.1]), np.array([1.0, -0.2, 0.05])]


@pytest.fixture
def gf():
    from cosmomap2_amd.utilities import gap_fill
    return gap_fill


@pytest.fixture
def no_gpu(monkeypatch):
    """As on a machine without a GPU, whether or not this one has one."""
    from cosmomap2_amd import device as D
    monkeypatch.setattr(D, "gpu_available", lambda: False)


def block_lo(sizes=SIZES, t=BANDS, offdiag=True):
    """A BlockLO as its constructor leaves it on the host side (the constructor itself needs the GPU)."""
    from cosmomap2_amd.interfaces.linearoperators import BlockLO
    N = BlockLO.__new__(BlockLO)
    N._BlockLO__isoffdiag = offdiag
    N.blocksize, N.covnoise, N._sizes, N._nt = sizes, t, list(sizes), sum(sizes)
    return N


def simulator(sizes):
    """A NoiseSimulator as far as the argument checks look at it."""
    from cosmomap2_amd.utilities.noise_sim import NoiseSimulator
    sim = NoiseSimulator.__new__(NoiseSimulator)
    sim.sizes, sim.nt, sim.h = list(sizes), sum(sizes), None
    return sim


class _Ready(object):
    """A GapFiller past its constructor (which needs the GPU): fill()'s own checks."""

    def __new__(cls, gf):
        g = gf.GapFiller.__new__(gf.GapFiller)
        g.sizes, g.nt, g.ng = list(SIZES), NT, 5
        return g


def flags_i32():
    pix = np.arange(NT, dtype=np.int32)
    pix[10:20] = -1
    return pix


def test_exported_from_utilities():
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd.utilities import gap_fill
    for name in ("GapFiller", "fill_gaps_linear"):
        assert getattr(U, name) is getattr(gap_fill, name)


@pytest.mark.parametrize("n", [NT - 1, NT + 1, 0])
def test_flags_of_the_wrong_length(gf, no_gpu, n):
    with pytest.raises(ValueError, match="flags|samples"):
        gf.GapFiller(np.zeros(n, dtype=np.int32), block_lo())
    with pytest.raises(ValueError, match="flags|samples"):
        gf.fill_gaps_linear(np.zeros(NT), np.zeros(n, dtype=bool), SIZES)


@pytest.mark.parametrize("flags", [np.zeros(NT), np.zeros(NT, dtype=np.uint32), np.zeros((NT, 1), dtype=bool),
                                   np.zeros((2, NT // 2), dtype=np.int32)])
def test_flags_of_the_wrong_kind(gf, no_gpu, flags):
    with pytest.raises(ValueError, match="flags"):
        gf.GapFiller(flags, block_lo())
    with pytest.raises(ValueError, match="flags"):
        gf.fill_gaps_linear(np.zeros(NT), flags, SIZES)


def test_noise_that_is_not_a_toeplitz_blocklo(gf, no_gpu):
    for N in (block_lo(t=[1.0, 2.0], offdiag=False), None, np.eye(3), "N"):
        with pytest.raises(ValueError, match="Toeplitz BlockLO"):
            gf.GapFiller(flags_i32(), N)
    with pytest.raises(ValueError, match="a_0"):
        gf.GapFiller(flags_i32(), block_lo(t=[np.array([1.0, 0.1]), np.array([0.0, 0.1])]))


@pytest.mark.parametrize("d", [np.zeros(NT - 1), np.zeros(NT + 1), np.zeros((NT, 1)), np.zeros(NT, dtype=complex)])
def test_stream_of_the_wrong_length(gf, no_gpu, d):
    with pytest.raises(ValueError, match="samples|TOD"):
        _Ready(gf).fill(d)
    with pytest.raises(ValueError, match="samples|TOD"):
        gf.fill_gaps_linear(d, flags_i32(), SIZES)


@pytest.mark.parametrize("blocksize", [[1000, 1999], [NT, 1], 7, 0, [], [1500.0, 1500.0]])
def test_blocks_that_do_not_add_up(gf, no_gpu, blocksize):
    with pytest.raises(ValueError, match="blocksize"):
        gf.fill_gaps_linear(np.zeros(NT), flags_i32(), blocksize)


@pytest.mark.parametrize("sizes", [[2000, 1000], [NT], [1000, 1000, 1000], [1000, 2001]])
def test_simulator_of_another_shape(gf, no_gpu, sizes):
    with pytest.raises(ValueError, match="simulator"):
        _Ready(gf).fill(np.zeros(NT), sim=simulator(sizes))
    with pytest.raises(ValueError, match="NoiseSimulator"):
        _Ready(gf).fill(np.zeros(NT), sim="sim")


@pytest.mark.parametrize("nedge", [0, -1, 1.5, "32", None, True])
def test_nedge_below_one(gf, no_gpu, nedge):
    with pytest.raises(ValueError, match="nedge"):
        gf.fill_gaps_linear(np.zeros(NT), flags_i32(), SIZES, nedge=nedge)


@pytest.mark.parametrize("rtol", [0.0, -1e-8, np.nan, np.inf, "x", None])
def test_rtol_not_positive(gf, no_gpu, rtol):
    with pytest.raises(ValueError, match="rtol"):
        _Ready(gf).fill(np.zeros(NT), rtol=rtol)


def test_other_bad_fill_arguments(gf, no_gpu):
    for maxiter in (0, -3, 2.5, "10"):
        with pytest.raises(ValueError, match="maxiter"):
            _Ready(gf).fill(np.zeros(NT), maxiter=maxiter)
    for realization in (-1, 1 << 64, 1.0, None):
        with pytest.raises(ValueError, match="realization"):
            _Ready(gf).fill(np.zeros(NT), realization=realization)


@pytest.mark.parametrize("out", [np.zeros(NT - 1), np.zeros(NT, dtype=np.float32), np.zeros(NT, dtype=np.int64),
                                 np.zeros(2 * NT)[::2], np.zeros((3, NT // 3)), [0.0] * NT, "out"])
def test_out_of_the_wrong_length_or_dtype(gf, no_gpu, out):
    with pytest.raises(ValueError, match="out"):
        _Ready(gf).fill(np.zeros(NT), out=out)
    with pytest.raises(ValueError, match="out"):
        gf.fill_gaps_linear(np.zeros(NT), flags_i32(), SIZES, out=out)


def test_tensors_that_are_not_float64_in_hbm(gf, no_gpu):
    torch = pytest.importorskip("torch")
    for out in (torch.zeros(NT, dtype=torch.float64), torch.zeros(NT, dtype=torch.float32)):
        with pytest.raises(ValueError, match="out"):
            _Ready(gf).fill(np.zeros(NT), out=out)
        with pytest.raises(ValueError, match="out"):
            gf.fill_gaps_linear(np.zeros(NT), flags_i32(), SIZES, out=out)
    with pytest.raises(ValueError, match="HBM"):
        gf.fill_gaps_linear(torch.zeros(NT, dtype=torch.float64), flags_i32(), SIZES)
    with pytest.raises(ValueError, match="float64"):
        gf.fill_gaps_linear(torch.zeros(NT, dtype=torch.float32), flags_i32(), SIZES)
    with pytest.raises(ValueError, match="flags"):
        gf.fill_gaps_linear(np.zeros(NT), torch.zeros(NT, dtype=torch.float64), SIZES)


def test_valid_calls_raise_hip_error_without_a_gpu(gf, no_gpu):
    from cosmomap2_amd import _hip
    d = np.zeros(NT)
    for call in (lambda: gf.GapFiller(flags_i32(), block_lo()),
                 lambda: gf.GapFiller(flags_i32() < 0, block_lo()),
                 lambda: gf.GapFiller(flags_i32().astype(np.int64), block_lo()),
                 lambda: gf.fill_gaps_linear(d, flags_i32(), SIZES),
                 lambda: gf.fill_gaps_linear(d, flags_i32() < 0, 500, nedge=1, out=np.zeros(NT)),
                 lambda: _Ready(gf).fill(d),
                 lambda: _Ready(gf).fill(d, sim=simulator(SIZES), realization=(1 << 64) - 1, rtol=1e-10, maxiter=500,
                                         out=np.zeros(NT))):
        with pytest.raises(_hip.HipError):
            call()


NEW = ("cm2_gaps_create", "cm2_gaps_destroy", "cm2_gaps_info", "cm2_gaps_index", "cm2_gaps_gather",
       "cm2_gaps_scatter", "cm2_gaps_normal_apply", "cm2_gaps_precond_apply", "cm2_gaps_masked_diff", "cm2_gaps_rhs",
       "cm2_gaps_finish", "cm2_gaps_fill_linear")
KERNELS = ("k_gap_gather", "k_gap_scatter", "k_gap_masked_diff<0>", "k_gap_masked_diff<1>", "k_gap_finish",
           "k_gap_edges<0>", "k_gap_edges<1>", "k_gap_interp", "k_gap_copy_valid<0>", "k_gap_copy_valid<1>")


def test_abi_lists_name_the_new_entry_points():
    from cosmomap2_amd import _hip, kernel_resources as KR
    for name in NEW:
        assert name in _hip.PROTOTYPES, name
    for name in ("cm2_gaps_destroy", "cm2_gaps_info", "cm2_gaps_index"):
        assert name not in _hip.RESTARTABLE
    for name in ("cm2_gaps_create", "cm2_gaps_gather", "cm2_gaps_scatter", "cm2_gaps_normal_apply",
                 "cm2_gaps_masked_diff", "cm2_gaps_finish", "cm2_gaps_fill_linear"):
        assert name in _hip.RESTARTABLE, name
    for kernel in KERNELS:
        assert any(re.search(p, kernel) for p in KR.NO_SPILL), kernel


def test_create_refuses_what_does_not_fit_32_bit_positions():
    """The argument checks of cm2_gaps_create come before its first HIP call: no GPU is needed to meet them."""
    import ctypes
    from cosmomap2_amd import _hip
    lib = _hip.load()
    h = ctypes.c_void_p()
    flags = (ctypes.c_int32 * 4)()                           # never read: every call below is refused first
    for nt, kind, sizes in (((1 << 32) - 1, 0, [(1 << 32) - 1]), (1 << 33, 1, [1 << 32, 1 << 32]), (0, 0, [1]),
                            (4, 2, [4]), (4, -1, [4]), (4, 0, [])):
        sz = (ctypes.c_int64 * max(len(sizes), 1))(*sizes)
        rc = lib.cm2_gaps_create(ctypes.byref(h), ctypes.addressof(flags), kind, nt, sz, len(sizes), None, None)
        assert rc == _hip.ERR_ARGUMENT and not h.value, (nt, kind, sizes, rc)
        assert b"cm2_gaps_create" in lib.cm2_last_error()
    assert lib.cm2_gaps_destroy(None) == 0


def test_header_declares_what_the_binding_lists():
    from cosmomap2_amd import _hip
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "cosmomap2.h")).read()
    assert re.search(r"#define CM2_ABI_VERSION 2\b", text)
    for name in NEW:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_hip.PROTOTYPES[name]), name


def test_library_cross_compiles_with_no_scratch_in_the_new_kernels():
    """python -m cosmomap2_amd.build for gfx950 (a no-op when the library is up to date), then the resource
    table of the shipped objects: the new kernels are there and use no scratch."""
    from cosmomap2_amd import build as B, kernel_resources as KR
    if not (os.path.exists(B.HIPCC) or shutil.which(B.HIPCC)):
        pytest.fail("hipcc not found at %s: the library cannot be built" % B.HIPCC)
    B.build(verbose=False)
    rows = {r["kernel"]: r for r in KR.load_all()}
    for kernel in KERNELS:
        assert kernel in rows, sorted(rows)
        assert rows[kernel].get("scratch_bytes_per_lane", 0) == 0, rows[kernel]
        assert rows[kernel].get("vgpr_spill", 0) == 0, rows[kernel]
    assert KR.offenders(list(rows.values())) == []
