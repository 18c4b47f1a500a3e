"""
The order-independent ground-bin sums without a GPU: the float64 limb recipe against exact rational arithmetic, the
restatement of _ground_exact_ref.py against math.fsum, the device-free arithmetic of
cosmomap2_amd/csrc/cm2_ground_exact_policy.h compiled with the host compiler, the refusals of the new entry points
(which come before the device is touched) and the new names in the C ABI and in the kernel resource table.

The common case: nt = 20001 samples in 64 bins, labels in [-1, 64).
"""
import ctypes
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ground_exact_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
NT, NBINS = 20001, 64


# ------------------------------------------------------------------ the arithmetic ------
@pytest.mark.parametrize("kind", R.KINDS)
def test_limb_recipe_is_the_exact_truncation(kind):
    """l0 2^64 + l1 2^32 + l2 == trunc(v 2^(95-e)) sample by sample, |l_k| < 2^32, the limbs carry v's sign"""
    g, v = R.case(kind, NT, NBINS)
    M = R.scale_word(g, v, NBINS)
    if kind == "zeros":
        assert M == 0
        assert (R.bits(R.exact_sums(g, v, NBINS)) == 0).all()            # +0.0, not -0.0
        return
    e = R.exponent(M)
    x = v[R.counted(g, NBINS)]
    assert np.abs(x).max() < math.ldexp(1.0, e + 1) and np.abs(x).max() >= math.ldexp(1.0, e)
    ls = R.limbs(x, e)
    for l in ls:
        assert np.abs(l).max() < 2 ** 32
        assert (np.sign(l) * np.sign(x) >= 0).all()
    assert R.joined(*ls) == R.truncated(x, e)
    if kind == "wide":
        assert all(np.count_nonzero(l) > 100 for l in ls)               # every limb is exercised
        assert np.count_nonzero(np.ldexp(x, 95 - e) != np.trunc(np.ldexp(x, 95 - e))) > 100   # and the truncation


@pytest.mark.parametrize("kind", R.KINDS)
def test_sums_do_not_depend_on_the_order_of_the_samples(kind):
    g, v = R.case(kind, NT, NBINS)
    p = np.random.default_rng(3).permutation(NT)
    assert (R.bits(R.exact_sums(g, v, NBINS)) == R.bits(R.exact_sums(g[p], v[p], NBINS))).all()


@pytest.mark.parametrize("kind", R.KINDS)
def test_sums_are_within_the_stated_error_of_fsum(kind):
    """|sum - fsum| <= half an ulp of the sum + hits 2^(e-95), bin by bin, in exact arithmetic"""
    g, v = R.case(kind, NT, NBINS)
    got = R.exact_sums(g, v, NBINS)
    M = R.scale_word(g, v, NBINS)
    delta = Fraction(2) ** (R.exponent(M) - 95) if M else Fraction(0)
    for b in range(NBINS):
        x = v[g == b]
        err = abs(Fraction(float(got[b])) - Fraction(math.fsum(x.tolist())))
        assert err <= Fraction(math.ulp(float(got[b]))) / 2 + x.size * delta, (kind, b, float(err))


def test_a_dropped_limb_is_caught_on_the_wide_case():
    g, v = R.case("wide", NT, NBINS)
    e = R.exponent(R.scale_word(g, v, NBINS))
    x = v[R.counted(g, NBINS)]
    assert R.joined(*R.limbs_without_l2(x, e)) != R.truncated(x, e)
    assert R.integer_sums(g, v, NBINS, R.limbs_without_l2)[1] != R.integer_sums(g, v, NBINS)[1]


def test_nan_poisons_every_bin_only_when_it_is_counted():
    g, v = R.case("normal", 999, 7, beyond=True)
    want = R.exact_sums(g, v, 7)
    for label in (-1, 7, 2 ** 31 - 1):
        g2, v2 = g.copy(), v.copy()
        g2[5], v2[5] = label, np.nan
        g1 = g.copy()
        g1[5] = label
        assert (R.bits(R.exact_sums(g2, v2, 7)) == R.bits(R.exact_sums(g1, v, 7))).all()
    v3 = v.copy()
    g3 = g.copy()
    g3[5], v3[5] = 3, np.inf
    assert np.isnan(R.exact_sums(g3, v3, 7)).all() and not np.isnan(want).any()


# ------------------------------------------- the device-free arithmetic of the kernels ------
DRIVER = r"""
#include "cm2_ground_exact_policy.h"
#include <cstdio>
#include <vector>
namespace gs = cm2::gsum;
// in: int64 nt, int64 nbins, int32 g[nt], double v[nt]; out: double sums[nbins], as the kernels form them
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t nt = 0, nbins = 0;
    if (fread(&nt, 8, 1, f) != 1 || fread(&nbins, 8, 1, f) != 1) return 2;
    std::vector<int32_t> g(nt);
    std::vector<double> v(nt);
    if (nt && (fread(g.data(), 4, nt, f) != (size_t)nt || fread(v.data(), 8, nt, f) != (size_t)nt)) return 2;
    fclose(f);
    uint64_t M = 0;
    for (int64_t i = 0; i < nt; ++i)
        if ((uint32_t)g[i] < (uint32_t)nbins && gs::abs_bits(v[i]) > M) M = gs::abs_bits(v[i]);
    std::vector<uint64_t> L(3 * nbins, 0);
    const gs::Kind kind = gs::kind_of(M);
    const int e = gs::exponent_of(M);
    if (kind == gs::kFinite)
        for (int64_t i = nt - 1; i >= 0; --i) {
            if ((uint32_t)g[i] >= (uint32_t)nbins) continue;
            int64_t l[3];
            gs::limbs(v[i], e, l);
            for (int k = 0; k < 3; ++k) L[k * nbins + g[i]] += (uint64_t)l[k];
        }
    std::vector<double> sums(nbins);
    for (int64_t b = 0; b < nbins; ++b)
        sums[b] = kind == gs::kZero ? 0.0 : kind == gs::kPoisoned ? gs::from_bits(gs::kNanBits)
                  : gs::round_sum((int64_t)L[b], (int64_t)L[nbins + b], (int64_t)L[2 * nbins + b], e);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(sums.data(), 8, nbins, f) != (size_t)nbins) return 2;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("ground_exact_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, str(src),
                           "-o", exe])
    return lambda g, v, nbins: _run(exe, d, g, v, nbins)


def _run(exe, d, g, v, nbins):
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.array([len(g), nbins], dtype=np.int64).tobytes())
        fh.write(np.ascontiguousarray(g, dtype=np.int32).tobytes())
        fh.write(np.ascontiguousarray(v, dtype=np.float64).tobytes())
    subprocess.run([exe, fin, fout], check=True)
    return np.fromfile(fout, dtype=np.float64)


@pytest.mark.parametrize("kind", R.KINDS)
def test_policy_header_gives_the_reference_bits(driver, kind):
    g, v = R.case(kind, NT, NBINS, beyond=True)
    assert (R.bits(driver(g, v, NBINS)) == R.bits(R.exact_sums(g, v, NBINS))).all()


def test_policy_header_rounds_ties_to_even_and_carries(driver):
    """one bin each: a tie below an even and below an odd mantissa, a remainder just above and just below half, a
    mantissa of all ones that rounds up to 2^53, a negative sum, and a sum of few bits"""
    rows = [[1.0, 2.0 ** -53], [1.0 + 2.0 ** -52, 2.0 ** -53], [1.0, 2.0 ** -53, 2.0 ** -90],
            [1.0, 2.0 ** -53, -2.0 ** -90], [2.0 - 2.0 ** -52, 2.0 ** -53], [-1.0, -2.0 ** -53, -2.0 ** -80],
            [1.5, -1.5, 2.0 ** -60], [1.75, 0.25]]
    g = np.concatenate([np.full(len(r), b) for b, r in enumerate(rows)]).astype(np.int32)
    v = np.concatenate(rows)
    want = R.exact_sums(g, v, len(rows))
    assert want[0] == 1.0 and want[1] == 1.0 + 2.0 ** -51 and want[2] == 1.0 + 2.0 ** -52 and want[3] == 1.0
    assert want[4] == 2.0 and want[5] == -1.0 - 2.0 ** -52 and want[6] == 2.0 ** -60 and want[7] == 2.0
    assert (R.bits(driver(g, v, len(rows))) == R.bits(want)).all()


def test_policy_header_poisons_and_zeroes(driver):
    g, v = R.case("normal", 999, 7)
    v[5], g[5] = np.nan, 3
    assert np.isnan(driver(g, v, 7)).all()
    g[5] = -1
    assert (R.bits(driver(g, v, 7)) == R.bits(R.exact_sums(g, v, 7))).all()
    assert (R.bits(driver(np.full(9, -1, dtype=np.int32), np.ones(9), 4)) == 0).all()        # no counted sample
    assert (R.bits(driver(np.zeros(0, dtype=np.int32), np.zeros(0), 4)) == 0).all()


# ------------------------------------------------------------------------------ the C ABI ------
NEW = ("cm2_ground_sums_create", "cm2_ground_sums_destroy", "cm2_ground_sums_info", "cm2_ground_sums_apply")
NOT_RESTARTABLE = ("cm2_ground_sums_destroy", "cm2_ground_sums_info")
KERNELS = ("k_gsum_absmax", "k_gsum_bin_lds", "k_gsum_bin_global", "k_gsum_finish")


class _Handle(ctypes.Structure):
    """The members of struct cm2_ground_sums (cm2_ground_exact.hip): the refusals of apply read nbins only, so a
    handle made here meets them on a machine where create cannot allocate."""
    _fields_ = [("nbins", ctypes.c_int), ("d_state", ctypes.c_void_p)]


def test_abi_lists_name_the_new_entry_points():
    from cosmomap2_amd import _hip, build as B, kernel_resources as KR
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
    assert "linearoperators.py:394-400" in text
    assert "cm2_ground_exact.hip" not in B.FMA_OK                         # the limb arithmetic needs plain IEEE steps


def test_new_entry_points_refuse_null_arguments():
    """Their argument checks come before the first HIP call: no GPU is needed to meet them."""
    from cosmomap2_amd import _hip
    lib = _hip.load()
    for name in NEW:
        if name == "cm2_ground_sums_destroy":
            assert lib.cm2_ground_sums_destroy(None) == 0
            continue
        args = [0 if a in (ctypes.c_int, ctypes.c_int64) else None for a in _hip.PROTOTYPES[name]]
        assert getattr(lib, name)(*args) == _hip.ERR_ARGUMENT, name
        assert name.encode() in lib.cm2_last_error(), (name, lib.cm2_last_error())


def test_bad_arguments_are_refused_before_the_device():
    from cosmomap2_amd import _hip
    lib = _hip.load()
    h = ctypes.c_void_p()
    for nbins in (0, -3):
        assert lib.cm2_ground_sums_create(ctypes.byref(h), nbins, None) == _hip.ERR_ARGUMENT
        msg = lib.cm2_last_error()
        assert b"cm2_ground_sums_create" in msg and b"nbins" in msg and not h.value, msg
    # the arrays are never read: every call below is refused first
    arr, out = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    small, large = _Handle(2048, None), _Handle(2049, None)

    def apply(hd, nt, route, d_bin=arr, d_v=arr, d_sums=out):
        rc = lib.cm2_ground_sums_apply(ctypes.cast(ctypes.pointer(hd), ctypes.c_void_p), nt, d_bin, d_v, route,
                                       d_sums, None)
        return rc, lib.cm2_last_error()

    for args, word in (((small, 2 ** 31, 0), b"2^31"), ((small, 2 ** 40, 2), b"2^31"), ((small, -1, 0), b"nt="),
                       ((small, 10, 3), b"route"), ((small, 10, -1), b"route"), ((large, 10, 1), b"2048"),
                       ((small, 10, 0, None), b"NULL"), ((small, 10, 0, arr, None), b"NULL"),
                       ((small, 10, 0, arr, arr, None), b"NULL")):
        rc, msg = apply(*args)
        assert rc == _hip.ERR_ARGUMENT and b"cm2_ground_sums_apply" in msg and word in msg, (args[1:], rc, msg)
    info = (ctypes.c_int64 * 4)()
    for hd, want in ((small, [2048, 2048, 3 * 8 * 2048, 1]), (large, [2049, 2048, 0, 2]), (_Handle(1, None), [1, 2048, 24, 1])):
        assert lib.cm2_ground_sums_info(ctypes.byref(hd), info) == 0
        assert list(info) == want


def test_new_kernels_use_no_scratch():
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


def test_reproducible_must_be_a_bool():
    """refused before the GPU is touched: this machine has none"""
    from cosmomap2_amd.interfaces import GroundFilterLO
    g = np.zeros(20, dtype=np.int32)
    for bad in (1, 0, "yes", None, np.True_):
        with pytest.raises(ValueError, match="reproducible"):
            GroundFilterLO(g, reproducible=bad)
