"""
The PCA filter without a GPU: cm2_pca_policy.h compiled with the host compiler (work items, units and slabs against a
brute-force enumeration, the LDS budget and layout, the limits), the prototypes and the header, every argument check
of PCAFilterLO, _pca_ref.py against brute force on tiny inputs, the sign rule, and the detection-quality case on the
reference alone.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _pca_ref as R
import _cmode_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
LD = R.LD
ENTRY_POINTS = {"create": 10, "destroy": 1, "info": 2, "cov_doubles": 1, "cov": 5, "set_modes": 3, "apply": 4,
                "fit": 4, "status": 2}


# ------------------------------------------------------------ names and header ----
def test_names_are_exported_and_the_header_declares_the_entry_points():
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd import _hip, kernel_resources as KR, build as B
    from cosmomap2_amd.interfaces import linearoperators as L
    for name in ("PCAFilterLO", "pca_select_modes"):
        assert callable(getattr(I, name)) and name in L.__all__
    hdr = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint(?:64_t)? cm2_pca_%s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_hip.PROTOTYPES["cm2_pca_" + name]), name
    assert _hip._RESTYPE["cm2_pca_cov_doubles"] is _hip._i64
    for name in ("create", "cov", "set_modes", "fit", "status"):
        assert "cm2_pca_" + name in _hip.RESTARTABLE
    assert "cm2_pca_apply" not in _hip.RESTARTABLE                      # its output may be its input
    assert re.search(r"#define CM2_PCA_TAU 0\.0009765625\b", hdr) and R.TAU == 0.0009765625
    assert re.search(r"#define CM2_PCA_MAX_K 10\b", hdr) and R.MAX_K == L.PCA_MAX_K == 10
    assert re.search(r"#define CM2_PCA_SEGMENT %d\b" % R.SEGMENT, hdr)
    for cls, name in enumerate(("FITTED", "EMPTY", "FEW", "PIVOT")):
        assert re.search(r"#define CM2_PCA_%s %d\b" % (name, cls), hdr) and getattr(R, name) == cls
    assert L.PCAFilterLO.CLASSES == ("fitted", "empty", "few", "pivot")
    assert hdr.index("---- f2f:") < hdr.index("---- f2g:") < hdr.index("---- f3:")
    for k in ("k_pca_cov", "k_pca_cov_final", "k_pca_apply<10>", "k_pca_fit<1>", "k_pca_class<6>"):
        assert any(re.search(p, k) for p in KR.NO_SPILL), k            # the build refuses spills in them
    assert "cm2_pca.hip" not in B.FMA_OK
    hip, unit = (open(os.path.join(CSRC, f)).read() for f in ("cm2_pca.hip", "cm2_modefit.h"))        # with the unit
    src = hip + unit
    atomics = re.findall(r"\batomic\w*\s*\(\s*&?\s*(\w+)", src)                # integer tallies only
    assert sorted(atomics) == ["counts", "tally"] and re.search(r"unsigned long long \*__restrict__ counts", src)
    assert "shfl" not in hip.split('#include "cm2_modefit.h"')[1]                # no cross-lane sums: the file's code
    assert "shfl" not in unit.split('#include "cm2_common.h"')[1]               # and the unit's
    assert not hasattr(L.PCAFilterLO, "_apply_tiles") and issubclass(L.PCAFilterLO, L._TimeFilter)
    assert "NOT linear in ``d``" in L.PCAFilterLO.__doc__ and "use_flags=False" in L.PCAFilterLO.__doc__


def test_arguments_are_refused_before_the_gpu_is_needed():
    from cosmomap2_amd import _hip
    from cosmomap2_amd.interfaces import PCAFilterLO
    from cosmomap2_amd.linop import ShapeError
    pix = np.zeros(100, dtype=np.int32)                                  # 4 detectors x 25 samples
    for kw in (dict(ndet=0), dict(ndet=2.5), dict(nmodes=0), dict(nmodes=11), dict(nmodes=1.5), dict(groups=0),
               dict(groups=[0, 3]), dict(groups=[0, 2, 2, 4]), dict(groups=[1, 4]), dict(chunks=0), dict(chunks=2.5),
               dict(chunks=[0, 24]), dict(chunks=[1, 25]), dict(chunks=[0, 10, 10, 25]), dict(chunks=[0, 12, 7, 25]),
               dict(modes=np.ones((1, 4, 4))), dict(modes=np.ones((1, 4, 2)), groups=2),  # a group below K + 1
               dict(modes=np.ones((1, 4, 1)), groups=[0, 1, 4]),
               dict(modes=np.ones((1, 4, 11))), dict(modes=np.ones((1, 4, 0))),
               dict(nmodes=3, modes=np.ones((1, 4, 2)))):
        args = dict(ndet=4)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            PCAFilterLO(pix, **args)
        assert str(e.value), kw
    for p, kw in ((pix, dict(ndet=3)), (pix[:0], dict(ndet=4)), (pix, dict(ndet=4, modes=np.ones((4, 2)))),
                  (pix, dict(ndet=4, modes=np.ones((2, 4, 2)))), (pix, dict(ndet=4, modes=np.ones((1, 5, 2)))),
                  (pix, dict(ndet=4, chunks=5, modes=np.ones((1, 4, 2)))), (pix, dict(ndet=4, groups=[[0, 4]])),
                  (pix, dict(ndet=4, chunks=[[0, 25]])), (pix, dict(ndet=4, chunks=[0.0, 25.0]))):
        with pytest.raises(ShapeError):
            PCAFilterLO(p, **kw)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipError):
            PCAFilterLO(pix, ndet=4, nmodes=2, chunks=10)


# ------------------------------------------------------- the policy header, on a CPU ----
DRIVER = r"""
#include "cm2_pca_policy.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace cm2::pca;
int main(int argc, char **argv)
{
    // driver tables|status ns ndet K g0 g1 ... @ c0 c1 ...
    if (argc < 6) return 2;
    printf("%d %d %d %d %d %d %d %d %d %d\n", kThreads, kMaxK, kMfma, kMfmaK, kTile, kWaveTile, kStep, kPitch, kSegment,
           (int)lds_bytes());
    printf("%d %d %d %d\n", (int)kFitted, (int)kEmpty, (int)kFew, (int)kPivot);
    // the banks of the operand reads of one half-wave (16 rows x 2 samples), for every MFMA block and sample quad
    int worst = 0;
    for (int blk = 0; blk < kTile / kMfma; ++blk)
        for (int q = 0; q < kStep / kMfmaK; ++q)
            for (int half = 0; half < 2; ++half) {
                int hits[64] = {0};
                for (int m = 0; m < 16; ++m)
                    for (int k = 0; k < 2; ++k) {
                        const int b = lds_bank(blk * kMfma + m, kMfmaK * q + 2 * half + k);
                        ++hits[b];
                        ++hits[(b + 1) % 64];
                    }
                for (int b = 0; b < 64; ++b) worst = hits[b] > worst ? hits[b] : worst;
            }
    printf("%d %d\n", worst, lds_at(kTile - 1, kStep - 1) + 1 + kTile * kPitch <= (int)(lds_bytes() / 8) ? 1 : 0);
    std::vector<int64_t> g, c;
    int i = 5;
    for (; i < argc && argv[i][0] != '@'; ++i) g.push_back(atoll(argv[i]));
    for (++i; i < argc; ++i) c.push_back(atoll(argv[i]));
    Plan p;
    const Status st = check(&p, atoll(argv[2]), atoll(argv[3]), (int64_t)g.size() - 1, g.data(), (int64_t)c.size() - 1,
                            c.data(), atoi(argv[4]));
    printf("%d\n", (int)st);
    if (st != kOk) return 0;
    printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)p.nt, (long long)p.units,
           (long long)p.cov_units, (long long)p.cov_per_chunk, (long long)p.cov_doubles, (long long)p.items,
           (long long)p.work_doubles, (long long)p.slabs, (long long)p.blocks, (long long)p.final_blocks,
           (long long)p.min_group);
    printf("%d %d %d\n", (int)modes_allowed(p.min_group, atoi(argv[4])), (int)modes_allowed(3, 2), (int)modes_allowed(2, 2));
    if (argv[1][0] != 't') return 0;
    std::vector<CovItem> items;
    std::vector<CovUnit> units;
    std::vector<Slab> slabs;
    cov_table((int64_t)g.size() - 1, g.data(), (int64_t)c.size() - 1, c.data(), &items, &units);
    slab_table((int64_t)c.size() - 1, c.data(), &slabs);
    printf("%zu %zu %zu\n", items.size(), units.size(), slabs.size());
    for (const CovItem &t : items)
        printf("%d %lld %lld %lld %d %d %d %lld\n", t.unit, (long long)t.row0, (long long)t.col0, (long long)t.first,
               t.len, t.rows, t.cols, (long long)t.part);
    for (const CovUnit &u : units)
        printf("%lld %lld %d %d\n", (long long)u.first_item, (long long)u.at, u.n, u.nseg);
    for (const Slab &s : slabs) printf("%lld %d %d\n", (long long)s.first, s.len, s.chunk);
    printf("%d %d %d %d\n", (int)apply_ok(4096, 4096, 10), (int)apply_ok(4096, 4096 + 80, 10),
           (int)apply_ok(4096, 4096 + 72, 10), (int)apply_ok(4096 + 72, 4096, 10));
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("pca_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _run(driver, mode, ns, ndet, K, gedges, cedges):
    args = [mode, ns, ndet, K] + list(gedges) + ["@"] + list(cedges)
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]


def test_policy_constants_lds_budget_and_banks(driver):
    out = _run(driver, "status", 10, 2, 1, [0, 2], [0, 10])
    assert out[0] == [R.THREADS, R.MAX_K, R.MFMA, R.MFMA_K, R.TILE, R.WAVE_TILE, R.STEP, R.PITCH, R.SEGMENT, R.LDS_BYTES]
    assert out[1] == [R.FITTED, R.EMPTY, R.FEW, R.PIVOT]
    assert R.LDS_BYTES == 36864 <= 64 * 1024                            # two slabs of 128 rows x 18 doubles
    assert R.TILE == 2 * R.WAVE_TILE and R.WAVE_TILE == 4 * R.MFMA and R.SEGMENT % R.STEP == 0 and R.STEP % R.MFMA_K == 0
    # every half-wave operand read touches each of the 64 banks exactly once; both slabs lie inside the LDS
    assert out[2] == [1, 1]


@pytest.mark.parametrize("gedges,cedges", [
    ([0, 2], [0, 1]),
    ([0, 15, 31, 48], [0, 1, 4, 8, 13, 45]),
    ([0, 127, 255, 384], [0, 255, 256, 513, 773]),
    ([0, 1, 18, 82, 112], [0, 3, R.SEGMENT + 2, 2 * R.SEGMENT + 2, 2 * R.SEGMENT + 7, 3 * R.SEGMENT + 8,
                           5 * R.SEGMENT + 15]),
    ([0, 300, 302], [0, R.SEGMENT - 1, 3 * R.SEGMENT + 6]),
])
def test_tables_against_brute_force(driver, gedges, cedges):
    ns, ndet, G, Cn = cedges[-1], gedges[-1], len(gedges) - 1, len(cedges) - 1
    K = 1
    out = _run(driver, "tables", ns, ndet, K, gedges, cedges)
    assert out[3] == [0] == [R.policy_status(ns, ndet, gedges, cedges, K)]
    want = R.work_items(gedges, cedges)
    sl = R.slabs(cedges)
    per = int((np.diff(gedges) ** 2).sum())
    nt, units, cov_units, per_chunk, cov_doubles, nitems, work, nslabs, blocks, final_blocks, min_group = out[4]
    assert min_group == min(np.diff(gedges))
    assert (nt, units, cov_units, per_chunk, cov_doubles) == (ndet * ns, G * ns, Cn * G, per, Cn * per)
    assert nitems == len(want) and nslabs == len(sl) and blocks == G * len(sl)
    assert final_blocks == -(-Cn * per // R.THREADS)
    assert out[5] == [int(min_group >= 2), 1, 0]                         # modes need K + 1 detectors in every group
    assert out[6] == [nitems, cov_units, nslabs]
    items, rest = out[7:7 + nitems], out[7 + nitems:]
    utab, stab, ok = rest[:cov_units], rest[cov_units:cov_units + nslabs], rest[cov_units + nslabs]
    # every item the brute force finds, once, with its sizes; partials packed without gaps or overlaps, in order
    seen, part = set(), 0
    for unit, row0, col0, first, ln, rows, cols, at in items:
        key = (unit, row0, col0, first)
        assert key in want and key not in seen and want[key] == [ln, rows, cols], key
        assert 1 <= ln <= R.SEGMENT and 1 <= rows <= R.TILE and 1 <= cols <= R.TILE and col0 <= row0
        assert at == part
        seen.add(key)
        part += rows * cols
    assert part == work and len(seen) == len(want)
    # ordered by unit, then tile pair, then segment: the segments of a pair are neighbours, ascending
    keys = [(u, r, c, f) for u, r, c, f, *_ in items]
    assert keys == sorted(keys)
    offs = R.cov_offsets(np.array(gedges), Cn)
    for u, (first_item, at, n, nseg) in enumerate(utab):
        c, g = divmod(u, G)
        T = -(-n // R.TILE)
        assert n == gedges[g + 1] - gedges[g] and at == offs[c][g] and nseg == -(-(cedges[c + 1] - cedges[c]) // R.SEGMENT)
        mine = [k for k, it in enumerate(items) if it[0] == u]
        assert mine == list(range(first_item, first_item + T * (T + 1) // 2 * nseg))
        for a in range(T):
            for b in range(a + 1):
                for s in range(nseg):                                    # where k_pca_cov_final looks an item up
                    it = items[first_item + (a * (a + 1) // 2 + b) * nseg + s]
                    assert it[1:4] == [gedges[g] + a * R.TILE, gedges[g] + b * R.TILE, cedges[c] + s * R.SEGMENT]
    assert [tuple(s) for s in stab] == sl
    covered = np.zeros(ns, dtype=int)
    for first, ln, c in sl:
        assert 1 <= ln <= R.THREADS and cedges[c] <= first and first + ln <= cedges[c + 1]
        covered[first:first + ln] += 1
    assert (covered == 1).all()
    assert ok == [1, 1, 0, 0]                                            # itself, disjoint, overlapping either way


def test_policy_refusals_and_limits(driver):
    def status(ns, ndet, K, gedges, cedges):
        got = _run(driver, "status", ns, ndet, K, gedges, cedges)[3][0]
        assert got == R.policy_status(ns, ndet, gedges, cedges, K), (ns, ndet, K, gedges, cedges)
        return got
    ok = ([0, 4], [0, 10])
    assert status(10, 4, 0, *ok) == 1 and status(10, 4, 11, *ok) == 1 and status(10, 4, -1, *ok) == 1
    assert status(0, 4, 3, [0, 4], [0, 0]) == 2 and status(10, 0, 3, [0, 0], [0, 10]) == 2
    assert status(10, 4, 3, [0, 3], [0, 10]) == 3 and status(10, 4, 3, [1, 4], [0, 10]) == 3
    assert status(10, 8, 1, [0, 4, 4, 8], [0, 10]) == 3 and status(10, 8, 1, [0, 6, 3, 8], [0, 10]) == 3
    assert status(10, 4, 3, [0, 4], [0, 9]) == 4 and status(10, 4, 3, [0, 4], [1, 10]) == 4
    assert status(10, 4, 3, [0, 4], [0, 5, 5, 10]) == 4 and status(10, 4, 3, [0, 4], [0, 7, 3, 10]) == 4
    assert status(10, 4, 4, *ok) == 0 and status(10, 1, 1, [0, 1], [0, 10]) == 0    # the covariance takes any group
    assert status(1 << 30, (1 << 16) + 2, 1, [0, (1 << 16) + 2], [0, 1 << 30]) == 5        # ndet ns > 2^46
    assert status(1 << 30, 1 << 16, 1, [0, 1 << 16], [0, 1 << 30]) == 5                     # 2^17 tile pairs x 2^18 segments
    assert status(1 << 20, 1 << 16, 1, list(range(0, (1 << 16) + 1, 128)), [0, 1 << 20]) == 0
    assert status(4, (1 << 23) + 2, 1, [0, (1 << 23) + 2], [0, 4]) == 5                 # ndet > 2^23
    assert status(4, 1 << 16, 1, [0, 1 << 16], [0, 4]) == 0 and status(4, 1 << 20, 1, [0, 1 << 20], [0, 4]) == 5  # 2^32 final workgroups
    assert status(1 << 45, 2, 1, [0, 2], [0, 1 << 45]) == 5                                 # 2^37 slabs, 2^33 segments
    assert status(((1 << 31) - 1) * 256, 1, 1, [0, 1], [0, ((1 << 31) - 1) * 256]) == 0
    assert status(((1 << 31) - 1) * 256 + 1, 1, 1, [0, 1], [0, ((1 << 31) - 1) * 256 + 1]) == 5
    many = list(range(0, (1 << 16) + 2))
    assert status((1 << 16) + 1, 2, 1, [0, 2], many) == 5 and status(1 << 16, 2, 1, [0, 2], many[:-1]) == 0


# ------------------------------------------------- _pca_ref against brute force ----
def test_cov_ref_against_brute_force():
    rng = np.random.default_rng(1)
    ndet, ns, gedges, cedges = 5, 9, [0, 2, 5], [0, 4, 9]
    d = rng.standard_normal(ndet * ns)
    pix = np.where(rng.random(ndet * ns) < 0.3, -1, 5).astype(np.int32)
    d[np.flatnonzero(pix < 0)[0]] = np.nan                               # a flagged sample is never read
    for flags in (None, pix):
        cov, S = R.cov_ref(d if flags is not None else np.nan_to_num(d), flags, ndet, gedges, cedges)
        x = np.nan_to_num(d).reshape(ndet, ns)
        for c in range(2):
            for g in range(2):
                n = gedges[g + 1] - gedges[g]
                assert cov[c][g].shape == (n, n) == S[c][g].shape and cov[c][g].dtype == LD
                for a in range(n):
                    for b in range(n):
                        tot, mag = LD(0), LD(0)
                        for i in range(cedges[c], cedges[c + 1]):
                            ka, kb = gedges[g] + a, gedges[g] + b
                            xa = LD(0) if flags is not None and flags[ka * ns + i] < 0 else LD(x[ka, i])
                            xb = LD(0) if flags is not None and flags[kb * ns + i] < 0 else LD(x[kb, i])
                            tot, mag = tot + xa * xb, mag + abs(xa) * abs(xb)
                        assert abs(cov[c][g][a, b] - tot) <= LD(2.0) ** -60 * mag and abs(S[c][g][a, b] - mag) <= \
                            LD(2.0) ** -60 * mag
    assert R.cov_offsets(np.array(gedges), 2) == [[0, 4], [13, 17]]
    # the acceptance: exact where S = 0, the bound elsewhere, NaN never accepted
    S1 = np.array([[1.0, 0.0], [0.0, 0.0]])
    assert R.cov_excess(np.zeros((2, 2)), np.zeros((2, 2)), S1, 4) == 0.0
    assert R.cov_excess(np.array([[0.0, 1e-300], [0, 0]]), np.zeros((2, 2)), S1, 4) == np.inf
    assert R.cov_excess(np.array([[np.nan, 0.0], [0, 0]]), np.zeros((2, 2)), S1, 4) == np.inf
    b = float(R.cov_bound(4, 1.0))
    assert b == 6 * 2.0 ** -53 * 1.01
    assert R.cov_excess(np.array([[0.9 * b, 0.0], [0, 0]]), np.zeros((2, 2)), S1, 4) <= 1.0 < \
        R.cov_excess(np.array([[1.1 * b, 0.0], [0, 0]]), np.zeros((2, 2)), S1, 4)


def test_per_chunk_restatement_against_a_scalar_walk():
    """pca_f64 is cmode_f64 per chunk with that chunk's modes: checked unit by unit against the order written in
    cm2_cmode.hip, with the scalar factor and solves of _hwpss_ref"""
    import _hwpss_ref as H
    rng = np.random.default_rng(2)
    ndet, ns, K, gedges, cedges = 7, 11, 2, np.array([0, 3, 7]), np.array([0, 1, 6, 11])
    modes = rng.standard_normal((3, ndet, K))
    v = rng.standard_normal(ndet * ns)
    pix = np.where(rng.random(ndet * ns) < 0.3, -1, 5).astype(np.int32)
    f = R.pca_f64(pix, ndet, gedges, cedges, modes, v)
    r = R.pca_ref(pix, ndet, gedges, cedges, modes, v)
    assert f.out.shape == (ndet * ns,) == r.S.shape and f.coeff.shape == (2, K, ns) and f.status.shape == (2, ns)
    assert np.array_equal(f.status, r.status) and len(set(f.status.reshape(-1).tolist())) >= 2
    ok, v2 = (pix >= 0).reshape(ndet, ns), v.reshape(ndet, ns)
    for i in range(ns):
        c = int(np.searchsorted(cedges, i, side="right") - 1)
        Phi = modes[c]
        for g in range(2):
            ks = [k for k in range(gedges[g], gedges[g + 1]) if ok[k, i]]
            G, b = np.zeros((K, K)), np.zeros(K)
            for k in ks:
                for a in range(K):
                    for cc in range(a + 1):
                        G[a, cc] += Phi[k, a] * Phi[k, cc]
                    b[a] += Phi[k, a] * v2[k, i]
            L = H.cholesky(G, np.float64)[0] if len(ks) >= K else None
            want, cf = np.zeros(ndet), np.zeros(K)
            if L is not None:
                cf = H.solve(L, b)
                for k in ks:
                    pr = cf[0] * Phi[k, 0]
                    for j in range(1, K):
                        pr += cf[j] * Phi[k, j]
                    want[k] = v2[k, i] - pr
            assert (f.status[g, i] == R.FITTED) == (L is not None)
            sl = slice(gedges[g], gedges[g + 1])
            assert np.array_equal(R.bits(f.out.reshape(ndet, ns)[sl, i]), R.bits(want[sl])), (g, i)
            assert np.array_equal(R.bits(f.coeff[g, :, i]), R.bits(cf)), (g, i)
    assert R.V.excess(f.out, r.out, r.S, C.c_bound(4, K)) <= 1.0


def test_selection_and_the_sign_rule():
    from cosmomap2_amd.interfaces import pca_select_modes
    rng = np.random.default_rng(3)
    A = rng.standard_normal((6, 40))
    cov = A @ A.T
    for K in (1, 3, 6):
        m, w = R.select_modes(cov, K)
        m2, w2 = pca_select_modes(cov, K)
        assert np.array_equal(R.bits(m), R.bits(m2)) and np.array_equal(R.bits(w), R.bits(w2))
        assert m.shape == (6, K) and w.shape == (6,) and (np.diff(w) <= 0).all()
        for j in range(K):
            assert np.abs(cov @ m[:, j] - w[j] * m[:, j]).max() <= 1e-12 * w[0]
            assert m[np.argmax(np.abs(m[:, j])), j] > 0
        assert np.abs(m.T @ m - np.eye(K)).max() <= 1e-13
    # a tie: the eigenvectors of [[2, 1], [1, 2]] are (1, 1) / sqrt 2 and (1, -1) / sqrt 2, both components of the
    # same magnitude; the first component decides
    m, w = R.select_modes(np.array([[2.0, 1.0], [1.0, 2.0]]), 2)
    m2, _ = pca_select_modes(np.array([[2.0, 1.0], [1.0, 2.0]]), 2)
    assert w.tolist() == [3.0, 1.0] and np.array_equal(R.bits(m), R.bits(m2))
    if abs(m[0, 1]) == abs(m[1, 1]):
        assert m[0, 1] > 0 > m[1, 1]
    else:                                                                # (rounding split the tie)
        assert m[np.argmax(np.abs(m[:, 1])), 1] > 0
    assert m[0, 0] > 0 and m[1, 0] > 0
    # exactly: a diagonal matrix with a negated eigenvector basis cannot occur, so force the rule on hand-made columns
    for col, want in (([-0.5, 0.5], [0.5, -0.5]), ([0.5, -0.5], [0.5, -0.5]), ([0.1, -0.9], [-0.1, 0.9])):
        top = int(np.argmax(np.abs(col)))
        got = [-x for x in col] if col[top] < 0 else col
        assert got == want and top == (0 if abs(col[0]) >= abs(col[1]) else 1)
    assert np.array_equal(R.learn([[cov]], 6, [0, 6], 2)[0], R.select_modes(cov, 2)[0])


def test_linear_fill_restated():
    d = np.arange(20.0)
    ok = np.ones(20, dtype=bool)
    ok[[0, 1, 7, 8, 9, 19]] = False
    out = R.linear_fill(d, ok, 1, nedge=2)
    assert np.array_equal(out[ok], d[ok])
    assert out[0] == out[1] == 2.5 and out[19] == 17.5                   # a side without samples takes the other's
    L, Rr = 5.5, 10.5
    assert np.allclose(out[7:10], [L + (Rr - L) * k / 4 for k in (1, 2, 3)], rtol=0, atol=1e-15)
    two = R.linear_fill(np.concatenate([d, d]), np.concatenate([ok, ok]), 2, nedge=2)     # detectors are blocks
    assert np.array_equal(two[:20], out) and np.array_equal(two[20:], out)


# ----------------------------------------------------------- detection quality ----
def test_quality_case_on_the_reference():
    """24 detectors in 2 groups, 4 x 1024 samples, a rank-2 atmosphere with a 1/f amplitude spectrum at 1000 x the
    noise, 5 % flags, K = 2, modes learnt from the linear gap fill with every sample used: the filtered unflagged
    samples are within 2 x the noise, the unfiltered ones beyond 100 x"""
    q, r = R.quality(), R.quality_on_the_host()
    assert (q.ndet, q.ns, q.K, q.gedges.tolist(), q.cedges.tolist()) == (24, 4096, 2, [0, 12, 24],
                                                                         [0, 1024, 2048, 3072, 4096])
    assert abs(1.0 - q.ok.mean() - 0.05) < 0.01
    print("rms over noise: unfiltered %.4g, modes from the zero-filled stream %.4g, from the gap-filled stream %.4g"
          % (r.unfiltered, r.zero_filled, r.gap_filled))
    assert r.gap_filled <= 2.0 and r.unfiltered >= 100.0
    assert r.zero_filled > r.gap_filled                                  # why the recipe fills the gaps first
