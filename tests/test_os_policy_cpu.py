"""The host decisions of the overlap-save N^-1 (cosmomap2_amd/csrc/cm2_os_policy.h) on a CPU: a small driver is
compiled against the header with the host g++ -- which is the proof that the header needs no device -- and its
answers are checked against the rules, computed here in Python.  No GPU, no library."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")

T, PTS, HALO = 256, 32, 2048          # threads, complex points per thread, halo
N = T * PTS                           # 8192 complex points = 16384 samples a window
HOP = 2 * N - 2 * HALO                # 12288 outputs a window
SORTED, DIRECT, INVERSE = 0, 1, 2     # os::Builder
PLAIN, RC, INV = 1, 2, 3              # list formats

DRIVER = r"""
#include "cm2_os_policy.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace cm2::os;
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "geometry")) {
        printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", kT, kPts, kHalo, N, W, HOP, RR, RSLOTS, RLEN, NLIST, PER, LDSD);
        for (int l = 0; l <= NLIST; ++l) printf("%d %d\n", list_off(l), l < NLIST ? list_len(l) : 0);
        printf("%zu\n", sizeof(WinDesc));
    } else if (!strcmp(argv[1], "windows")) {                  // windows off0 off1 ...
        std::vector<int64_t> off;
        for (int i = 2; i < argc; ++i) off.push_back(atoll(argv[i]));
        for (int rep = 0; rep < 2; ++rep)                       // (no hidden state: the same answer twice)
            for (const WinDesc &w : windows(off))
                printf("%lld %lld %lld %lld %d %d\n", (long long)w.start, (long long)w.len, (long long)w.lo,
                       (long long)w.hi, (int)w.blk, (int)w.pad);
    } else if (!strcmp(argv[1], "lists")) {                    // lists want sort tile_off ntiles ...
        for (int i = 5; i < argc; ++i) {
            const int64_t nt = atoll(argv[i]);
            const ListChoice c = choose_lists(atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4]) != 0, nt);
            printf("%d %d %d %d %d\n", (int)c.builder, c.mode, c.rmax, rmax(nt), table_fits(c.rmax) ? 1 : 0);
        }
    } else if (!strcmp(argv[1], "descriptor")) {               // descriptor flat nvalid ...
        for (int i = 3; i < argc; ++i) printf("%u\n", descriptor_bytes(atoll(argv[i]), atoi(argv[2]) != 0));
    } else if (!strcmp(argv[1], "lds")) {                      // lds mode rmax
        printf("%zu\n", kernel_lds_bytes(atoi(argv[2]), atoi(argv[3])));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("os_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]


def test_geometry_of_the_one_window_kernel(driver):
    out = _run(driver, "geometry")
    rr, rslots = 2, (PTS - 8) // 2
    rlen = 512 * rslots
    assert out[0] == [T, PTS, HALO, N, 2 * N, HOP, rr, rslots, rlen, 2 + rr, 2 * N + HOP, N + N // 32]
    assert (N, HOP, rlen) == (8192, 12288, 6144) and rr * rlen == HOP
    # two window halves, then the result rounds: the lists of a window follow one another without a gap
    assert [o for o, _ in out[1:6]] == [0, N, 2 * N, 2 * N + rlen, 2 * N + HOP]
    assert [n for _, n in out[1:5]] == [N, N, rlen, rlen]
    assert out[6] == [40]                                      # WinDesc as the kernels read it: 4 x i64 + 2 x i32


LAYOUTS = {
    "empty": [0],
    "no_blocks": [],
    "empty_block": [0, 0, 5, 5],
    "one_short": [0, 1000],
    "exactly_hop": [0, HOP],
    "hop_plus_one": [0, HOP + 1],
    "offset_start": [777, 777 + 3 * HOP - 1],
    "uneven": [0] + list(np.cumsum(np.random.default_rng(5).integers(1, 5 * HOP, 23))),
    "many_equal": list(range(0, 40 * 30000 + 1, 30000)),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_windows_tile_every_block(driver, layout):
    off = [int(x) for x in LAYOUTS[layout]]
    rows = _run(driver, "windows", *off)
    assert rows[:len(rows) // 2] == rows[len(rows) // 2:]      # called twice: the same windows
    wins = rows[:len(rows) // 2]
    nb = max(len(off) - 1, 0)
    assert len(wins) == sum(-(-(off[b + 1] - off[b]) // HOP) for b in range(nb))
    at = 0
    for b in range(nb):
        mine = []
        while at < len(wins) and wins[at][4] == b:
            mine.append(wins[at])
            at += 1
        if off[b + 1] == off[b]:
            assert not mine
            continue
        for start, ln, lo, hi, blk, pad in mine:
            assert (lo, hi, pad) == (off[b], off[b + 1], 0)
            assert 0 < ln <= HOP and lo <= start and start + ln <= hi          # inside its block
        starts = [w[0] for w in mine]
        lens = [w[1] for w in mine]
        assert starts[0] == off[b] and starts[-1] + lens[-1] == off[b + 1]
        assert starts[1:] == [s + n for s, n in zip(starts[:-1], lens[:-1])]   # no gap, no overlap
        assert all(n == HOP for n in lens[:-1])                                # only the last one is shorter
    assert at == len(wins)                                                     # blocks in order, nothing else
    if layout == "exactly_hop":
        assert [w[:2] for w in wins] == [[0, HOP]]
    if layout == "hop_plus_one":
        assert [w[:2] for w in wins] == [[0, HOP], [HOP, 1]]


def _rmax(ntiles):
    bound = min(ntiles if ntiles > 0 else N, N)
    return max((bound + 63) // 64 * 64, 64)


NTILES = [0, 1, 512, 767, 768, 1536, 2048, 2049, 4096, 4097]


@pytest.mark.parametrize("want,sort,tile_off", list(itertools.product([0, PLAIN, RC, INV], [0, 1], [0, 1])))
def test_list_format_and_builder(driver, want, sort, tile_off):
    rows = _run(driver, "lists", want, sort, tile_off, *NTILES)
    for nt, (builder, mode, rmax, rmax_alone, fits) in zip(NTILES, rows):
        assert rmax == rmax_alone == _rmax(nt) and rmax % 64 == 0 and 64 <= rmax <= N
        assert fits == (1 if rmax <= 2048 else 0)
        wanted = want if want else (RC if nt < 768 else INV)               # auto: run-coded below 768 tiles
        direct = (not sort) and tile_off and 0 < nt <= 4096
        if not direct:
            assert builder == SORTED
            assert mode != INV                                             # the sorted path never yields inverse lists
            assert mode == (RC if wanted >= RC and rmax <= 2048 else PLAIN)
        elif wanted == INV and rmax <= 2048:
            assert (builder, mode) == (INVERSE, INV)
        else:
            assert builder == DIRECT
            assert mode == (RC if wanted >= RC and rmax <= 2048 else PLAIN)
        if mode != PLAIN:
            assert rmax <= 2048                                            # run tables only while they fit LDS
    # spelled out: the defaults of the two bench configurations and the boundaries
    if (want, sort, tile_off) == (0, 0, 1):
        got = {nt: (r[0], r[1]) for nt, r in zip(NTILES, rows)}
        assert got[512] == (DIRECT, RC) and got[767] == (DIRECT, RC) and got[768] == (INVERSE, INV)
        assert got[1536] == (INVERSE, INV) and got[2048] == (INVERSE, INV) and got[2049] == (DIRECT, PLAIN)
        assert got[4096] == (DIRECT, PLAIN) and got[4097] == (SORTED, PLAIN) and got[0] == (SORTED, PLAIN)


def test_descriptor_or_flat_addressing(driver):
    edge = 0xFFFFFFF0
    nvalid = [-1, 0, 1, 12345, edge // 8 - 1, edge // 8, edge // 8 + 1, 1 << 29, 1 << 40]
    got = [r[0] for r in _run(driver, "descriptor", 0, *nvalid)]
    want = [n * 8 if n > 0 and n * 8 < edge else 0 for n in nvalid]
    assert got == want
    assert got[4] == edge - 8 and got[5] == 0 and got[6] == 0              # nvalid * 8 just below / at / above
    assert [r[0] for r in _run(driver, "descriptor", 1, *nvalid)] == [0] * len(nvalid)    # CM2_OS_FLAT


def test_kernel_lds_bytes(driver):
    plane = 8 * (N + N // 32)                                  # the padded exchange plane
    for mode, rmax in itertools.product([0, PLAIN, RC, INV], [0, 64, 512, 1536, 2048]):
        tables = 2 * 4 * rmax if mode >= RC else 0             # the two run tables of a list pair
        assert _run(driver, "lds", mode, rmax) == [[plane + tables + 2048]]
    assert _run(driver, "lds", RC, 512)[0][0] == 67584 + 4096 + 2048                  # C4: 512 pixel tiles
