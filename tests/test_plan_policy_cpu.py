"""The host decisions of the tile plan (cosmomap2_amd/csrc/cm2_plan_policy.h) on a CPU: a small driver is
compiled against the header with the host g++ -- which is the proof that the header needs no device -- and
its answers for hit histograms generated here are checked as properties, with the expected values computed
in NumPy / Python.  No GPU, no library."""
import heapq
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")

TP = 64                       # tile width
S, ITEM, CHUNK = 256, 4096, 16384     # slice length, work-item length, hot-range length
SLOTS = 512
HOT_MIN_FLOOR = 32768         # policy::kHotTileMin

DRIVER = r"""
#include "cm2_plan_policy.h"
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <string>
using namespace cm2::policy;
typedef std::vector<int64_t> V;
template <typename T> static void put(const char *k, const std::vector<T> &v)
{
    printf("%s", k);
    for (auto x : v) printf(" %lld", (long long)x);
    printf("\n");
}
static V offsets(const V &p0, const std::vector<unsigned int> &hits)      // first address of every tile
{
    V off(p0.size(), 0);
    for (size_t b = 0; b + 1 < p0.size(); ++b) {
        off[b + 1] = off[b];
        for (int64_t p = p0[b]; p < p0[b + 1]; ++p) off[b + 1] += hits[(size_t)p];
    }
    return off;
}
static void plan(const char *name, const V &p0, const std::vector<unsigned int> &hits, int forced)
{
    const std::string n(name);
    const V off = offsets(p0, hits);
    put((n + ".p0").c_str(), p0);
    put((n + ".off").c_str(), off);
    const Slices sl = slices(off, @S@);
    put((n + ".slice0").c_str(), sl.slice0);
    put((n + ".pairs").c_str(), sl.pairs);
    const WorkItems w = work_items(off, @ITEM@);
    put((n + ".item0").c_str(), w.tile_item0);
    put((n + ".item_tile").c_str(), w.tile);
    put((n + ".item_k0").c_str(), w.k0);
    put((n + ".item_k1").c_str(), w.k1);
    const HotRanges h = hot_ranges(p0, off, @CHUNK@);
    put((n + ".hot_flag").c_str(), h.flag);
    put((n + ".hot_range").c_str(), h.range);
    put((n + ".hot_tiles").c_str(), h.tiles);
    put((n + ".hot_range_tile").c_str(), h.range_tile);
    put((n + ".hot_tile").c_str(), h.hot_tile);
    put((n + ".hot_chunk0").c_str(), h.hot_chunk0);
    V load(p0.size() - 1, 0), ns(p0.size() - 1, 0);
    for (size_t b = 0; b + 1 < p0.size(); ++b) {
        ns[b] = sl.slice0[b + 1] - sl.slice0[b];
        if (!is_hot_tile(p0[b + 1] - p0[b], off[b + 1] - off[b])) load[b] = off[b + 1] - off[b];
    }
    put((n + ".load").c_str(), load);
    const PartsChoice c = choose_parts(load, ns, @S@, @SLOTS@, forced);
    printf("%s.parts_target %lld\n%s.parts_makespan %.17g\n", name, (long long)c.target, name, c.makespan);
    put((n + ".parts").c_str(), c.parts);
    V first;                                                           // first slice of every part, + end
    for (size_t b = 0; b + 1 < p0.size(); ++b)
        for (int64_t j = 0; j <= c.parts[b]; ++j) first.push_back(part_slice(ns[b], j, c.parts[b]));
    put((n + ".part_slices").c_str(), first);
}
static void report(int64_t npix, const std::vector<unsigned int> &hits, int64_t hot_min, int forced)
{
    put("shared_cuts", shared_cuts(npix, @TP@));
    const V uni = uniform_tiles(npix, @TP@);
    plan("uniform", uni, hits, forced);
    const V off = offsets(uni, hits);
    int mult = 0;
    const V equal = equal_load_tiles(hits, npix, @TP@, (int64_t)uni.size() - 1, off.back(), &mult);
    printf("equal.mult %d\n", mult);
    plan("equal", equal, hits, forced);
    bool any = false;
    const V hot = hot_pixel_tiles(hits, npix, @TP@, hot_min, &any);
    printf("hot.any %d\n", any ? 1 : 0);
    plan("hot", hot, hits, forced);
    const Balance sw[4] = {Balance::automatic, Balance::off, Balance::cut, Balance::parts};
    for (int i = 0; i < 4; ++i)
        for (int exact = 0; exact < 2; ++exact) {
            const TilingChoice c = choose_tiling(off, exact != 0, sw[i]);
            printf("choice.%d.%d %d %d %lld\n", i, exact, (int)c.tiling, c.pt_split ? 1 : 0, (long long)c.hot_min);
        }
    printf("wanted %d %d %d %d\n", wanted_slice(1536, 400.0, 0.0, 2048, 512), wanted_slice(1536, 700.0, 0.3, 2048, 512),
           wanted_slice(1536, 100.0, 0.0, 1536, 512), wanted_slice(1536, 9000.0, 0.0, 2048, 512));
}
// ---- the fixed-order lists: LDS budget, list offsets, slice tuning, sub-ranges of an ascending tile list ----
static int fx_main(int argc, char **argv)
{
    const std::string what(argv[1]);
    if (what == "lds") {                                        // lds <tp> <pol> <S>...
        const int tp = atoi(argv[2]), pol = atoi(argv[3]);
        printf("bytes");
        for (int i = 4; i < argc; ++i) printf(" %lld", (long long)fx_lds_bytes(tp, pol, atoi(argv[i])));
        printf("\nmax_slice %d\nfills %d\n", fx_max_slice(tp, pol), fx_tile_fills_lds(tp, pol) ? 1 : 0);
        printf("budgets %lld %lld\n", (long long)kLdsTwoPerCU, (long long)kLdsOnePerCU);
        printf("per_cu");
        for (int i = 4; i < argc; ++i) printf(" %d", fx_workgroups_per_cu(tp, pol, atoi(argv[i])));
        printf("\n");
        return 0;
    }
    if (what == "offsets") {                                    // offsets <S> <threads> <shift>: ntiles, off, hot, counts
        const int64_t S = atoll(argv[2]);
        long long n = 0, x;
        if (scanf("%lld", &n) != 1) return 2;
        V off((size_t)n + 1, 0);
        std::vector<uint8_t> hot((size_t)n, 0);
        for (auto &o : off) { if (scanf("%lld", &x) != 1) return 2; o = x; }
        for (auto &h : hot) { if (scanf("%lld", &x) != 1) return 2; h = (uint8_t)x; }
        std::vector<uint32_t> counts;
        while (scanf("%lld", &x) == 1) counts.push_back((uint32_t)x);
        const Slices sl = slices(off, S);
        if ((int64_t)counts.size() != 4 * sl.slice0.back()) return 3;
        for (int rep = 0; rep < 2; ++rep) {
            const FxOffsets r = fx_offsets(counts, sl, hot, S, atoi(argv[3]), atoi(argv[4]));
            put("meta", r.meta);
            put("tent_off", r.tent_off);
            printf("totals %lld %lld %lld\nfits %d\nfill %.17g %.17g\n", (long long)r.ngroups, (long long)r.ntrun,
                   (long long)r.ntent, r.fits ? 1 : 0, r.mean_groups, r.over);
        }
        return 0;
    }
    if (what == "tune") {                                       // tune <forced> <smax> <sample_first>: (mean, over) answers
        std::vector<double> ans;
        double d;
        while (scanf("%lf", &d) == 1) ans.push_back(d);
        size_t at = 0;
        auto step = [&](const char *name) {
            return [&, name](int S, double &mean, double &over) {
                printf("%s %d\n", name, S);
                if (at + 2 > ans.size()) return 9;
                mean = ans[at++];
                over = ans[at++];
                return mean < 0.0 ? 7 : 0;                      // (a negative mean stands for a failed step)
            };
        };
        int S = 0;
        const int rc = tune_slice(atoi(argv[2]), atoi(argv[3]), 512, atoi(argv[4]) != 0, step("count"), step("build"), &S);
        printf("rc %d\nS %d\n", rc, S);
        return 0;
    }
    if (what == "range") {                                      // range: list on stdin, then -1, then (lo, hi) pairs
        V asc, q;
        long long x;
        while (scanf("%lld", &x) == 1 && x >= 0) asc.push_back(x);
        while (scanf("%lld", &x) == 1) q.push_back(x);
        for (size_t i = 0; i + 1 < q.size(); i += 2) {
            const IndexRange r = tiles_in_range(asc, q[i], q[i + 1]);
            printf("%lld %lld\n", (long long)r.lo, (long long)r.hi);
        }
        return 0;
    }
    return -1;
}
int main(int argc, char **argv)
{
    if (argc >= 2 && !isdigit((unsigned char)argv[1][0]) && std::string(argv[1]) != "makespan") return fx_main(argc, argv);
    if (argc == 3 && std::string(argv[1]) == "makespan") {      // makespan <slots>: items on stdin
        V items;
        long long x;
        while (scanf("%lld", &x) == 1) items.push_back(x);
        printf("%.17g\n%.17g\n", parts_makespan(items, atoi(argv[2])), parts_makespan(items, atoi(argv[2])));
        return 0;
    }
    const int64_t npix = atoll(argv[1]), hot_min = atoll(argv[2]);
    const int forced = atoi(argv[3]);
    std::vector<unsigned int> hits;
    long long x;
    while (scanf("%lld", &x) == 1) hits.push_back((unsigned int)x);
    if ((int64_t)hits.size() != npix) return 2;
    report(npix, hits, hot_min, forced);
    printf("again\n");
    report(npix, hits, hot_min, forced);                        // (no hidden state: the same answers)
    return 0;
}
"""
for _k, _v in dict(S=S, ITEM=ITEM, CHUNK=CHUNK, SLOTS=SLOTS, TP=TP).items():
    DRIVER = DRIVER.replace("@%s@" % _k, str(_v))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _hits(kind, npix, nt=1 << 21):
    rng = np.random.default_rng(17)
    if kind == "empty":
        return np.zeros(npix, np.int64)
    pix = rng.integers(0, npix, nt)
    if kind == "uneven":                                      # half of the samples on a tenth of the map
        h = rng.random(nt) < 0.5
        pix[h] = pix[h] % (npix // 10)
    if kind == "hot":                                         # one pixel with 5 % of the samples
        pix[rng.random(nt) < 0.05] = npix // 3
    return np.bincount(pix, minlength=npix).astype(np.int64)


CASES = {"uniform": ("uniform", 32768), "uneven": ("uneven", 32768), "hot": ("hot", 32768),
         "ragged": ("uneven", 32768 + 37), "empty": ("empty", 32768)}


def _run(driver, hits, hot_min, forced=-1):
    p = subprocess.run([driver, str(len(hits)), str(hot_min), str(forced)], input=" ".join(map(str, hits)),
                       stdout=subprocess.PIPE, text=True, check=True)
    first, again = p.stdout.split("again\n")
    assert first == again                                     # calling anything twice: the same result
    out = {}
    for ln in first.splitlines():
        k, *v = ln.split()
        out[k] = [float(x) for x in v] if k.endswith("makespan") else np.array([int(x) for x in v], np.int64)
    return out


def _makespan(items, slots):
    """policy::parts_makespan, operation for operation (IEEE doubles in the same order)"""
    cost, rmax = 4096.0, 1.5
    heap, V, T, nxt = [], 0.0, 0.0, 0
    while nxt < len(items) and len(heap) < slots:
        heapq.heappush(heap, float(items[nxt]) + cost)
        nxt += 1
    total = 0.0
    for x in items:
        total += float(x) + cost
    while heap:
        vf = heap[0]
        T += (vf - V) / min(float(slots) / float(len(heap)), rmax)
        V = vf
        heapq.heappop(heap)
        if nxt < len(items):
            heapq.heappush(heap, V + float(items[nxt]) + cost)
            nxt += 1
    return T * float(slots) / total if total > 0.0 else 1.0


def _parts_items(load, ns, target):
    items = []
    for ld, n in zip(load.tolist(), ns.tolist()):
        if ld == 0:
            continue
        k = 1 if (ld * 10 <= target * 11 or n <= 1) else min(-(-ld // target), n)
        items += [ld // k] * k
    return items


def _check_pieces(off, first, k0, k1, limit):
    """pieces [k0, k1) listed tile after tile tile every non-empty bucket without gap or overlap"""
    assert first[0] == 0 and first[-1] == len(k0) and np.all(np.diff(first) >= 0)
    assert np.all(k1 > k0) and np.all(k1 - k0 <= limit)
    for b in range(len(off) - 1):
        a, e = first[b], first[b + 1]
        if off[b + 1] == off[b]:
            assert a == e
            continue
        assert k0[a] == off[b] and k1[e - 1] == off[b + 1]
        assert np.array_equal(k0[a + 1:e], k1[a:e - 1])
        assert np.all(k1[a:e - 1] - k0[a:e - 1] == limit)    # only the last piece is shorter


@pytest.mark.parametrize("case", sorted(CASES))
def test_tilings_cover_the_map_and_share_the_cuts(driver, case):
    kind, npix = CASES[case]
    hits = _hits(kind, npix)
    nvalid, base = int(hits.sum()), -(-npix // TP)
    hot_min = max(int(0.5 * nvalid / base), HOT_MIN_FLOOR)
    r = _run(driver, hits, hot_min)
    # the nine cuts every rank shares: the uniform boundaries nearest to eighths of the map (cm2_tiles_group_tiles)
    want_cuts = np.minimum((base * np.arange(9) // 8) * TP, npix)
    want_cuts[8] = npix
    assert np.array_equal(r["shared_cuts"], want_cuts)
    assert np.array_equal(r["uniform.p0"], np.minimum(np.arange(base + 1) * TP, npix))
    for name in ("uniform", "equal", "hot"):
        p0 = r[name + ".p0"]
        assert p0[0] == 0 and p0[-1] == npix and np.all(np.diff(p0) > 0) and np.all(np.diff(p0) <= TP), name
        assert np.all(np.isin(want_cuts, p0)), name
        assert np.array_equal(r[name + ".off"], np.concatenate([[0], np.cumsum(hits)])[p0])
    # equal-load cut: at most mult x the uniform count for the mult it stopped at (the multiples are only
    # tried when the uniform count is a multiple of 512; 4 is the last one), a heavy pixel alone in its tile
    mult, p0 = int(r["equal.mult"][0]), r["equal.p0"]
    assert 1 <= mult <= 4
    if base % 512 == 0:
        assert len(p0) - 1 <= mult * base or mult == 4
    else:
        assert mult == 1
    target = int(1.02 * float(nvalid) / float(base * mult)) + 1
    for p in np.flatnonzero(hits > target):
        assert p in p0 and p + 1 in p0
    loads = np.diff(r["equal.off"])
    assert np.all(loads[np.diff(p0) > 1] <= target)           # (no tile of several pixels over the target)
    # hot pixels: exactly those with hits >= hot_min are tiles of their own, the rest is the uniform grid
    hot = np.flatnonzero(hits >= hot_min)
    assert int(r["hot.any"][0]) == (1 if len(hot) else 0)
    want = np.unique(np.concatenate([np.arange(0, npix, TP), hot, hot + 1, [npix]]))
    assert np.array_equal(r["hot.p0"], want)
    if case == "hot":
        assert list(hot) == [npix // 3]


@pytest.mark.parametrize("case", sorted(CASES))
def test_choose_tiling_follows_the_hit_map_the_order_and_the_switch(driver, case):
    kind, npix = CASES[case]
    hits = _hits(kind, npix)
    r = _run(driver, hits, HOT_MIN_FLOOR)
    loads = np.diff(r["uniform.off"])
    nvalid, ntiles = int(loads.sum()), len(loads)
    mean = float(nvalid) / float(ntiles)
    uneven = ntiles >= 64 and nvalid >= (1 << 20) and float(loads.max()) > 1.25 * mean
    assert uneven == (kind in ("uneven", "hot"))
    hot_min = max(int(0.5 * mean), HOT_MIN_FLOOR)
    UNIFORM, EQUAL, PARTS = 0, 1, 2
    for i, sw in enumerate(("automatic", "off", "cut", "parts")):
        for exact in (0, 1):
            tiling, split, hmin = (int(x) for x in r["choice.%d.%d" % (i, exact)])
            want = {"automatic": (EQUAL if exact else PARTS) if uneven else UNIFORM, "off": UNIFORM,
                    "cut": EQUAL if nvalid else UNIFORM, "parts": PARTS if nvalid else UNIFORM}[sw]
            assert tiling == want, (sw, exact)
            assert split == (1 if tiling == PARTS else 0)
            assert hmin == (hot_min if tiling == PARTS and loads.max() >= hot_min else 0)
    # slice length wanted: ~0.92 x 512 groups a slice, multiples of 64 in [256, smax], shorter when many overflow
    assert list(r["wanted"]) == [int(0.92 * 512 * 1536 / 400.0) // 64 * 64, min(int(0.92 * 512 * 1536 / 700.0) // 64 * 64,
                                                                              1536 * 7 // 8 // 64 * 64), 1536, 256]


@pytest.mark.parametrize("forced", [-1, 0, 9000])
@pytest.mark.parametrize("case", sorted(CASES))
def test_slices_items_ranges_and_parts_tile_every_bucket(driver, case, forced):
    kind, npix = CASES[case]
    hits = _hits(kind, npix)
    nvalid, base = int(hits.sum()), -(-npix // TP)
    r = _run(driver, hits, max(int(0.5 * nvalid / base), HOT_MIN_FLOOR), forced)
    for name in ("uniform", "equal", "hot"):
        p0, off = r[name + ".p0"], r[name + ".off"]
        pairs = r[name + ".pairs"].reshape(-1, 2)
        _check_pieces(off, r[name + ".slice0"], pairs[:, 0], pairs[:, 1], S)
        _check_pieces(off, r[name + ".item0"], r[name + ".item_k0"], r[name + ".item_k1"], ITEM)
        assert np.array_equal(r[name + ".item_tile"], np.repeat(np.arange(len(p0) - 1), np.diff(r[name + ".item0"])))
        # hot tiles: one pixel, at least kHotTileMin samples; their ranges tile the bucket in time order
        is_hot = (np.diff(p0) == 1) & (np.diff(off) >= HOT_MIN_FLOOR)
        assert np.array_equal(r[name + ".hot_flag"], is_hot.astype(np.int64))
        hot_tile = np.flatnonzero(is_hot)
        assert np.array_equal(r[name + ".hot_tile"], hot_tile)
        rng_ = r[name + ".hot_range"].reshape(-1, 2)
        c0 = r[name + ".hot_chunk0"]
        hoff = np.concatenate([[0], np.cumsum(np.diff(off)[hot_tile])])
        _check_pieces(hoff, c0, rng_[:, 0] - np.repeat((off[hot_tile] - hoff[:-1]), np.diff(c0)),
                      rng_[:, 1] - np.repeat((off[hot_tile] - hoff[:-1]), np.diff(c0)), CHUNK)
        tiles = r[name + ".hot_tiles"].reshape(-1, 3)
        assert np.array_equal(tiles[:, 0], p0[hot_tile]) and np.array_equal(tiles[:, 1], c0[:-1])
        assert np.array_equal(tiles[:, 2], np.diff(c0))
        assert np.array_equal(r[name + ".hot_range_tile"], np.repeat(np.arange(len(hot_tile)), np.diff(c0)))
        if name == "hot" and case == "hot":
            assert len(hot_tile) == 1 and p0[hot_tile[0]] == npix // 3
        # parts: hot tiles carry no load; never more parts than slices; the parts' slice ranges partition the
        # tile's slices in order
        load, parts, ns = r[name + ".load"], r[name + ".parts"], np.diff(r[name + ".slice0"])
        assert np.array_equal(load, np.where(is_hot, 0, np.diff(off)))
        assert np.all(parts >= 1) and np.all(parts[ns > 0] <= ns[ns > 0]) and np.all(parts[load == 0] == 1)
        ps, at = r[name + ".part_slices"], 0
        for b in range(len(parts)):
            cut = ps[at:at + parts[b] + 1]
            at += parts[b] + 1
            assert cut[0] == 0 and cut[-1] == ns[b] and np.all(np.diff(cut) >= (1 if parts[b] > 1 else 0))
        assert at == len(ps)
        target, mk = int(r[name + ".parts_target"][0]), r[name + ".parts_makespan"][0]
        whole = _makespan(load[load > 0].tolist(), SLOTS)
        if forced == 0 or load.sum() == 0:
            assert target == 0 and np.all(parts == 1)
        elif forced > 0:
            assert target == forced and mk == _makespan(_parts_items(load, ns, target), SLOTS)
        else:
            # the candidates of the search: target 0 exactly when none of them beats whole tiles by 5 %
            per_slot = float(load.sum()) / float(SLOTS)
            cands = [int(per_slot * (1.25 - 0.025 * step)) + 1 for step in range(43)]
            cands = cands[:next((i for i, t in enumerate(cands) if t < 4 * S), len(cands))]
            best = min([_makespan(_parts_items(load, ns, t), SLOTS) for t in cands], default=1e30)
            assert (target == 0) == (best > 0.95 * whole)
            if target:
                assert target in cands and mk == _makespan(_parts_items(load, ns, target), SLOTS)
                assert mk <= best + 0.01 and mk <= 0.95 * whole
                assert np.all(parts[load * 10 > target * 11] >= np.minimum(2, ns[load * 10 > target * 11]))
            if kind == "uniform" and name == "uniform":
                assert target == 0                             # (512 equal tiles on 512 slots: nothing to gain)
            if kind == "uneven" and name == "uniform":
                assert target > 0 and parts.max() > 1          # (a tenth of the tiles holds half of the samples)
        if target:
            want_parts = np.array([len(_parts_items(load[b:b + 1], ns[b:b + 1], target)) or 1 for b in range(len(load))])
            assert np.array_equal(parts, want_parts)


def test_parts_makespan_is_one_for_equal_items_and_grows_with_a_heavier_one(driver):
    def run(items, slots):
        p = subprocess.run([driver, "makespan", str(slots)], input=" ".join(map(str, items)), stdout=subprocess.PIPE,
                           text=True, check=True)
        a, b = (float(x) for x in p.stdout.split())
        assert a == b
        return a
    equal = [20000] * SLOTS
    assert run(equal, SLOTS) == 1.0
    assert run([], SLOTS) == 1.0
    last = 1.0
    for heavy in (30000, 60000, 240000):
        mk = run([heavy] + equal[1:], SLOTS)
        assert mk > last and mk == _makespan([heavy] + equal[1:], SLOTS)
        last = mk
    # one item more than slots: a second round for a single workgroup, which cannot use the whole chip
    assert run(equal + [20000], SLOTS) > 1.3


# ---------------------------------------------------------------- the fixed-order lists -------
def _fx(driver, args, stdin=""):
    p = subprocess.run([driver] + [str(a) for a in args], input=stdin, stdout=subprocess.PIPE, text=True, check=True)
    return [ln.split() for ln in p.stdout.splitlines()]


TWO_PER_CU, ONE_PER_CU = 79 * 1024, 159 * 1024                # LDS a workgroup may take for two / one to fit a CU
LDS_S = (64, 1024, 1025, 1536, 2048)


def _lds(tp, pol, S):
    return 8 * (tp * pol + 2 * max(2, -(-S // 512)) * 512 + 384)


# ((2304, 3) is the one shape class where only S = 1024 leaves room for two workgroups: the search ends there)
@pytest.mark.parametrize("tp,pol", [(256, 1), (1024, 3), (2048, 3), (4096, 3), (8192, 3), (16384, 3), (2304, 3)])
def test_lds_budget_gives_the_longest_slice_that_fits(driver, tp, pol):
    r = {ln[0]: [int(x) for x in ln[1:]] for ln in _fx(driver, ["lds", tp, pol] + list(LDS_S))}
    assert r["budgets"] == [TWO_PER_CU, ONE_PER_CU]
    assert r["bytes"] == [_lds(tp, pol, S) for S in LDS_S]
    assert r["per_cu"] == [2 if _lds(tp, pol, S) <= TWO_PER_CU else 1 for S in LDS_S]
    # the longest multiple of 512 (down to 1024) that leaves room for two workgroups a CU, when there is one;
    # otherwise the longest slice that fits once, going down in steps of 256
    two = [S for S in (2048, 1536, 1024) if _lds(tp, pol, S) <= TWO_PER_CU]
    one = [S for S in range(2048, 255, -256) if _lds(tp, pol, S) <= ONE_PER_CU]
    want = two[0] if two else (one[0] if one else 256)
    assert r["max_slice"] == [want]
    assert r["fills"] == [0 if one else 1]                    # "atomics instead" exactly when no slice fits
    if (tp, pol) == (2048, 3):
        assert want == 1536
    if (tp, pol) == (1024, 3):
        assert want == 2048
    if (tp, pol) == (16384, 3):
        assert r["fills"] == [1]
    if (tp, pol) == (2304, 3):
        assert want == 1024


def _offsets(driver, S, off, hot, counts, threads=512, shift=28):
    text = " ".join(map(str, [len(hot)] + list(off) + list(hot) + list(np.asarray(counts).ravel())))
    lines = _fx(driver, ["offsets", S, threads, shift], text)
    assert lines[:len(lines) // 2] == lines[len(lines) // 2:]  # (no hidden state)
    return {ln[0]: ln[1:] for ln in lines[:len(lines) // 2]}


def test_list_offsets_are_the_running_sums_of_the_counts(driver):
    rng = np.random.default_rng(5)
    S, threads = 256, 512
    # 8 tiles, tile 2 empty, tile 5 flagged hot; ~40 slices, the last one of most tiles shorter than S
    loads = np.array([5 * S + 17, 3 * S, 0, 7 * S + 1, 4 * S + 200, 9 * S, 6 * S + 64, S - 1])
    off = np.concatenate([[0], np.cumsum(loads)])
    hot = np.zeros(8, np.int64)
    hot[5] = 1
    ns = -(-loads // S)
    nslices = int(ns.sum())
    assert 36 <= nslices <= 44
    counts = np.stack([rng.integers(300, 700, nslices), rng.integers(0, 4, nslices), rng.integers(0, 900, nslices),
                       rng.integers(0, 15, nslices)], axis=1)
    r = _offsets(driver, S, off, hot, counts, threads)
    meta = np.array([int(x) for x in r["meta"]], np.int64).reshape(-1, 2)
    tent_off = np.array([int(x) for x in r["tent_off"]], np.int64)
    ex = np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(counts[:, :3], axis=0)])     # exclusive sums + totals
    assert len(meta) == nslices + 1 and len(tent_off) == nslices + 1
    assert np.array_equal(meta[:, 0], ex[:, 0])
    assert np.array_equal(meta[:, 1] & 0x0FFFFFFF, ex[:, 1])
    assert np.array_equal(tent_off, ex[:, 2])
    assert np.array_equal(meta[:-1, 1] >> 28, counts[:, 3]) and meta[-1, 1] >> 28 == 0
    assert [int(x) for x in r["totals"]] == list(ex[-1]) and r["fits"] == ["1"]
    # fill statistics over the tiles that are not hot: groups per FULL slice, share of ALL slices over the threads
    first = np.concatenate([[0], np.cumsum(ns)])
    gsum, nfull, nover, ncounted = 0.0, 0, 0, 0
    for b in range(8):
        if hot[b]:
            continue
        for s in range(first[b], first[b + 1]):
            ncounted += 1
            nover += int(counts[s, 0] > threads)
            if min(S, loads[b] - (s - first[b]) * S) == S:
                nfull += 1
                gsum += float(counts[s, 0])
    assert nfull < ncounted and nover > 0
    assert r["fill"] == ["%.17g" % (gsum / float(nfull)), "%.17g" % (float(nover) / float(ncounted))]
    # nothing to count: zeros, not a division by zero
    r = _offsets(driver, S, [0, 0, 0], [0, 0], [])
    assert r["fill"] == ["0", "0"] and r["totals"] == ["0", "0", "0"] and r["meta"] == ["0", "0"]


@pytest.mark.parametrize("column,limit", [(0, 1 << 32), (2, 1 << 32), (1, 1 << 28)])
@pytest.mark.parametrize("nslices", [3, 4])
def test_list_offsets_report_each_limit_at_the_limit_and_not_below(driver, column, limit, nslices):
    S = 64
    parts = [limit // 2, limit // 2 - 7, 5, 2][:nslices]
    parts[-1] += limit - sum(parts)                           # the counts of the slices sum to exactly the limit
    for short, fits in ((0, "0"), (1, "1")):
        counts = np.zeros((nslices, 4), np.int64)
        counts[:, column] = parts
        counts[-1, column] -= short
        r = _offsets(driver, S, [0, nslices * S], [0], counts)
        assert [int(x) for x in r["totals"]][(0, 1, 2)[column]] == limit - short
        assert r["fits"] == [fits]


def _wanted(S, mean, over, smax, threads=512):
    want = int(0.92 * threads * S / mean) // 64 * 64
    if over > 0.10:
        want = want if want < S * 7 // 8 else S * 7 // 8 // 64 * 64
    return max(min(want, smax), 256)


def _tune(forced, smax, sample_first, answers):
    """policy::tune_slice restated: the steps taken, the return code and the last slice length"""
    ans, steps = list(answers), []

    def step(name, S):
        steps.append([name, str(S)])
        mean, over = ans.pop(0)
        return (7 if mean < 0 else 0), mean, over
    if 64 <= forced <= 2048:
        S = min(forced, smax)
        return steps, step("build", S)[0], S
    S = min(1536, smax)
    if sample_first:
        rc, mean, over = step("count", S)
        if rc:
            return steps, rc, S
        if mean > 0.0:
            S = _wanted(S, mean, over, smax)
    rc, mean, over = step("build", S)
    if rc:
        return steps, rc, S
    for _ in range(3):
        if not mean > 0.0:
            break
        want = _wanted(S, mean, over, smax)
        close_enough = S * 15 // 16 <= want <= S * 17 // 16 and over <= 0.10
        if close_enough or want == S:
            break
        S = want
        rc, mean, over = step("build", S)
        if rc:
            return steps, rc, S
    return steps, 0, S


TUNE = {   # forced, smax, sample first, (mean, over) answers -> the slice lengths built
    "stops at once, want == S": (0, 1536, 0, [(100.0, 0.0)], [1536]),
    "stops by close_enough": (0, 2048, 0, [(0.92 * 512 * 1536 / 1500.0, 0.05)], [1536]),
    "close but many overflow": (0, 2048, 0, [(0.92 * 512 * 1536 / 1500.0, 0.3), (0.92 * 512, 0.0)], [1536, 1344]),
    "all three rebuilds": (0, 2048, 0, [(900.0, 0.0), (200.0, 0.0), (900.0, 0.0), (200.0, 0.0), (1.0, 0.0)],
                           [1536, 768, 1792, 896]),
    "forced, clamped to smax": (2000, 1536, 1, [(300.0, 0.0)], [1536]),
    "forced": (640, 1536, 1, [(300.0, 0.0)], [640]),
    "sample first": (0, 2048, 1, [(600.0, 0.0), (471.0, 0.0)], [1152]),
    "sample of nothing": (0, 1024, 1, [(0.0, 0.0), (0.0, 0.0)], [1024]),
    "a failed build ends it": (0, 2048, 0, [(900.0, 0.0), (-1.0, 0.0)], [1536, 768]),
}


@pytest.mark.parametrize("case", sorted(TUNE))
def test_slice_tuning_tries_the_lengths_the_rule_gives(driver, case):
    forced, smax, sample_first, answers, built = TUNE[case]
    out = _fx(driver, ["tune", forced, smax, sample_first], " ".join("%r %r" % a for a in answers))
    steps, rc, S = _tune(forced, smax, sample_first, answers)
    assert out == steps + [["rc", str(rc)], ["S", str(S)]]
    assert [int(s[1]) for s in steps if s[0] == "build"] == built and S == built[-1]
    assert rc == (7 if case.startswith("a failed") else 0)
    assert ("count" in [s[0] for s in steps]) == (bool(sample_first) and not 64 <= forced <= 2048)


def test_tiles_in_range_is_searchsorted_on_the_ascending_list(driver):
    asc = np.array([3, 4, 9, 17, 18, 40])
    ranges = [(0, 3), (5, 9), (10, 17), (41, 50), (7, 7),          # empty: before, between, touching, after, no width
              (4, 18), (9, 10),                                    # inside
              (3, 41), (3, 40), (4, 41),                           # touching both ends, one end
              (0, 100)]                                            # everything
    text = " ".join(map(str, asc)) + " -1 " + " ".join("%d %d" % r for r in ranges)
    got = [[int(x) for x in ln] for ln in _fx(driver, ["range"], text)]
    for (lo, hi), (a, e) in zip(ranges, got):
        assert a == np.searchsorted(asc, lo, "left") and e == max(a, np.searchsorted(asc, hi, "left")), (lo, hi)
        assert np.array_equal(asc[a:e], asc[(asc >= lo) & (asc < hi)])
    assert _fx(driver, ["range"], "-1 0 5") == [["0", "0"]]    # an empty list
