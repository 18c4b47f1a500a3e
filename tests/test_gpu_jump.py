"""
The jump corrector on the GPU against the NumPy restatement of _jump_ref.py: t compared with ==, noeval, sigma, the
table, the heights, the offsets, the corrected stream, the classes and the counts bit for bit.  The shapes are the
smallest at which the kernels can go wrong (the lists are in _jump_ref.py and checked in test_jump_cpu.py); outputs
sit in the sentinel-guarded buffers of _guarded.py.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import _jump_ref as R
from _guarded import INT_FILL, Guarded, GuardedInt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.utilities import gap_fill, jumps as J
    return SimpleNamespace(U=U, J=J, hip=_hip, torch=torch, D=D, flags_to_dev=gap_fill._flags_to_dev)


def same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


class Raw(object):
    """The C entry points on guarded buffers: every output comes back with its guards checked."""

    def __init__(self, cm, sizes, w):
        self.cm, self.sizes, self.nt, self.nb = cm, sizes, sum(sizes), len(sizes)
        self.g = cm.J._Jump(self.nt, sizes, w)
        self.st = cm.D.stream()

    def stat(self, d, flags=None, prev=None, min_count=1):
        cm = self.cm
        x = Guarded(cm, self.nt, d)
        if flags is not None and flags.dtype == np.uint8:            # bytes as a uint8 tensor brings them: kind 1
            f, kind = cm.D.to_dev(flags), 1
        else:
            f, kind = (None, 0) if flags is None else cm.flags_to_dev(flags)
        p = None if prev is None else cm.D.to_dev(prev)
        t, noeval = Guarded(cm, self.nt), GuardedInt(cm, self.nt, "uint8")
        cm.hip.call("cm2_jump_stat", self.g.h, x.ptr, cm.D.ptr(f), kind, cm.D.ptr(p), int(min_count), t.ptr,
                    noeval.ptr, self.st)
        out = t.get(), noeval.get()
        t.intact("cm2_jump_stat (t)")
        noeval.intact("cm2_jump_stat (noeval)")
        x.intact("cm2_jump_stat (input)")
        assert same_bits(x.get(), d)
        return out

    def scale(self, t, noeval):
        cm = self.cm
        tt, ne, s = Guarded(cm, self.nt, t), GuardedInt(cm, self.nt, "uint8", noeval), Guarded(cm, self.nb)
        cm.hip.call("cm2_jump_scale", self.g.h, tt.ptr, ne.ptr, s.ptr, self.st)
        out = s.get()
        s.intact("cm2_jump_scale")
        return out

    def find(self, t, noeval, sigma, nsigma, capacity, room=None):
        """the table buffers hold `room` entries (default: the capacity); they stay in self.table for correct()"""
        cm = self.cm
        room = capacity if room is None else room
        tt, ne = Guarded(cm, self.nt, t), GuardedInt(cm, self.nt, "uint8", noeval)
        s = Guarded(cm, self.nb, np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (self.nb,))))
        pos, hgt, off = GuardedInt(cm, room, "int64"), Guarded(cm, room), Guarded(cm, room)
        nj = GuardedInt(cm, self.nb + 1, "int64")
        cm.hip.call("cm2_jump_find", self.g.h, tt.ptr, ne.ptr, s.ptr, float(nsigma), int(capacity), pos.ptr, hgt.ptr,
                    off.ptr, nj.ptr, self.st)
        out = SimpleNamespace(pos=pos.get(), heights=hgt.get(), offsets=off.get(), njumps=nj.get())
        for buf, what in ((pos, "positions"), (hgt, "heights"), (off, "offsets"), (nj, "njumps")):
            buf.intact("cm2_jump_find (%s)" % what)
        self.table = SimpleNamespace(pos=pos, offsets=off, njumps=nj, capacity=int(capacity))
        return out

    def correct(self, d, prev, radius, in_place=False):
        cm, tb = self.cm, self.table
        x = Guarded(cm, self.nt, d)
        o = x if in_place else Guarded(cm, self.nt)
        p = None if prev is None else cm.D.to_dev(prev)
        cls, counts = GuardedInt(cm, self.nt, "uint8"), GuardedInt(cm, 3 * self.nb, "int64")
        cm.hip.call("cm2_jump_correct", self.g.h, x.ptr, cm.D.ptr(p), tb.pos.ptr, tb.offsets.ptr, tb.njumps.ptr,
                    tb.capacity, int(radius), o.ptr, cls.ptr, counts.ptr, self.st)
        out = o.get(), cls.get(), counts.get().reshape(self.nb, 3)
        for buf, what in ((o, "d_out"), (cls, "classes"), (counts, "counts"), (x, "input")):
            buf.intact("cm2_jump_correct (%s)" % what)
        return out


def check_table(got, want, capacity):
    n = want.pos.size
    assert got.njumps.tolist() == want.njumps.tolist() + [n]
    assert np.array_equal(got.pos[:n], want.pos), (got.pos[:n], want.pos)
    assert same_bits(got.heights[:n], want.heights) and same_bits(got.offsets[:n], want.offsets)
    assert (got.pos[n:] == INT_FILL["int64"]).all()                       # nothing beyond the jumps is written
    assert np.isnan(got.heights[n:]).all() and np.isnan(got.offsets[n:]).all()


def check_corrected(got, want):
    out, cls, counts = got
    bad = np.flatnonzero(R.bits(out) != R.bits(want.d_out))
    assert bad.size == 0, (bad[:10], out[bad[:10]], want.d_out[bad[:10]])
    assert np.array_equal(cls, want.cls), np.flatnonzero(cls != want.cls)[:10]
    assert np.array_equal(counts, want.counts)


# ------------------------------------------------------------------------- one whole pass ----
@pytest.mark.parametrize("name", R.STREAM_CASES)
def test_one_pass_of_the_stream_cases(cm, name):
    c, want = R.stream_case(name), R.stream_expected(name)
    raw = Raw(cm, c.sizes, c.w)
    t, noeval = raw.stat(c.d, c.flags, c.prev, c.min_count)
    bad = np.flatnonzero(~(t == want.t))
    assert bad.size == 0, (name, bad[:10], t[bad[:10]], want.t[bad[:10]])
    assert same_bits(t[noeval == 1], np.zeros(int(noeval.sum())))         # +0.0 where not evaluable
    assert np.array_equal(noeval, want.noeval), np.flatnonzero(noeval != want.noeval)[:10]
    sigma = raw.scale(t, noeval)
    assert same_bits(sigma, want.sigma), (name, sigma, want.sigma)
    capacity = max(1, want.pos.size) + 3
    check_table(raw.find(t, noeval, want.sigma_used, c.nsigma, capacity), want, capacity)
    check_corrected(raw.correct(c.d, c.prev, c.radius), want)
    info = raw.g.info()
    assert (info["nt"], info["nblocks"], info["half_window"], info["tile"], info["lds_bytes"]) == \
        (sum(c.sizes), len(c.sizes), c.w, R.TILE, R.stat_lds_bytes(c.w))
    assert info["bytes"] >= sum(c.sizes) + 2 * 8 * (len(c.sizes) + 1) + 8192 * len(c.sizes)


# ------------------------------------------------------ peaks, table, offsets and classes ----
@pytest.mark.parametrize("name", R.PEAK_CASES)
def test_peaks_offsets_and_classes(cm, name):
    c, want = R.peak_case(name), R.peak_expected(name)
    raw = Raw(cm, c.sizes, c.w)
    capacity = max(1, want.pos.size) + 2
    for _ in range(2):                                                    # the second call finds the marks rewritten
        check_table(raw.find(c.t, c.noeval, c.sigma, c.nsigma, capacity), want, capacity)
    check_corrected(raw.correct(c.d, want.prev, c.radius), want)
    check_corrected(raw.correct(c.d, want.prev, c.radius, in_place=True), want)


def test_scale_of_made_up_statistics(cm):
    t, noeval, sizes = R.scale_cases()
    want, eb = R.scale(t, noeval, sizes)
    raw = Raw(cm, sizes, 3)
    for _ in range(2):                                                    # the second call finds the histograms cleared
        sigma = raw.scale(t, noeval)
        assert same_bits(sigma, want), (sigma, want)


@pytest.mark.parametrize("short", [0, 1, 400])
def test_capacity_reached_and_exceeded(cm, short):
    c, want = R.peak_case("many"), R.peak_expected("many")
    n = want.pos.size
    capacity = n - short
    raw = Raw(cm, c.sizes, c.w)
    got = raw.find(c.t, c.noeval, c.sigma, c.nsigma, capacity, room=n + 4)
    assert got.njumps.tolist() == want.njumps.tolist() + [n]              # the true counts
    assert np.array_equal(got.pos[:capacity], want.pos[:capacity])
    assert same_bits(got.heights[:capacity], want.heights[:capacity])
    assert same_bits(got.offsets[:capacity], want.offsets[:capacity])
    assert (got.pos[capacity:] == INT_FILL["int64"]).all()                # nothing beyond the capacity
    assert np.isnan(got.heights[capacity:]).all() and np.isnan(got.offsets[capacity:]).all()
    jc = cm.U.JumpCorrector(c.sizes, half_window=c.w)
    t, noeval = cm.D.f64(c.t), cm.D.to_dev(c.noeval)
    if short:
        with pytest.raises(RuntimeError) as e:
            jc.find(t, noeval, c.sigma, nsigma=c.nsigma, capacity=capacity)
        assert str(n) in str(e.value) and "capacity" in str(e.value)
        d = cm.D.f64(c.d)
        with pytest.raises(RuntimeError):
            jc.run(d, sigma=1e-3, nsigma=c.nsigma, capacity=1, iterations=1)    # (noise: a jump every few samples)
        assert same_bits(cm.D.to_host(d), c.d)                            # raised before correcting
    else:
        table = jc.find(t, noeval, c.sigma, nsigma=c.nsigma, capacity=capacity)
        assert table.total == n and np.array_equal(cm.D.to_host(table.positions), want.pos)


# --------------------------------------------------------------------- the Python layer ----
def test_python_layer_gives_the_same_pass(cm):
    c, want = R.stream_case("min_count_flags_and_prev"), R.stream_expected("min_count_flags_and_prev")
    jc = cm.U.JumpCorrector(c.sizes, half_window=c.w)
    for d, flags, prev in ((c.d, c.flags, c.prev), (cm.D.f64(c.d), cm.D.i32(c.flags), cm.D.to_dev(c.prev)),
                           (c.d, c.flags < 0, c.prev), (c.d, c.flags.astype(np.int64), c.prev)):
        t, noeval = jc.statistic(d, flags=flags, classes=prev, min_count=c.min_count)
        assert cm.D.is_dev(t) and t.dtype == cm.torch.float64 and noeval.dtype == cm.torch.uint8
        assert (cm.D.to_host(t) == want.t).all() and np.array_equal(cm.D.to_host(noeval), want.noeval)
        sigma = jc.scale(t, noeval)
        assert cm.D.is_dev(sigma) and same_bits(cm.D.to_host(sigma), want.sigma)
        for s in (c.sigma, [c.sigma] * 2, cm.D.f64(np.full(2, c.sigma))):
            table = jc.find(t, noeval, s, nsigma=c.nsigma)
            assert table.total == want.pos.size and table.njumps.tolist() == want.njumps.tolist()
            assert np.array_equal(cm.D.to_host(table.positions)[:table.total], want.pos)
            assert same_bits(cm.D.to_host(table.heights)[:table.total], want.heights)
        out, cls, counts = jc.correct(d, table, classes=prev, radius=c.radius)
        assert cm.D.is_dev(out) and cm.D.is_dev(cls) and cls.dtype == cm.torch.uint8
        check_corrected((cm.D.to_host(out), cm.D.to_host(cls), counts), want)
        if cm.D.is_dev(d):
            assert out.data_ptr() != d.data_ptr() and same_bits(cm.D.to_host(d), c.d)     # the input is left alone
            same = jc.correct(d, table, classes=prev, radius=c.radius, out=d)[0]
            assert same.data_ptr() == d.data_ptr() and same_bits(cm.D.to_host(d), want.d_out)
    host = np.empty(c.d.size)
    assert jc.correct(c.d, table, classes=c.prev, radius=c.radius, out=host)[0] is host and same_bits(host, want.d_out)
    assert jc.info(sum(c.sizes))["half_window"] == c.w


def test_run_with_the_default_min_count_and_the_robust_scale(cm):
    c = R.stream_case("sizes_w64")
    want_out, want_cls, winfo = R.run(c.d, c.sizes, c.w, flags=c.flags, nsigma=c.nsigma, radius=c.radius,
                                      iterations=2)
    out, cls, info = cm.U.correct_jumps(c.d, c.sizes, flags=c.flags, half_window=c.w, nsigma=c.nsigma,
                                        radius=c.radius, iterations=2)
    check_corrected((cm.D.to_host(out), cm.D.to_host(cls), info["counts"]),
                    SimpleNamespace(d_out=want_out, cls=want_cls, counts=winfo["counts"]))
    assert info["passes"] == winfo["passes"] and np.array_equal(info["positions"], winfo["positions"])
    assert same_bits(info["heights"], winfo["heights"])
    assert info["short_blocks"].tolist() == winfo["short_blocks"].tolist() == [0, 1, 2, 3]
    assert all(same_bits(a, b) for a, b in zip(info["sigma"], winfo["sigma"]))


# --------------------------------------------------------------------------- iteration ----
def test_iteration_finds_the_hidden_jump_in_the_second_pass(cm):
    c = R.iteration_case()
    jc = cm.U.JumpCorrector(c.sizes, half_window=c.w)
    d = cm.D.f64(c.d)
    out, cls, info = jc.run(d, nsigma=6.0, radius=4, iterations=3)
    assert same_bits(cm.D.to_host(d), c.d) and out.data_ptr() != d.data_ptr()
    assert info["passes"] == c.info["passes"] == 3 and info["found_in_pass"].tolist() == [0, 1]
    assert np.array_equal(info["positions"], c.info["positions"]) and same_bits(info["heights"], c.info["heights"])
    check_corrected((cm.D.to_host(out), cm.D.to_host(cls), info["counts"]),
                    SimpleNamespace(d_out=c.d_out, cls=c.cls, counts=c.info["counts"]))
    assert all(same_bits(a, b) for a, b in zip(info["sigma"], c.info["sigma"])) and len(info["sigma"]) == 3
    assert info["short_blocks"].size == 0
    for k in (1, 2):                                                  # stopped early: the stream of that pass
        out_k, cls_k, info_k = jc.run(c.d, nsigma=6.0, radius=4, iterations=k)
        each = c.info["each"][k - 1]
        check_corrected((cm.D.to_host(out_k), cm.D.to_host(cls_k), info_k["counts"]), each)
        assert info_k["passes"] == k
    inplace = cm.D.f64(c.d)                                           # in place: out is d
    out, cls, info = jc.run(inplace, nsigma=6.0, radius=4, iterations=3, out=inplace)
    assert out.data_ptr() == inplace.data_ptr() and same_bits(cm.D.to_host(inplace), c.d_out)


# ------------------------------------------------------------------ guards and overlap ----
def test_overlaps_and_bad_arguments_are_refused(cm):
    nt, sizes, w = 1000, [600, 400], 4
    g = cm.J._Jump(nt, sizes, w)
    buf = Guarded(cm, 2 * nt, np.zeros(2 * nt))
    before = buf.get()
    p = buf.ptr
    t = cm.torch
    sig, ne, cls = cm.D.zeros(2), cm.D.zeros(nt, t.uint8), cm.D.zeros(nt, t.uint8)
    pos, hgt, off = cm.D.zeros(8, t.int64), cm.D.zeros(8), cm.D.zeros(8)
    nj, counts = cm.D.zeros(3, t.int64), cm.D.zeros(6, t.int64)
    P = cm.D.ptr
    st = cm.D.stream()

    def refused(name, *args):
        with pytest.raises(cm.hip.HipError) as e:
            cm.hip.call(name, *args)
        assert e.value.status == cm.hip.ERR_ARGUMENT and name in str(e.value), str(e.value)

    refused("cm2_jump_stat", g.h, p, None, 0, None, 2, p, P(ne), st)                      # t is d_in
    refused("cm2_jump_stat", g.h, p, None, 0, None, 2, p + 8 * (nt - 1), P(ne), st)       # one shared sample
    refused("cm2_jump_stat", g.h, p, None, 0, None, 2, p + 8 * nt, p + 8, st)             # noeval inside d_in
    refused("cm2_jump_stat", g.h, p, None, 0, P(ne), 2, p + 8 * nt, P(ne), st)            # noeval is prev
    refused("cm2_jump_stat", g.h, p, P(cls), 2, None, 2, p + 8 * nt, P(ne), st)           # flag_kind
    refused("cm2_jump_stat", g.h, p, None, 0, None, 0, p + 8 * nt, P(ne), st)             # min_count
    refused("cm2_jump_stat", g.h, p, None, 0, None, w + 1, p + 8 * nt, P(ne), st)
    refused("cm2_jump_stat", g.h, p, None, 0, None, 2, None, P(ne), st)
    refused("cm2_jump_scale", g.h, p, P(ne), p + 8, st)                                   # sigma inside t
    refused("cm2_jump_find", g.h, p, P(ne), P(sig), 0.0, 8, P(pos), P(hgt), P(off), P(nj), st)
    refused("cm2_jump_find", g.h, p, P(ne), P(sig), float("inf"), 8, P(pos), P(hgt), P(off), P(nj), st)
    refused("cm2_jump_find", g.h, p, P(ne), P(sig), 5.0, 0, P(pos), P(hgt), P(off), P(nj), st)          # capacity
    refused("cm2_jump_find", g.h, p, P(ne), P(sig), 5.0, 8, P(pos), p + 16, P(off), P(nj), st)          # heights in t
    refused("cm2_jump_find", g.h, p, P(ne), P(sig), 5.0, 8, P(pos), P(hgt), P(hgt), P(nj), st)          # two outputs
    refused("cm2_jump_correct", g.h, p, None, P(pos), P(off), P(nj), 8, 257, p + 8 * nt, P(cls), P(counts), st)
    refused("cm2_jump_correct", g.h, p, None, P(pos), P(off), P(nj), 8, -1, p + 8 * nt, P(cls), P(counts), st)
    refused("cm2_jump_correct", g.h, p, None, P(pos), P(off), P(nj), 8, 2, p + 8, P(cls), P(counts), st)   # shifted
    refused("cm2_jump_correct", g.h, p, P(cls), P(pos), P(off), P(nj), 8, 2, p + 8 * nt, P(cls), P(counts), st)
    refused("cm2_jump_correct", g.h, p, None, P(pos), P(off), P(nj), 8, 2, p + 8 * nt, P(cls), P(nj), st)
    assert same_bits(buf.get(), before)
    buf.intact("refused calls")
    # d_out == d_in is the one overlap that is taken; t right behind d_in is none
    cm.hip.call("cm2_jump_stat", g.h, p, None, 0, None, 2, p + 8 * nt, P(ne), st)
    cm.hip.call("cm2_jump_find", g.h, p + 8 * nt, P(ne), P(sig), 5.0, 8, P(pos), P(hgt), P(off), P(nj), st)
    cm.hip.call("cm2_jump_correct", g.h, p, None, P(pos), P(off), P(nj), 8, 2, p, P(cls), P(counts), st)
    assert not buf.get().any() and cm.D.to_host(nj).tolist() == [0, 0, 0]
    assert cm.D.to_host(counts).tolist() == [600, 0, 0, 400, 0, 0]
    buf.intact("the accepted calls")


# --------------------------------------------------------------------------- end to end ----
def test_end_to_end_after_the_glitch_flags(cm):
    q, e = R.quality_case(glitches=40), R.end_to_end_expected()
    d, pix = cm.D.f64(q.d), cm.D.i32(q.pix)
    gcls, ginfo = cm.U.flag_glitches(d, q.sizes, flags=pix, half_width=16, nsigma=5.0, grow=2, iterations=3)
    assert np.array_equal(cm.D.to_host(gcls), e.gcls)
    out, cls, info = cm.U.correct_jumps(d, q.sizes, flags=pix, classes=gcls, half_window=q.w,
                                        nsigma=R.QUALITY_NSIGMA, radius=4, iterations=3)
    got = cm.D.to_host(out)
    check_corrected((got, cm.D.to_host(cls), info["counts"]),
                    SimpleNamespace(d_out=e.d_out, cls=e.cls, counts=e.info["counts"]))
    assert np.array_equal(info["positions"], e.info["positions"]) and same_bits(info["heights"], e.info["heights"])
    assert info["passes"] == e.info["passes"] and info["found_in_pass"].tolist() == e.info["found_in_pass"].tolist()
    assert all(same_bits(a, b) for a, b in zip(info["sigma"], e.info["sigma"])) and info["short_blocks"].size == 0
    # every injected jump within 3 samples, nothing else
    pos = info["positions"]
    assert pos.size == q.where.size and (np.abs(np.sort(pos) - q.where) <= 3).all()
    # the low bins of the GPU's own Welch PSD: the jumps are gone from them
    power = {}
    for name, x in (("clean", q.clean), ("uncorrected", q.d), ("corrected", got)):
        f, psd = cm.U.noise_psd(x, q.sizes, R.QUALITY_L)
        power[name] = float(np.mean(cm.D.to_host(psd).reshape(len(q.sizes), -1)[:, 1:6]))
    print("low-bin power:", power)
    assert power["corrected"] <= 20.0 * power["clean"]
    assert power["uncorrected"] >= 100.0 * power["corrected"]
    pixs = cm.U.apply_flags(pix, cls)                                     # the classes flag the samples as any others
    assert np.array_equal(cm.D.to_host(pixs) < 0, (q.pix < 0) | (e.cls != 0))
