"""
CPU tests of the file formats either side of the solve: the pure-Python
HDF5 subset (cosmomap2_amd/utilities/hdf5_lite.py) against files the reference's h5py code
wrote, the CES readers and the Ritz-vector checkpoint.  No GPU: NumPy arrays only.
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def U():
    import cosmomap2_amd.utilities as U
    return U


@pytest.mark.parametrize("case", [3, 4])
def test_reader_on_the_reference_data_files(U, case):
    """data/testcase_block_diag_{3,4}.hdf5 of the reference (h5py, big-endian datasets) through
    the reader, against the arrays an independent minimal parser extracted from them
    (tests/golden/make_hdf5_fixtures.py)."""
    from cosmomap2_amd.utilities import hdf5_lite as h5
    ref = np.load(os.path.join(GOLD, "reference_inputs.npz"))
    path = os.path.join(GOLD, "testcase_block_diag_%d.hdf5" % case)
    f = h5.read_file(path)
    assert list(f) == ["bolo_pair"] and sorted(f["bolo_pair"]) == ["pixel", "pol_angle", "sum", "weight"]
    for key in ("pixel", "pol_angle", "sum", "weight"):
        want = ref["case%d_%s" % (case, key)]
        got = f["bolo_pair"][key]
        assert got.dtype == want.dtype and got.shape == want.shape
        np.testing.assert_array_equal(got, want)
    det, pix, phi, w = U.read_from_hdf5(path)                 # IOfiles.py:317-330 return order
    np.testing.assert_array_equal(det, ref["case%d_sum" % case])
    np.testing.assert_array_equal(pix, ref["case%d_pixel" % case])
    np.testing.assert_array_equal(phi, ref["case%d_pol_angle" % case])
    np.testing.assert_array_equal(w, ref["case%d_weight" % case])


def test_write_to_hdf5_reproduces_the_reference_files_content(U, tmp_path):
    """write_to_hdf5 (IOfiles.py:277-300) followed by the reader gives back the inputs; the
    datasets are stored big-endian like the reference's, and the object headers carry the same
    messages as the h5py-written file (dataspace, datatype, fill value, layout)."""
    from cosmomap2_amd.utilities import hdf5_lite as h5
    ref = np.load(os.path.join(GOLD, "reference_inputs.npz"))
    p = str(tmp_path / "t.hdf5")
    U.write_to_hdf5(p, ref["case3_pixel"], ref["case3_weight"], ref["case3_sum"], phi=ref["case3_pol_angle"])
    det, pix, phi, w = U.read_from_hdf5(p)
    np.testing.assert_array_equal(det, ref["case3_sum"])
    np.testing.assert_array_equal(pix, ref["case3_pixel"])
    np.testing.assert_array_equal(phi, ref["case3_pol_angle"])
    np.testing.assert_array_equal(w, ref["case3_weight"])

    def dataset_messages(path, name):
        data = open(path, "rb").read()
        R = h5._Reader(data)
        for t, q, s in R.messages(R.root_header):
            if t == 0x11:
                (g, ga), = R.group_entries(R.u64(q), R.u64(q + 8))
        for t, q, s in R.messages(ga):
            if t == 0x11:
                ents = dict(R.group_entries(R.u64(q), R.u64(q + 8)))
        return {t: data[q:q + s] for t, q, s in R.messages(ents[name])}
    theirs = dataset_messages(os.path.join(GOLD, "testcase_block_diag_3.hdf5"), "pixel")
    ours = dataset_messages(p, "pixel")
    assert ours[0x03] == theirs[0x03]                         # datatype message: STD_I32BE
    assert ours[0x05] == theirs[0x05]                         # fill-value message
    assert ours[0x08][:2] == theirs[0x08][:2] == b"\x03\x01"  # layout v3, contiguous
    assert dataset_messages(p, "sum")[0x03] == dataset_messages(
        os.path.join(GOLD, "testcase_block_diag_3.hdf5"), "sum")[0x03]     # IEEE_F64BE


@pytest.mark.parametrize("case", [3, 4])
def test_written_files_are_read_by_the_independent_walker(U, tmp_path, case):
    """The writer's second reader: the minimal walker of tests/golden/make_hdf5_fixtures.py shares
    no code with hdf5_lite (it was written against the h5py files of the reference, where it
    produced the committed golden arrays) and follows the format by fixed offsets -- superblock
    v0, root symbol table, one B-tree leaf, one SNOD, v1 object headers, contiguous v3 layout.  A
    file from write_to_hdf5 (IOfiles.py:277-300) goes through it unchanged."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_hdf5_fixtures", os.path.join(GOLD, "make_hdf5_fixtures.py"))
    walker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(walker)                           # defines parse(); main() is not run
    ref = np.load(os.path.join(GOLD, "reference_inputs.npz"))
    want = {k: ref["case%d_%s" % (case, k)] for k in ("pixel", "pol_angle", "sum", "weight")}
    assert set(walker.parse(os.path.join(GOLD, "testcase_block_diag_%d.hdf5" % case))) == set(want)
    p = str(tmp_path / "w.hdf5")
    U.write_to_hdf5(p, want["pixel"], want["weight"], want["sum"], phi=want["pol_angle"])
    got = walker.parse(p)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k])
    # and a file of other sizes and values than the reference's two
    rng = np.random.default_rng(case)
    n = 1000 * case + 7
    pix = rng.integers(0, 12 * 64 * 64, n).astype(np.int32)
    w = rng.standard_normal((case, 5))
    s, phi = rng.standard_normal(n), rng.uniform(0, np.pi, n)
    U.write_to_hdf5(p, pix, w, s, phi=phi)
    got = walker.parse(p)
    for k, v in (("pixel", pix), ("weight", w), ("sum", s), ("pol_angle", phi)):
        np.testing.assert_array_equal(got[k], v)


def test_hdf5_lite_round_trip_groups_scalars_and_many_links(tmp_path):
    from cosmomap2_amd.utilities import hdf5_lite as h5
    rng = np.random.default_rng(0)
    tree = {"a": rng.standard_normal((7, 3)), "n": np.array(5, dtype=">i4"),
            "empty": np.zeros(0), "f4": rng.standard_normal(9).astype("<f4"),
            "u": np.arange(4, dtype="<u8"),
            "g": {"h": {"x": np.arange(6, dtype=">i4").reshape(2, 3)}},
            "many": {"bolo_pair_%d" % i: {"pixel": np.arange(i + 1, dtype=">i4")} for i in range(200)}}
    p = str(tmp_path / "rt.h5")
    h5.write_file(p, tree)
    g = h5.read_file(p)

    def same(a, b):
        if isinstance(a, dict):
            assert sorted(a) == sorted(b)
            for k in a:
                same(a[k], b[k])
        else:
            assert a.shape == np.asarray(b).shape and a.dtype == np.asarray(b).dtype.newbyteorder("=")
            np.testing.assert_array_equal(a, b)
    same(g, tree)
    # chunked, unfiltered datasets (the reference's Ritz writer passes chunks=True): chunk grid
    # with padded edge chunks, 1-d and 2-d, big- and little-endian
    big = rng.standard_normal((37, 10))
    ctree = {"Ritz_eigenvectors": {"Eigenvectors": h5.Chunked(big, (16, 4)),
                                   "n_eigenvectors": np.array(10, dtype=">i4")},
             "v": h5.Chunked(np.arange(23, dtype=">i4"), (5,))}
    pc = str(tmp_path / "chunked.h5")
    h5.write_file(pc, ctree)
    gc = h5.read_file(pc)
    np.testing.assert_array_equal(gc["Ritz_eigenvectors"]["Eigenvectors"], big)
    np.testing.assert_array_equal(gc["v"], np.arange(23))
    # more chunks than one B-tree leaf indexes (64): written with coarser chunks, same array back
    h5.write_file(str(tmp_path / "many.h5"), {"x": h5.Chunked(np.arange(1000.0), (1,))})
    np.testing.assert_array_equal(h5.read_file(str(tmp_path / "many.h5"))["x"], np.arange(1000.0))
    with pytest.raises(h5.Hdf5FormatError):
        h5._Reader(b"not an hdf5 file at all")
    with pytest.raises(h5.Hdf5FormatError):
        h5.write_file(str(tmp_path / "bad.h5"), {"s": np.array(["text"])})


def _write_ces(path, rng, npairs, ns, sub_n, sub_t, npix):
    from cosmomap2_amd.utilities import hdf5_lite as h5
    tree = {"obspix": np.arange(100, 100 + npix, dtype=">i4"),
            "n_bolo_pair": np.array(npairs, dtype=">i4"), "n_sample_ces": np.array(ns, dtype=">i4"),
            "subscans": {"n_sample": np.asarray(sub_n, dtype=">i4"), "t_start": np.asarray(sub_t, dtype=">i4")}}
    for i in range(npairs):
        tree["bolo_pair_%d" % i] = {
            "pixel": rng.integers(0, npix, ns).astype(">i4"), "pol_angle": rng.random(ns).astype(">f8"),
            "ground": rng.integers(0, 20, ns).astype(">f8"), "sum": rng.random(ns).astype(">f8"),
            "dif": rng.random(ns).astype(">f8"), "weight_sum": np.array(1.0 + i, dtype=">f8"),
            "weight_dif": np.array(2.0 + i, dtype=">f8")}
    h5.write_file(path, tree)
    return tree


def test_ces_readers(U, tmp_path):
    """read_from_data / read_from_data_with_subscan_resize / read_multiple_ces
    (IOfiles.py:18-210) on two synthetic scans in the AnalysisBackend layout."""
    rng = np.random.default_rng(3)
    ns, npairs, npix = 120, 3, 30
    sub_n, sub_t = [30, 40, 25], [5, 40, 90]
    paths, trees = [], []
    for k in range(2):
        p = str(tmp_path / ("ces%d.hdf5" % k))
        trees.append(_write_ces(p, rng, npairs, ns, sub_n, sub_t, npix))
        paths.append(p)
    d, w, phi, pix, hp, ground, n_ces = U.read_from_data(paths[0], 3)
    assert n_ces == ns and d.shape == (npairs * ns,) and w.tolist() == [2.0, 3.0, 4.0]
    np.testing.assert_array_equal(d[ns:2 * ns], trees[0]["bolo_pair_1"]["dif"])
    np.testing.assert_array_equal(pix[:ns], trees[0]["bolo_pair_0"]["pixel"])
    np.testing.assert_array_equal(hp, np.arange(100, 130))
    assert ground.dtype.kind == "i"
    d1, w1 = U.read_from_data(paths[0], 1, npairs=2)[:2]
    assert d1.shape == (2 * ns,) and w1.tolist() == [1.0, 2.0]
    np.testing.assert_array_equal(d1[:ns], trees[0]["bolo_pair_0"]["sum"])
    out = U.read_from_data_with_subscan_resize(paths[0], 2)
    pr = out[3][:ns]
    keep = np.zeros(ns, dtype=bool)
    for t, n in zip(sub_t, sub_n):
        keep[t:t + n] = True
    keep[sub_t[-1] + sub_n[-1]:] = True            # the reference leaves the tail unflagged (:149-155)
    np.testing.assert_array_equal(pr[~keep], -1)
    np.testing.assert_array_equal(pr[keep], np.asarray(trees[0]["bolo_pair_0"]["pixel"])[keep])
    assert out[7] == npairs and out[8][0].tolist() == sub_n and out[8][1].tolist() == sub_t
    res = U.read_multiple_ces(paths, 3)
    assert len(res) == 10 and res[0].shape == (2 * npairs * ns,) and res[1].shape == (2 * npairs,)
    assert res[8] == [ns, ns] and res[9] == [npairs, npairs]
    assert [s.tolist() for s in res[6]] == [sub_n, sub_n] and [s.tolist() for s in res[7]] == [sub_t, sub_t]
    res2 = U.read_multiple_ces(paths, 1, filtersubscan=False)
    assert len(res2) == 8 and res2[0].shape == (2 * npairs * ns,)
    a, b = np.array([1, 2, 3, 4]), np.array([2, 3, 4, 5])
    U.flagging_not_in_allCES([a, b])
    assert a.tolist() == [-1, 2, 3, 4] and b.tolist() == [2, 3, 4, -1]


def test_ritz_checkpoint_and_map_lists(U, tmp_path):
    """write_ritz_eigenvectors_to_hdf5 / read_ritz_eigenvectors_from_hdf5 (IOfiles.py:214-256):
    reference dataset names, values back bit for bit; save_maplist / read_maplist (:351-375);
    obspix (:258-275)."""
    from cosmomap2_amd.utilities import hdf5_lite as h5
    rng = np.random.default_rng(5)
    z, ev = rng.standard_normal((301, 6)), np.sort(rng.random(6))
    p = str(tmp_path / "ritz.hdf5")
    U.write_ritz_eigenvectors_to_hdf5(z, p, eigvals=ev)
    f = h5.read_file(p)
    assert sorted(f) == ["Ritz_eigenvalues", "Ritz_eigenvectors"]
    assert sorted(f["Ritz_eigenvectors"]) == ["Eigenvectors", "n_eigenvectors"]
    z2, n2, ev2 = U.read_ritz_eigenvectors_from_hdf5(p, eigvals=True)
    np.testing.assert_array_equal(z2, z)
    np.testing.assert_array_equal(ev2, ev)
    assert int(n2) == 6
    assert len(U.read_ritz_eigenvectors_from_hdf5(p)) == 2
    fn = U.write_ritz_eigenvectors(z, str(tmp_path / "ck"))
    assert fn.endswith("ck.hdf5")
    np.testing.assert_array_equal(U.read_ritz_eigenvectors(str(tmp_path / "ck")), z)
    maps = [rng.standard_normal(12), rng.standard_normal(12)]
    U.save_maplist(maps, str(tmp_path / "maps.h5"))
    got, n = U.read_maplist(str(tmp_path / "maps.h5"))
    assert n == 2 and all(np.array_equal(a, b) for a, b in zip(got, maps))
    U.write_obspix_to_hdf5(str(tmp_path / "o.h5"), np.array([5, 9, 11]))
    assert U.read_obspix_from_hdf5(str(tmp_path / "o.h5")).tolist() == [5, 9, 11]


# ------------------------------------------------------------------ HEALPix FITS -----
REF_FITS = os.path.join(GOLD, "reference_cmb_map_head.fits")


def test_healpix_fits_write_read_round_trip(tmp_path):
    """hp.write_map / hp.read_map stand-ins: one and three maps, float32 (healpy's default) and
    float64, header keywords of a HEALPix map file, 2880-byte blocking."""
    from cosmomap2_amd.utilities import healpix_fits as hf
    rng = np.random.default_rng(9)
    nside = 16
    npix = 12 * nside * nside
    I, Q, U = rng.standard_normal((3, npix))
    p = str(tmp_path / "iqu.fits")
    hf.write_map(p, [I, Q, U])
    assert os.path.getsize(p) % 2880 == 0
    a, b, c, h = hf.read_map(p, field=[0, 1, 2], h=True)
    for got, want in ((a, I), (b, Q), (c, U)):
        np.testing.assert_array_equal(got, want.astype(np.float32).astype(np.float64))
    assert h["PIXTYPE"] == "HEALPIX" and h["ORDERING"] == "RING" and h["NSIDE"] == nside
    assert h["FIRSTPIX"] == 0 and h["LASTPIX"] == npix - 1 and h["INDXSCHM"] == "IMPLICIT"
    assert h["TFORM1"] == "1024E" and h["TTYPE2"] == "Q_POLARISATION" and h["TFIELDS"] == 3
    np.testing.assert_array_equal(hf.read_map(p), a)                     # field=0 by default
    assert len(hf.read_map(p, field=None)) == 3
    p1 = str(tmp_path / "t.fits")
    hf.write_map(p1, I, dtype=np.float64, nest=True)
    np.testing.assert_array_equal(hf.read_map(p1, nest=True), I)
    np.testing.assert_array_equal(hf.read_map(p1, nest=None), I)
    # a NESTED file read with healpy's default nest=False comes back in RING ordering
    np.testing.assert_array_equal(hf.read_map(p1, nest=False), hf.reorder(I, n2r=True))
    np.testing.assert_array_equal(hf.read_map(p1), hf.reorder(I, n2r=True))
    np.testing.assert_array_equal(hf.read_map(p, nest=True),
                                  hf.reorder(I.astype(np.float32).astype(np.float64), r2n=True))
    small = rng.standard_normal(12 * 2 * 2)                              # npix not a multiple of 1024
    hf.write_map(p1, small, dtype=np.float64)
    np.testing.assert_array_equal(hf.read_map(p1), small)
    with pytest.raises(ValueError):
        hf.write_map(p1, np.zeros(100))
    with pytest.raises(hf.FitsFormatError):
        open(p1, "wb").write(b"junk" * 1000)
        hf.read_map(p1)


def _ring_centres(nside):
    """(z, phi) of every pixel centre in RING order, ring by ring from the pixelisation's
    definition (Gorski et al. 2005, eqs. 2-9)."""
    z, phi = [], []
    for i in range(1, 4 * nside):
        if i < nside:                                   # north polar cap: 4 i pixels
            n, zz = 4 * i, 1.0 - i * i / (3.0 * nside * nside)
            ph = (np.arange(1, n + 1) - 0.5) * np.pi / (2.0 * i)
        elif i <= 3 * nside:                            # equatorial belt: 4 nside pixels
            n, zz = 4 * nside, 4.0 / 3.0 - 2.0 * i / (3.0 * nside)
            # pixels of a ring are numbered by increasing phi in [0, 2 pi): every other ring is
            # shifted by half a pixel, the others have a pixel centre at phi = 0
            fodd = 1.0 if (i + nside) % 2 else 0.5
            ph = (np.arange(1, n + 1) - fodd) * np.pi / (2.0 * nside)
        else:                                           # south polar cap
            k = 4 * nside - i
            n, zz = 4 * k, -(1.0 - k * k / (3.0 * nside * nside))
            ph = (np.arange(1, n + 1) - 0.5) * np.pi / (2.0 * k)
        z += [zz] * n
        phi += list(ph)
    return np.array(z), np.array(phi)


def _nest_centres(nside):
    """(z, phi) of every pixel centre in NESTED order from the face geometry: base face f, cell
    (ix, iy) of its nside x nside grid (the HEALPix C++ pix2loc, floating point on purpose: no ring
    offsets, no shift bit)."""
    jrll = [2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4]
    jpll = [1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7]
    z, phi = [], []
    for p in range(12 * nside * nside):
        f, ipf = divmod(p, nside * nside)
        ix = sum(((ipf >> (2 * b)) & 1) << b for b in range(16))
        iy = sum(((ipf >> (2 * b + 1)) & 1) << b for b in range(16))
        jr = jrll[f] * nside - ix - iy - 1
        if jr < nside:
            nr, zz = jr, 1.0 - jr * jr / (3.0 * nside * nside)
        elif jr > 3 * nside:
            nr = 4 * nside - jr
            zz = nr * nr / (3.0 * nside * nside) - 1.0
        else:
            nr, zz = nside, (2 * nside - jr) * 2.0 / (3.0 * nside)
        tmp = (jpll[f] * nr + ix - iy) % (8 * nr)
        z.append(zz)
        phi.append(np.pi / 4.0 * tmp / nr)
    return np.array(z), np.array(phi)


@pytest.mark.parametrize("nside", [1, 2, 4, 8])
def test_ring_nested_reordering_against_pixel_geometry(nside):
    """nest2ring / ring2nest (integer arithmetic) against the permutation found by matching
    pixel-centre coordinates of the two orderings, each built from its own definition."""
    from cosmomap2_amd.utilities import healpix_fits as hf
    npix = 12 * nside * nside
    zr, pr = _ring_centres(nside)
    zn, pn = _nest_centres(nside)
    assert zr.size == npix and zn.size == npix
    table = np.empty(npix, dtype=np.int64)                 # hand-built: table[nest] = ring
    for p in range(npix):
        hit = np.flatnonzero((np.abs(zr - zn[p]) < 1e-12) & (np.abs(pr - pn[p]) < 1e-12))
        assert hit.size == 1, (p, hit)
        table[p] = hit[0]
    assert sorted(table) == list(range(npix))
    np.testing.assert_array_equal(hf.nest2ring(nside, np.arange(npix)), table)
    np.testing.assert_array_equal(hf.ring2nest(nside, table), np.arange(npix))
    assert hf.nest2ring(nside, 0) == int(table[0]) and isinstance(hf.nest2ring(nside, 0), int)
    m = np.random.default_rng(nside).standard_normal((2, npix))
    ring = hf.reorder(m, n2r=True)
    np.testing.assert_array_equal(ring[:, table], m)
    np.testing.assert_array_equal(hf.reorder(ring, r2n=True), m)
    if nside == 1:
        np.testing.assert_array_equal(table, np.arange(12))     # the base pixels are ring-ordered
    with pytest.raises(ValueError):
        hf.nest2ring(3, 0)
    with pytest.raises(ValueError):
        hf.nest2ring(nside, npix)
    with pytest.raises(ValueError):
        hf.reorder(m)


def test_healpix_fits_reader_on_the_reference_map():
    """The reference's input map data/cmb_r0.2_3.5arcmin_128.fits (synfast, 3 x 1024E columns)
    through read_map.  The 2.3 MB file itself is not committed; tests/golden/make_fits_fixture.py
    stores its header cards, pixel samples and sums, and reference_cmb_map_head.fits: the file's own
    bytes cut to its first 12 table rows (nside 32; only NAXIS2, NSIDE and LASTPIX rewritten).  The
    full header cards are checked against the parser, the cut file against a separate NumPy view of
    its table, against the samples that fall in it and against the sums of its rows."""
    from cosmomap2_amd.utilities import healpix_fits as hf
    G = np.load(os.path.join(GOLD, "reference_cmb_map_samples.npz"))
    cards = [bytes(row).decode("ascii") for row in G["header_cards"]]
    raw = "".join(cards).encode("ascii") + ("%-80s" % "END").encode("ascii")
    raw += b" " * (-len(raw) % 2880)
    hdr, _ = hf._parse_header(raw, 0)
    assert hdr["XTENSION"] == "BINTABLE" and hdr["NAXIS1"] == 12288 and hdr["NAXIS2"] == 192
    assert hdr["TFORM1"] == "1024E" and hdr["NSIDE"] == 128 and hdr["ORDERING"] == "RING"
    assert hdr["POLAR"] is True and abs(hdr["BAD_DATA"] + 1.6375e30) < 1e18
    rows = int(G["head_rows"])
    npix = rows * 1024
    I, Q, U, h = hf.read_map(REF_FITS, field=[0, 1, 2], h=True)
    assert I.shape == Q.shape == U.shape == (npix,) and I.dtype == np.float64
    assert h["NSIDE"] == 32 and 12 * h["NSIDE"] ** 2 == npix and h["LASTPIX"] == npix - 1
    # every header card of the cut file but the three size cards is the reference's
    assert {k: v for k, v in h.items() if k not in ("NAXIS2", "NSIDE", "LASTPIX")} == \
        {k: v for k, v in hdr.items() if k in h and k not in ("NAXIS2", "NSIDE", "LASTPIX")}
    data = open(REF_FITS, "rb").read()
    table = np.frombuffer(data, dtype=">f4", count=rows * 3 * 1024,
                          offset=int(G["header_bytes"])).reshape(rows, 3, 1024)
    for i, m in enumerate((I, Q, U)):
        np.testing.assert_array_equal(m, table[:, i, :].reshape(-1).astype(np.float64))
    pix = G["pixels"]
    sel = pix < npix
    assert sel.sum() > 200
    np.testing.assert_array_equal(I[pix[sel]], G["I"][sel])
    np.testing.assert_array_equal(Q[pix[sel]], G["Q"][sel])
    np.testing.assert_array_equal(U[pix[sel]], G["U"][sel])
    np.testing.assert_allclose([I.sum(), Q.sum(), U.sum()], G["head_sums"], rtol=1e-12)
    np.testing.assert_allclose([(I * I).sum(), (Q * Q).sum(), (U * U).sum()], G["head_sumsq"], rtol=1e-12)
    np.testing.assert_array_equal(hf.read_map(REF_FITS), I)


def test_hdf5_round_trip_fuzz(tmp_path):
    """write_file -> read_file gives back random trees: nested groups (more children than one
    symbol-table node holds), either byte order, int / float dtypes, scalars, empty and
    multi-dimensional arrays, contiguous and chunked layout."""
    hyp = pytest.importorskip("hypothesis")
    from hypothesis import given, settings, strategies as st, HealthCheck
    from cosmomap2_amd.utilities import hdf5_lite as h5

    dtypes = st.sampled_from(["<f8", ">f8", "<f4", ">i4", "<i4", ">i8", "<i2", "u1"])
    shapes = st.one_of(st.just(()), st.tuples(st.integers(0, 40)),
                       st.tuples(st.integers(1, 9), st.integers(1, 7)),
                       st.tuples(st.integers(1, 4), st.integers(1, 4), st.integers(1, 3)))

    @st.composite
    def arrays(draw):
        dt, shape = np.dtype(draw(dtypes)), draw(shapes)
        n = int(np.prod(shape)) if shape else 1
        seed = draw(st.integers(0, 2 ** 31 - 1))
        rng = np.random.default_rng(seed)
        if dt.kind == "f":
            a = rng.standard_normal(n)
        else:
            info = np.iinfo(dt)
            a = rng.integers(max(info.min, -10 ** 9), min(info.max, 10 ** 9), n, endpoint=True)
        a = a.astype(dt).reshape(shape)
        if len(shape) >= 1 and n > 0 and draw(st.booleans()):
            chunks = tuple(draw(st.integers(1, max(1, s))) for s in shape)
            return h5.Chunked(a, chunks)
        return a

    names = st.text("abcdefghijklmnopqrstuvwxyz_0123456789", min_size=1, max_size=12)
    trees = st.recursive(st.dictionaries(names, arrays(), min_size=0, max_size=5),
                         lambda children: st.dictionaries(names, st.one_of(arrays(), children),
                                                          min_size=1, max_size=6), max_leaves=25)

    def check(got, want):
        assert sorted(got) == sorted(want)
        for k, w in want.items():
            if isinstance(w, dict):
                check(got[k], w)
                continue
            a = w.array if isinstance(w, h5.Chunked) else w
            g = got[k]
            assert g.shape == a.shape and g.dtype == a.dtype.newbyteorder("="), (k, g.dtype, a.dtype)
            np.testing.assert_array_equal(g, a)

    counter = [0]

    @settings(max_examples=60, deadline=None, suppress_health_check=list(HealthCheck))
    @given(trees)
    def run(tree):
        counter[0] += 1
        p = str(tmp_path / ("fuzz%d.hdf5" % counter[0]))
        h5.write_file(p, tree)
        check(h5.read_file(p), tree)
        os.remove(p)

    run()
    # a group with more links than one symbol-table leaf (2 K_leaf = 64) holds
    big = {"d%03d" % i: np.arange(i % 5, dtype=">i4") for i in range(150)}
    p = str(tmp_path / "many.hdf5")
    h5.write_file(p, {"g": big, "x": np.float64(3.5)})
    back = h5.read_file(p)
    assert len(back["g"]) == 150 and float(back["x"]) == 3.5
    for k, v in big.items():
        np.testing.assert_array_equal(back["g"][k], v)


def test_fits_map_round_trip_fuzz(tmp_path):
    """write_map -> read_map for 1 and 3 maps, float32 / float64 columns, both orderings."""
    from cosmomap2_amd.utilities import healpix_fits as hf
    rng = np.random.default_rng(3)
    k = 0
    for nside in (1, 2, 8, 32):
        npix = 12 * nside * nside
        for nmaps in (1, 3):
            for dt in (np.float32, np.float64):
                for nest in (False, True):
                    maps = [rng.standard_normal(npix).astype(dt) for _ in range(nmaps)]
                    p = str(tmp_path / ("m%d.fits" % k)); k += 1
                    hf.write_map(p, maps if nmaps > 1 else maps[0], nest=nest, dtype=dt)
                    got = hf.read_map(p, field=None, dtype=np.float64, nest=nest, h=True)
                    hdr = got[-1]
                    assert hdr["NSIDE"] == nside and hdr["ORDERING"] == ("NESTED" if nest else "RING")
                    assert hdr["TFIELDS"] == nmaps and len(got) == nmaps + 1
                    for a, b in zip(got[:-1], maps):
                        np.testing.assert_array_equal(a, b.astype(np.float64))
                    # asked for the other ordering, the reader converts (hp.read_map does)
                    other = hf.read_map(p, nest=not nest)
                    np.testing.assert_array_equal(
                        other, hf.reorder(maps[0].astype(np.float64), n2r=nest, r2n=not nest))


def test_corrupt_files_raise_the_format_errors(tmp_path):
    """Truncated files and files with random bytes changed either still parse or raise
    Hdf5FormatError / FitsFormatError -- no other exception, no hang, no huge allocation."""
    from cosmomap2_amd.utilities import hdf5_lite as h5, healpix_fits as hf
    rng = np.random.default_rng(0)
    p = str(tmp_path / "c.hdf5")
    h5.write_file(p, {"g": {"a": np.arange(100.), "h": {"z": np.arange(5)},
                            "b": h5.Chunked(np.arange(64, dtype=">i4").reshape(8, 8), (4, 4))},
                      "x": np.float64(2.0)})
    good = open(p, "rb").read()
    outcomes = set()
    for i in range(600):
        d = bytearray(good)
        if i % 2 == 0:
            d = d[:int(rng.integers(0, len(d)))]
        else:
            for _ in range(int(rng.integers(1, 6))):
                d[int(rng.integers(0, len(d)))] = int(rng.integers(0, 256))
        open(p, "wb").write(bytes(d))
        try:
            h5.read_file(p)
            outcomes.add("ok")
        except h5.Hdf5FormatError:
            outcomes.add("format error")
    assert outcomes == {"ok", "format error"}
    q = str(tmp_path / "c.fits")
    hf.write_map(q, [np.arange(12 * 4 * 4, dtype=float)] * 3)
    good = open(q, "rb").read()
    outcomes = set()
    for i in range(400):
        d = bytearray(good)
        if i % 2 == 0:
            d = d[:int(rng.integers(0, len(d)))]
        else:
            for _ in range(int(rng.integers(1, 6))):
                d[int(rng.integers(0, min(len(d), 6000)))] = int(rng.integers(0, 256))
        open(q, "wb").write(bytes(d))
        try:
            hf.read_map(q, field=None)
            outcomes.add("ok")
        except (hf.FitsFormatError, NotImplementedError):     # (a flipped ORDERING keyword)
            outcomes.add("format error")
    assert outcomes == {"ok", "format error"}


def test_chunked_dataset_with_more_than_64_chunks(tmp_path):
    """A Ritz checkpoint whose chunk grid exceeds one B-tree leaf (64 chunks) is written with
    coarser chunks instead of failing, and reads back bit for bit."""
    from cosmomap2_amd.utilities import hdf5_lite as h5
    a = np.arange(40 * 30, dtype=np.float64).reshape(40, 30)
    p = str(tmp_path / "many.hdf5")
    h5.write_file(p, {"Z": h5.Chunked(a, (2, 3))})            # 20 x 10 = 200 chunks asked for
    np.testing.assert_array_equal(np.asarray(h5.read_file(p)["Z"]), a)
