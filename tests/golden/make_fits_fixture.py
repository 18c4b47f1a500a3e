"""
Fixtures from the HEALPix map the reference holds for its runs: its data/cmb_r0.2_3.5arcmin_128.fits
(synfast output, 3 x 196608 float32 pixels in a binary table of 1024-pixel rows; read by hp.read_map at
src/test_BD_precond_onto_real_data.py:31-37).  The file is 2.3 MB, so instead of a copy this script
stores what pins a reader:

* reference_cmb_map_samples.npz: the two headers' keyword cards as written, and the pixel values of
  every column at 4096 seeded pixel numbers plus per-column sums (whole map, and its first HEAD_ROWS
  rows), all taken with a few lines of NumPy that know this one file's layout (two header units of
  2880 and 8640 bytes, then 192 rows of 3 x 1024 big-endian float32);
* reference_cmb_map_head.fits: the file's own bytes cut to its first HEAD_ROWS table rows, a complete
  HEALPix file of nside 32 (12 rows of 1024 pixels).  Only the three cards that state the size are
  rewritten in place (NAXIS2, NSIDE, LASTPIX: same 80-byte slots, comments kept); every other header
  byte is the reference's, and the table is zero-padded to the 2880-byte block as FITS requires.

Build container only (the reference tree is not part of this repository):

    python tests/golden/make_fits_fixture.py <reference tree>/data/cmb_r0.2_3.5arcmin_128.fits
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD_ROWS = 12                                   # 12 x 1024 = 12 * 32**2 pixels: nside 32


def _set_card(header, key, value):
    """Rewrite the value of the card `key` in place (right-justified in columns 11-30, comment kept)."""
    for i in range(0, len(header), 80):
        if header[i:i + 8] == ("%-8s" % key).encode("ascii"):
            header[i + 10:i + 30] = ("%20d" % value).encode("ascii")
            return
    raise KeyError(key)


def main(src):
    d = open(src, "rb").read()
    # header units end with a card that starts with 'END' in an 80-byte slot
    ends = [i for i in range(0, 5 * 2880, 80) if d[i:i + 8] == b"END     "]
    h1_end = (ends[0] // 2880 + 1) * 2880
    h2_end = (ends[1] // 2880 + 1) * 2880
    table = np.frombuffer(d, dtype=">f4", count=192 * 3 * 1024, offset=h2_end).reshape(192, 3, 1024)
    cols = [table[:, i, :].reshape(-1).astype(np.float64) for i in range(3)]
    head = [c[:HEAD_ROWS * 1024] for c in cols]
    rng = np.random.default_rng(20161202)
    idx = np.sort(rng.choice(196608, 4096, replace=False))
    cards = [d[i:i + 80].decode("ascii") for i in range(0, h2_end, 80)]
    keyed = [c for c in cards if c[8:10] == "= "]
    np.savez(os.path.join(HERE, "reference_cmb_map_samples.npz"),
             pixels=idx, I=cols[0][idx], Q=cols[1][idx], U=cols[2][idx],
             sums=np.array([c.sum() for c in cols]), sumsq=np.array([(c * c).sum() for c in cols]),
             header_cards=np.frombuffer("".join(keyed).encode("ascii"), dtype=np.uint8).reshape(-1, 80), header_bytes=np.int64(h2_end),
             primary_bytes=np.int64(h1_end), head_rows=np.int64(HEAD_ROWS),
             head_sums=np.array([c.sum() for c in head]), head_sumsq=np.array([(c * c).sum() for c in head]))
    header = bytearray(d[:h2_end])
    nside = int(round((HEAD_ROWS * 1024 / 12) ** 0.5))
    _set_card(header, "NAXIS2", HEAD_ROWS)
    _set_card(header, "NSIDE", nside)
    _set_card(header, "LASTPIX", 12 * nside * nside - 1)
    rows = d[h2_end:h2_end + HEAD_ROWS * 12288]
    with open(os.path.join(HERE, "reference_cmb_map_head.fits"), "wb") as fh:
        fh.write(bytes(header) + rows + b"\0" * (-len(rows) % 2880))
    print("header units:", h1_end, h2_end - h1_end, "cards:", len(keyed), "head file: %d rows, nside %d"
          % (HEAD_ROWS, nside))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
