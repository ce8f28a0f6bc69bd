"""k_wipe and k_scan_idle (csrc/k_wipe.hip) through the test hook gsc_debug_wipe, against a numpy model: byte-exact heads and tails at every
alignment, rows of a pitch, lists of descriptors of mixed sizes in one launch, the plane image by row class, offsets past 2^32 — and every
byte outside a descriptor untouched.  The kernels clear (and check) every key-derived buffer of the prover (csrc/wipe_plan.hpp)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
FILL = 0xA5


def _model(nbytes, descs, cls=b""):
    buf = np.full(nbytes, FILL, dtype=np.uint8)
    for d in descs:
        off, rows, pitch, width = d[:4]
        image = len(d) > 4 and d[4]
        for r in range(rows):
            buf[off + r * pitch: off + r * pitch + width] = 0x80 if image and cls[r % len(cls)] else 0
    return buf


def _check(gsc, descs, cls=b"", nbytes=MIB):
    got, _, _ = gsc.debug_wipe(nbytes, FILL, descs, cls)
    got = np.frombuffer(got, dtype=np.uint8)
    want = _model(nbytes, descs, cls)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing byte %d of %d: got %#x, want %#x (descs %r)" % (bad[0], bad.size, got[bad[0]], want[bad[0]], descs[:4])


OFFSETS = (0, 1, 3, 15, 16, 17)
WIDTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4095)


def test_every_alignment_of_head_and_tail_one_descriptor_each(gsc):
    # rows = 1, pitch = width: one launch per (offset, width), neighbours on both sides compared with the model
    for off in OFFSETS:
        for w in WIDTHS:
            _check(gsc, [(4096 + off, 1, w, w)], nbytes=3 * 4096 + 64)


def test_all_alignments_in_one_launch_list(gsc):
    # the same 54 descriptors, twice, side by side in ONE list: more than the 64 a launch carries, so the launcher cuts it
    pairs = [(o, w) for o in OFFSETS for w in WIDTHS] * 2
    descs = [(k * 8192 + 4096 + off, 1, w, w) for k, (off, w) in enumerate(pairs)]
    _check(gsc, descs)


@pytest.mark.parametrize("n", [1, 5, 63])
def test_columns_of_each_2k_row(gsc, n):
    # what a latency-path call clears: columns < n (32 bytes each) of every row of 64 columns; 333 rows (several units of short rows, a ragged last one)
    _check(gsc, [(2048 * 3, 333, 2048, 32 * n)])
    _check(gsc, [(2048 * 3 + 16, 333, 2048, 32 * n)])      # rows that start on a 16-byte boundary only
    _check(gsc, [(7, 500, 2048, 32 * n + 1)])              # ... and on none


def test_adjacent_descriptors_and_rows_that_touch(gsc):
    _check(gsc, [(100, 1, 901, 901), (1001, 1, 4099, 4099), (5100, 1, 12, 12)])      # each starts where the last one ended
    _check(gsc, [(64, 200, 48, 48)])                                                # pitch == width: the rows are one long row
    _check(gsc, [(64, 200, 49, 48)])                                                # one byte between the rows survives


def test_forty_descriptors_of_mixed_size_in_one_launch(gsc):
    rnd = np.random.default_rng(40)
    descs, at = [], 0
    for k in range(40):
        kind = k % 4
        if kind == 0:
            rows, width = 1, int(rnd.integers(1, 60000))
            pitch = width
        elif kind == 1:
            rows, width = int(rnd.integers(2, 40)), int(rnd.integers(1, 300))
            pitch = width + int(rnd.integers(0, 100))
        elif kind == 2:
            rows, width, pitch = int(rnd.integers(2, 9)), int(rnd.integers(2049, 9000)), 9100
        else:
            rows, width, pitch = 1, int(rnd.integers(0, 3)), 7
        at += int(rnd.integers(0, 40))
        descs.append((at, rows, pitch, width))
        at += (rows - 1) * pitch + width
    assert at < MIB
    _check(gsc, descs)


def test_plane_image_by_row_class(gsc):
    # a byte plane of 3 groups x 41 rows of 64 bytes; rows 0, 7 and the last one of every group are marked wide: they get 0x80, the others 0
    rows = 41
    cls = bytearray(rows)
    cls[0] = cls[7] = cls[rows - 1] = 1
    _check(gsc, [(4096, 3 * rows, 64, 64, 1)], bytes(cls))
    _check(gsc, [(4096 + 5, 3 * rows, 64, 64, 1), (65536, 2 * rows, 64, 64, 0)], bytes(cls))      # off every boundary; a zero descriptor in the same list
    # a long row of an image (one class for the whole row)
    _check(gsc, [(1000, 2, 10000, 9001, 1)], b"\x01\x00")


def test_scan_counts_known_buffers(gsc):
    n = 300000
    # all off the zero image / all idle after a wipe of the window
    _, c, _ = gsc.debug_wipe(MIB, FILL, [], windows=[(0, 1, MIB, MIB), (5, 1, n, n), (3, 77, 2048, 33)], want_buffer=False)
    assert c == [MIB, n, 77 * 33]
    _, c, _ = gsc.debug_wipe(MIB, FILL, [(5, 1, n, n)], windows=[(5, 1, n, n), (4, 1, n + 2, n + 2), (0, 1, MIB, MIB)], want_buffer=False)
    assert c == [0, 2, MIB - n]      # one byte off at each end of the wider window
    _, c, _ = gsc.debug_wipe(MIB, 0, [], windows=[(0, 1, MIB, MIB)], want_buffer=False)
    assert c == [0]


def test_scan_reads_marked_rows_by_their_image(gsc):
    rows = 41
    cls = bytearray(rows)
    cls[0] = cls[7] = cls[rows - 1] = 1
    plane = (4096, 2 * rows, 64, 64, 1)
    # the image written: clean as an image, and the six marked rows are off as a zero region
    _, c, _ = gsc.debug_wipe(MIB, FILL, [plane], bytes(cls), windows=[plane, plane[:4]], want_buffer=False)
    assert c == [0, 6 * 64]
    # the plane zeroed instead: the marked rows read as off
    _, c, _ = gsc.debug_wipe(MIB, FILL, [plane[:4]], bytes(cls), windows=[plane, plane[:4]], want_buffer=False)
    assert c == [6 * 64, 0]
    # one marked row holding 0x80 is clean, the same row holding 0 is off
    row7 = (4096 + 7 * 64, 1, 64, 64, 1)
    _, c, _ = gsc.debug_wipe(MIB, 0x80, [], b"\x01", windows=[row7], want_buffer=False)
    assert c == [0]
    _, c, _ = gsc.debug_wipe(MIB, 0, [], b"\x01", windows=[row7], want_buffer=False)
    assert c == [64]


def test_offsets_past_four_gib(gsc):
    # a 4 GiB + 4 KiB buffer; one descriptor across 2^32, one whose rows x pitch passes it; 256-byte scan windows on either side of each edge
    G4 = 1 << 32
    nbytes = G4 + 4096
    lo, hi = G4 - 64, G4 + 64
    pitch = 1 << 22
    rows = 1025                       # row 1024 starts at 2^32 + 2048
    descs = [(lo, 1, 128, 128), (2048, rows, pitch, 1000)]
    last = 2048 + (rows - 1) * pitch
    assert last > G4 and last + 1000 <= nbytes
    wins = [(lo - 256, 1, 256, 256), (lo, 1, 128, 128), (hi, 1, 256, 256),            # before, inside, after the first
            (last - 256, 1, 256, 256), (last, 1, 1000, 1000), (last + 1000, 1, 256, 256),  # ... the last row of the second
            (2048 + 1023 * pitch, 1, 1256, 1256),                                       # the row before it, and what follows
            (0, 1, 2048, 2048), (2048, 1, 1000, 1000)]                                 # the first row
    _, c, ms = gsc.debug_wipe(nbytes, FILL, descs, windows=wins, want_buffer=False)
    assert c == [256, 0, 256, 256, 0, 256, 256, 2048, 0], c
    # a truncated offset would land in the low 4 KiB: with the first descriptor alone nothing but its 128 bytes changes anywhere
    _, c, _ = gsc.debug_wipe(nbytes, FILL, [(lo, 1, 128, 128)], windows=[(0, 1, 4096, 4096), (0, 1, nbytes, nbytes)], want_buffer=False)
    assert c == [4096, nbytes - 128]


def test_hook_refuses_descriptors_outside_the_buffer(gsc):
    for bad in [(MIB - 10, 1, 11, 11), (0, 3, MIB // 2, MIB // 2 + 1), (0, 2, 5, 6), (1 << 63, 1, 1, 1), (0, 1 << 62, 1 << 62, 1)]:
        with pytest.raises(RuntimeError):
            gsc.debug_wipe(MIB, FILL, [bad], want_buffer=False)
    with pytest.raises(RuntimeError):
        gsc.debug_wipe(MIB, FILL, [(0, 4, 64, 64, 1)], want_buffer=False)      # an image without row classes
