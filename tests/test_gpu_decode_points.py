"""GPU tests of the key-point decode of InitAlgorithm through gsc_debug_decode_points (include/libprove.h): the host walk over a slice of
compressed and raw elements and the decode kernels of csrc/k_init.hip — k_decompress_g1/g2 for the compressed elements, k_decode_raw_g1/g2
for the raw ones, k_g2_subgroup over every finite G2 point — against big-integer decoding (tests/keyraw.py).  Slices of 1, 63, 64, 65 and
130 elements put every case at the edges of a wave; the four layouts are all compressed, all raw, alternating, and raw at the last index only."""
import pytest

import keyraw as K

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 130]
LAYOUTS = ["compressed", "raw", "alternating", "raw_last"]


def _flag(b, flag):
    b = bytearray(b); b[0] = (b[0] & 0x3F) | flag
    return bytes(b)


def _g1_cases():
    """[(compressed element or None, raw element or None)]: one case per line of the issue's list"""
    g = (1, 2)
    pts = [K.g1_mul(g, k) for k in (1, 2, 3, 7)]
    neg = lambda p: (p[0], -p[1] % K.P)
    cases = [(K.enc_g1(p, False), K.enc_g1(p, True)) for p in pts]
    cases += [(K.enc_g1(neg(p), False), K.enc_g1(neg(p), True)) for p in pts[:2]]                   # a point and its negative
    x, y = pts[0]
    assert x + K.P < 1 << 254
    cases.append((_flag(K.be(x + K.P), 0x80), K.be(x + K.P) + K.be(y)))                            # x >= p
    cases.append((None, K.be(x) + K.be(y + K.P)))                                                  # y >= p
    assert all(r[0] & 0xC0 == 0 and K.decode_g1(r)[0] == 1 for _, r in cases[-2:])
    cases.append((None, K.be(pts[1][0]) + K.be((pts[1][1] + 1) % K.P)))                            # y off by one
    cases.append((None, K.be(pts[2][0]) + K.be((pts[2][1] - 1) % K.P)))
    nox = next(v for v in range(2, 100) if K.sqrt_fp(K.g1_rhs(v)) is None)
    cases.append((_flag(K.be(nox), 0xC0), K.be(nox) + K.be(5)))                                    # x with no point above it
    cases.append((K.enc_g1(None, False), K.enc_g1(None, True)))                                    # infinity: flag 01 / all-zero raw
    stray = bytearray(K.enc_g1(None, False)); stray[31] = 1
    cases.append((bytes(stray), None))                                                             # flag 01 with a stray bit
    cases.append((None, bytes(63) + b"\x01"))                                                      # almost the raw infinity: (0, 1)
    return cases


def _g2_cases():
    pts = [K.g2_mul(K.G2_GEN, k) for k in (1, 2, 3, 5)]                                            # small multiples of the generator
    neg = lambda p: (p[0], ((-p[1][0]) % K.P, (-p[1][1]) % K.P))
    cases = [(K.enc_g2(p, False), K.enc_g2(p, True)) for p in pts]
    cases += [(K.enc_g2(neg(p), False), K.enc_g2(neg(p), True)) for p in pts[:2]]
    out = K.twist_point_outside_g2()
    cases.append((K.enc_g2(out, False), K.enc_g2(out, True)))                                      # on the twist, outside the subgroup
    cases.append((K.enc_g2(neg(out), False), K.enc_g2(neg(out), True)))
    (x0, x1), (y0, y1) = pts[0]
    # a coordinate >= p: the same residue plus p.  The second halves (a0) have 256 bits to hold it; x.a1 opens the element, so it must stay
    # below 2^254 for the flag bits to be its own: the first small multiple of the generator whose x.a1 < 2^254 - p
    small = next(q for q in (K.g2_mul(K.G2_GEN, k) for k in range(1, 60)) if q[0][1] + K.P < 1 << 254)
    (s0, s1), (t0, t1) = small
    assert K.decode_g2(K.enc_g2(small, True))[0] == 0 and s1 + K.P < 1 << 254 and max(x0, y0, y1) + K.P < 1 << 256
    cases.append((_flag(K.be(s1 + K.P) + K.be(s0), 0xC0 if K.large2((t0, t1)) else 0x80), K.be(s1 + K.P) + K.be(s0) + K.be(t1) + K.be(t0)))      # x.a1 >= p, both forms
    cases.append((_flag(K.be(x1) + K.be(x0 + K.P), 0xC0 if K.large2((y0, y1)) else 0x80), K.be(x1) + K.be(x0 + K.P) + K.be(y1) + K.be(y0)))      # x.a0 >= p, both forms
    cases.append((None, K.be(x1) + K.be(x0) + K.be(y1) + K.be(y0 + K.P)))                          # y.a0 >= p
    cases.append((None, K.be(x1) + K.be(x0) + K.be(y1 + K.P) + K.be(y0)))                          # y.a1 >= p
    for c, r in cases[-4:]:      # each of them is refused for the coordinate alone: the residues are a point of the group
        assert r[0] & 0xC0 == 0 and K.decode_g2(r)[0] == 1 and (c is None or K.decode_g2(c)[0] == 1)
    (u0, u1), (v0, v1) = pts[1]
    cases.append((None, K.be(u1) + K.be(u0) + K.be(v1) + K.be((v0 + 1) % K.P)))                    # y off by one, either component
    cases.append((None, K.be(u1) + K.be(u0) + K.be((v1 + 1) % K.P) + K.be(v0)))
    nox = next(v for v in range(1, 100) if K.sqrt_fp2(K.g2_rhs((v, 2))) is None)
    cases.append((_flag(K.be(2) + K.be(nox), 0xC0), K.be(2) + K.be(nox) + K.be(0) + K.be(5)))      # x with no point above it
    cases.append((K.enc_g2(None, False), K.enc_g2(None, True)))                                    # infinity
    for pos in (31, 63):
        stray = bytearray(K.enc_g2(None, False)); stray[pos] = 1
        cases.append((bytes(stray), None))                                                         # flag 01 with a stray bit in either half
    cases.append((None, bytes(127) + b"\x01"))
    return cases


@pytest.fixture(scope="module")
def cases():
    """per group: the cases with the expected (status, point) of each form, decoded once with Python integers"""
    out = []
    for group, cs, dec in ((0, _g1_cases(), K.decode_g1), (1, _g2_cases(), K.decode_g2)):
        out.append([(c, None if c is None else dec(c), r, None if r is None else dec(r)) for c, r in cs])
    # the list must hold what it claims: accepted points, refusals and infinities in both forms
    for group in (0, 1):
        for form in (1, 3):
            assert {e[form][0] for e in out[group] if e[form] is not None} == {0, 1, 2}
    st = {(e[1][0], e[3][0]) for e in out[1][6:8]}
    assert out[1][6][0] == K.enc_g2(K.twist_point_outside_g2(), False) and st == {(1, 1)}      # the twist point outside the subgroup: status 1 in both encodings
    return out


def _slice(group_cases, n, layout):
    """n elements in the forms the layout asks for: element i is case i + 3 (mod the count) of the cases that have that form"""
    comp = [(e[0], e[1]) for e in group_cases if e[0] is not None]
    raws = [(e[2], e[3]) for e in group_cases if e[2] is not None]
    els, want = [], []
    for i in range(n):
        raw = layout == "raw" or (layout == "alternating" and i % 2 == 1) or (layout == "raw_last" and i == n - 1)
        pool = raws if raw else comp
        e, dec = raws[1] if layout == "raw_last" and i == n - 1 else pool[(i + 3) % len(pool)]      # raw_last: a good point at the very end
        els.append(e); want.append(dec)
    return els, want


def _expected_bytes(group, dec):
    st, p = dec
    if st != 0:
        return bytes(64 if group == 0 else 128)
    return K.enc_g1(p, True) if group == 0 else K.enc_g2(p, True)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("group", [0, 1])
def test_decode_matches_big_integers(gsc, cases, group, n):
    w = 64 if group == 0 else 128
    for layout in LAYOUTS:
        els, want = _slice(cases[group], n, layout)
        if layout == "raw_last":
            assert els[-1][0] & 0xC0 == 0 and want[-1][0] == 0
        out, st = gsc.debug_decode_points(group, b"".join(els), n)
        assert list(st) == [d[0] for d in want], (layout, [i for i in range(n) if st[i] != want[i][0]])
        for i in range(n):
            assert out[w * i:w * i + w] == _expected_bytes(group, want[i]), (layout, i)


def test_every_case_sits_at_a_wave_edge(gsc, cases):
    """each case, in each of its forms, at indices 0, 63, 64 and 129 of an otherwise good slice of 130"""
    for group in (0, 1):
        w = 64 if group == 0 else 128
        good, gdec = cases[group][0][0], cases[group][0][1]
        for c, cdec, r, rdec in cases[group]:
            for e, dec in ((c, cdec), (r, rdec)):
                if e is None:
                    continue
                els, want = [good] * 130, [gdec] * 130
                for at in (0, 63, 64, 129):
                    els[at], want[at] = e, dec
                out, st = gsc.debug_decode_points(group, b"".join(els), 130)
                assert list(st) == [d[0] for d in want], (group, e.hex())
                assert out == b"".join(_expected_bytes(group, d) for d in want), (group, e.hex())


def test_malformed_slices_are_refused(gsc, cases):
    c, _, r, _ = cases[0][0]
    assert gsc.debug_decode_points(0, b"", 0) == (b"", b"")
    for enc, n in ((c + r[:40], 2), (c + r, 3), (c + r + b"\x00", 2), (r[:63], 1), (c, 1 << 21)):
        with pytest.raises(RuntimeError):
            gsc.debug_decode_points(0, enc, n)
    with pytest.raises(RuntimeError):
        gsc.debug_decode_points(2, c, 1)
