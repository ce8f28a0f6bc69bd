"""Test helper: gnark-crypto's two point encodings on BN254 with Python integers, and key files rewritten between them.

  compressed   32 B (G1: X) / 64 B (G2: X.A1 | X.A0), flag bits 10 / 11 (smaller / larger Y) or 01 (infinity) on top of byte 0
  raw          64 B (G1: X | Y) / 128 B (G2: X.A1 | X.A0 | Y.A1 | Y.A0), flag bits 00; all-zero bytes are the point at infinity

rewrite_pk / rewrite_vk turn chosen points of a compressed key (the layout tests/test_gpu_degenerate.py::_edit_pk walks; csrc/formats.cpp
parse_pk, csrc/verify_common.cpp parse_vk_layout) into their raw form; decode_g1 / decode_g2 are the reference decoders of the GPU tests
(G2 with the subgroup test [r]Q = O).  Nothing here calls the library."""
import functools

P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
HALF = (P - 1) // 2
_INV82 = pow(82, -1, P)
TWIST_B = (27 * _INV82 % P, -3 * _INV82 % P)                      # 3 / (9 + u)
G2_GEN = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
          (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


# ---- Fp, Fp2 = Fp[u] / (u^2 + 1); an Fp2 value is (a0, a1) ----
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def sqrt_fp(a):
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def sqrt_fp2(a):      # norm method, p = 3 mod 4
    if a[1] == 0:
        s = sqrt_fp(a[0])
        if s is not None:
            return (s, 0)
        s = sqrt_fp(-a[0] % P)
        return None if s is None else (0, s)
    n = sqrt_fp((a[0] * a[0] + a[1] * a[1]) % P)
    if n is None:
        return None
    for t in ((a[0] + n) * pow(2, -1, P) % P, (a[0] - n) * pow(2, -1, P) % P):
        x0 = sqrt_fp(t)
        if x0:
            x = (x0, a[1] * pow(2 * x0, -1, P) % P)
            if f2mul(x, x) == (a[0] % P, a[1] % P):
                return x
    return None


def g1_rhs(x):
    return (x * x * x + 3) % P


def g2_rhs(x):
    return f2add(f2mul(f2mul(x, x), x), TWIST_B)


def large1(y):
    return y > HALF


def large2(y):      # gnark-crypto's lexicographic order on Fp2: the imaginary part decides unless it is zero
    return y[1] > HALF if y[1] else y[0] > HALF


# ---- the group law on E'(Fp2), affine with None = infinity (the reference of the subgroup test; a few hundred operations per point) ----
def g2_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == (0, 0):
            return None
        lam = f2mul(f2mul((3, 0), f2mul(p[0], p[0])), f2inv(f2add(p[1], p[1])))
    else:
        lam = f2mul(f2sub(q[1], p[1]), f2inv(f2sub(q[0], p[0])))
    x3 = f2sub(f2sub(f2mul(lam, lam), p[0]), q[0])
    return (x3, f2sub(f2mul(lam, f2sub(p[0], x3)), p[1]))


def g2_mul(p, k):
    acc = None
    for bit in bin(k)[2:]:
        acc = g2_add(acc, acc)
        if bit == "1":
            acc = g2_add(acc, p)
    return acc


@functools.lru_cache(maxsize=None)
def g2_in_subgroup(p):
    return g2_mul(p, R) is None


def g1_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x3 = (lam * lam - p[0] - q[0]) % P
    return (x3, (lam * (p[0] - x3) - p[1]) % P)


def g1_mul(p, k):
    acc = None
    for bit in bin(k)[2:]:
        acc = g1_add(acc, acc)
        if bit == "1":
            acc = g1_add(acc, p)
    return acc


@functools.lru_cache(maxsize=None)
def twist_point_outside_g2():
    """(x, y) on E'(Fp2) but NOT in the r-torsion subgroup (a random twist point is in G2 with probability ~2^-254); the same point as
    tests/test_verifier.py::_twist_point_outside_g2: the first x = (k, 1), k = 1, 2, ..., with a point above it."""
    k = 1
    while True:
        x = (k, 1)
        y = sqrt_fp2(g2_rhs(x))
        if y is not None:
            return x, y
        k += 1


# ---- encoders (points as integers; None = infinity) ----
def be(v):
    return int(v).to_bytes(32, "big")


def enc_g1(p, raw):
    if p is None:
        return bytes(64) if raw else bytes([0x40]) + bytes(31)
    if raw:
        return be(p[0]) + be(p[1])
    b = bytearray(be(p[0])); b[0] |= 0xC0 if large1(p[1]) else 0x80
    return bytes(b)


def enc_g2(p, raw):
    if p is None:
        return bytes(128) if raw else bytes([0x40]) + bytes(63)
    x, y = p
    if raw:
        return be(x[1]) + be(x[0]) + be(y[1]) + be(y[0])
    b = bytearray(be(x[1]) + be(x[0])); b[0] |= 0xC0 if large2(y) else 0x80
    return bytes(b)


# ---- reference decoders: (status, point) with status 0 a point of the group, 1 refused, 2 infinity — what the library must answer ----
def element_size(group, first_byte):
    cb = 32 if group == 0 else 64
    return 2 * cb if first_byte & 0xC0 == 0 else cb


def decode_g1(e):
    flag = e[0] & 0xC0
    if flag == 0:
        assert len(e) == 64
        if e == bytes(64):
            return 2, None
        x, y = int.from_bytes(e[:32], "big"), int.from_bytes(e[32:], "big")
        if x >= P or y >= P or y * y % P != g1_rhs(x):
            return 1, None
        return 0, (x, y)
    assert len(e) == 32
    x = int.from_bytes(e, "big") & ((1 << 254) - 1)
    if flag == 0x40:
        return (2, None) if x == 0 else (1, None)
    if x >= P:
        return 1, None
    y = sqrt_fp(g1_rhs(x))
    if y is None:
        return 1, None
    if large1(y) != (flag == 0xC0):
        y = -y % P
    return 0, (x, y)


def decode_g2(e):
    flag = e[0] & 0xC0
    if flag == 0:
        assert len(e) == 128
        if e == bytes(128):
            return 2, None
        x1, x0, y1, y0 = (int.from_bytes(e[32 * i:32 * i + 32], "big") for i in range(4))
        if max(x0, x1, y0, y1) >= P or f2mul((y0, y1), (y0, y1)) != g2_rhs((x0, x1)):
            return 1, None
        p = ((x0, x1), (y0, y1))
    else:
        assert len(e) == 64
        x1, x0 = int.from_bytes(e[:32], "big") & ((1 << 254) - 1), int.from_bytes(e[32:], "big")
        if flag == 0x40:
            return (2, None) if x0 == 0 and x1 == 0 else (1, None)
        if x0 >= P or x1 >= P:
            return 1, None
        y = sqrt_fp2(g2_rhs((x0, x1)))
        if y is None:
            return 1, None
        if large2(y) != (flag == 0xC0):
            y = ((-y[0]) % P, (-y[1]) % P)
        p = ((x0, x1), y)
    return (0, p) if g2_in_subgroup(p) else (1, None)


def to_raw(group, comp):
    """one compressed element of a key -> the raw element of the same point (no subgroup test: the caller may want a bad point in raw form)"""
    if group == 0:
        st, p = decode_g1(comp)
        assert st != 1, "not a G1 point"
        return enc_g1(p, True)
    flag = comp[0] & 0xC0
    if flag == 0x40:
        return bytes(128)
    x = (int.from_bytes(comp[32:], "big"), int.from_bytes(comp[:32], "big") & ((1 << 254) - 1))
    y = sqrt_fp2(g2_rhs(x))
    assert y is not None, "not a twist point"
    if large2(y) != (flag == 0xC0):
        y = ((-y[0]) % P, (-y[1]) % P)
    return enc_g2((x, y), True)


# ---- key files ----
PK_HEADER = 8 + 5 * 32 + 1                                        # domain size, five Fr constants, the precompute flag


def _walk(b, o, group, count):
    """offsets of `count` elements (either encoding) starting at o -> ([(offset, size)], end)"""
    out = []
    for _ in range(count):
        sz = element_size(group, b[o])
        out.append((o, sz)); o += sz
    return out, o


def pk_sections(pk):
    """[(name, group, has_count_prefix, [(offset, size)])] of every point set of a proving key, then the offset where the points end and the
    offset of the tail between G2.B and the commitment keys"""
    o = PK_HEADER
    secs = []

    def single(name, group):
        nonlocal o
        el, o = _walk(pk, o, group, 1); secs.append((name, group, False, el))

    def sl(name, group):
        nonlocal o
        n = int.from_bytes(pk[o:o + 4], "big"); o += 4
        el, o = _walk(pk, o, group, n); secs.append((name, group, True, el))
    for nm in ("g1.alpha", "g1.beta", "g1.delta"):
        single(nm, 0)
    for nm in ("g1.A", "g1.B", "g1.Z", "g1.K"):
        sl(nm, 0)
    single("g2.beta", 1); single("g2.delta", 1); sl("g2.B", 1)
    nw = int.from_bytes(pk[o:o + 8], "big")
    o += 24 + 2 * nw
    nck = int.from_bytes(pk[o:o + 4], "big"); o += 4
    for k in range(nck):
        sl("ped.basis", 0); sl("ped.sigma", 0)
    assert o == len(pk), "trailing bytes"
    return secs


def _rewrite(key, secs, choose, replace):
    out = bytearray(); at = 0
    for name, group, _, elems in secs:
        for i, (o, sz) in enumerate(elems):
            out += key[at:o]; at = o + sz
            e = key[o:o + sz]
            if replace and (name, i) in replace:
                e = replace[(name, i)]
            elif choose(name, i) and e[0] & 0xC0:
                e = to_raw(group, e)
            out += e
    return bytes(out + key[at:])


def rewrite_pk(pk, choose=lambda name, i: False, replace=None):
    """pk with element i of set `name` made raw where choose(name, i), or replaced by the encoded element replace[(name, i)]"""
    return _rewrite(pk, pk_sections(pk), choose, replace)


def vk_sections(vk):
    o = 0
    secs = []

    def single(name, group):
        nonlocal o
        el, o = _walk(vk, o, group, 1); secs.append((name, group, False, el))
    single("g1.alpha", 0); single("g1.beta", 0); single("g2.beta", 1); single("g2.gamma", 1); single("g1.delta", 0); single("g2.delta", 1)
    n = int.from_bytes(vk[o:o + 4], "big"); o += 4
    el, o = _walk(vk, o, 0, n); secs.append(("g1.K", 0, True, el))
    outer = int.from_bytes(vk[o:o + 4], "big"); o += 4 + 4 * outer
    nck = int.from_bytes(vk[o:o + 4], "big"); o += 4
    for k in range(nck):
        single("ped.g", 1); single("ped.gsn", 1)
    assert o == len(vk), "trailing bytes"
    return secs


def rewrite_vk(vk, choose=lambda name, i: False, replace=None):
    return _rewrite(vk, vk_sections(vk), choose, replace)


def raw_vk(vk):
    """the verifying key of the raw-key tests: alpha, beta2, gamma2, delta2 and every second K point raw"""
    return rewrite_vk(vk, lambda name, i: name in ("g1.alpha", "g2.beta", "g2.gamma", "g2.delta") or (name == "g1.K" and i % 2 == 0))


def mixed_pk(pk):
    """the proving key of the raw-key tests: alpha, beta, delta, every third of the first 2 000 points of each G1 slice and the first 500 of G2.B raw"""
    def choose(name, i):
        if name in ("g1.alpha", "g1.beta", "g1.delta", "g2.beta", "g2.delta"):
            return True
        if name == "g2.B":
            return i < 500
        return i < 2000 and i % 3 == 0
    return rewrite_pk(pk, choose)
