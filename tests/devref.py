"""References and case tables for the per-operation tests of the device's field and curve code (gsc_debug_limb_ops,
gsc_debug_curve_ops; include/libprove.h).  Everything here is Python integers; nothing calls the oracle or the library.

Radix-2^29 products are predicted LIMB FOR LIMB: for the integers A, B (C, D) the raw limbs denote, N = A*B, A^2 or A*B - C*D,
m = -N / p mod 2^261 and V = (N + m p) / 2^261 exactly; the result's limbs 0..7 are V's 29-bit digits and limb 8 is the signed rest
V >> 232.  norm / freeze / freeze_near keep the value (mod p for the freezes) and return its tight digits.

The generators produce exactly the operand classes bn254_fp29.hpp documents, and assert it for every case:
  T1   tight        limbs 0..7 in [0, 2^29), |limb 8| < 2^29
  T1s  signed-tight |limb| < 2^29
  T2   loose        |limb| < 2^30
mul: T1/T1s x T1/T1s and T2 x T1/T1s; sqr: T1s; fmms: four T1s; norm: |limb| <= 2^31 - 4; freeze: value in (-8p, 24p), |limb| < 2^30;
freeze_near: value in (-2p, 6p), |limb| < 2^30.

The curve reference is affine chord-and-tangent arithmetic: G1 y^2 = x^3 + 3 over Fp, G2 y^2 = x^3 + 3/(9+u) over Fp[u]/(u^2+1).
"""
import os
import random
import struct
import subprocess

P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
MASK = (1 << 29) - 1
M29, M30 = (1 << 29) - 1, (1 << 30) - 1          # largest limb of a (signed-)tight / loose operand
FIELD_MOD = {0: P, 1: R, 2: P}                     # field selectors of the hooks: 0 Fp29, 1 Fr29, 2 Fp29f (chained products)
MUL, SQR, FMMS, NORM, FREEZE, FREEZE_NEAR = range(6)
OP_NAMES = {MUL: "mul", SQR: "sqr", FMMS: "fmms", NORM: "norm", FREEZE: "freeze", FREEZE_NEAR: "freeze_near"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")


# ---------------------------------------------------------------- limbs ----------------------------------------------------------------
def value(l):
    return sum(v << (29 * i) for i, v in enumerate(l))


def tight(v):
    """the digits Field29::norm leaves: limbs 0..7 in [0, 2^29), limb 8 the signed rest"""
    return tuple((v >> (29 * i)) & MASK for i in range(8)) + (v >> 232,)


def predict_product(mod, n):
    m = (-n * pow(mod, -1, 1 << 261)) % (1 << 261)
    v, rest = divmod(n + m * mod, 1 << 261)
    assert rest == 0
    out = tight(v)
    assert -(1 << 31) <= out[8] < (1 << 31)
    return out


def in_class(e, cls):
    if cls == "T1":
        return all(0 <= v <= M29 for v in e[:8]) and abs(e[8]) <= M29
    return all(abs(v) <= {"T1s": M29, "T2": M30, "wide": (1 << 31) - 4}[cls] for v in e)


def _limb(rnd, top, signed):
    v = rnd.randint(0, top)
    if rnd.randrange(5) == 0:
        v = top
    if rnd.randrange(11) == 0:
        v = 0
    return -v if signed and rnd.getrandbits(1) else v


def random_elem(rnd, cls):
    top = {"T1": M29, "T1s": M29, "T2": M30, "wide": (1 << 31) - 4}[cls]
    return tuple(_limb(rnd, top, cls != "T1" or i == 8) for i in range(9))


def extreme_elems(cls):
    """all limbs at +-max, all zero, one non-zero limb in each position, a negative top limb, alternating signs"""
    top = {"T1": M29, "T1s": M29, "T2": M30, "wide": (1 << 31) - 4}[cls]
    lo = 0 if cls == "T1" else -top          # the least value of limbs 0..7
    out = [(top,) * 9, (lo,) * 8 + (-top,), (0,) * 9, (top,) * 8 + (-top,), (top,) * 8 + (-1,), (lo,) * 8 + (top,)]
    out += [tuple(top if i % 2 else lo for i in range(9)), tuple(lo if i % 2 else top for i in range(8)) + (-top,)]
    for i in range(9):
        out.append(tuple(top if j == i else 0 for j in range(9)))
        out.append(tuple(1 if j == i else 0 for j in range(9)))
        if lo or i == 8:
            out.append(tuple(-top if j == i else 0 for j in range(9)))
    assert all(in_class(e, cls) for e in out)
    return out


def _operand_lists(rnd, classes, n):
    """n tuples of operands, operand j of class classes[j]: crossed extremes first, then random limbs with forced extremes"""
    ext = [extreme_elems(c) for c in classes]
    rows = []
    if len(classes) == 2:
        rows += [(x, y) for x in ext[0][:8] for y in ext[1][:8]]
    for i in range(max(len(e) for e in ext)):
        rows.append(tuple(e[(i + 3 * j) % len(e)] for j, e in enumerate(ext)))
    rows += [tuple(e[i % 8] for e in ext) for i in range(8)]          # the same extreme in every operand
    while len(rows) < n:
        rows.append(tuple(random_elem(rnd, c) for c in classes))
    return rows[:n]


MUL_CLASSES = [("T1", "T1"), ("T1s", "T1s"), ("T1", "T1s"), ("T2", "T1"), ("T2", "T1s")]
# element counts: no multiple of 64 among them, at least 4096 per op and field over its classes
LIMB_CLASSES = {
    MUL: {"%sx%s" % c: 835 for c in MUL_CLASSES},
    SQR: {"T1s": 2085, "T1": 2085},
    FMMS: {"T1s": 2085, "T1": 2085},
    NORM: {"T1s": 1381, "T2": 1381, "wide": 1381},
    FREEZE: {"multiples": 0, "extreme": 1051, "random": 3001},
    FREEZE_NEAR: {"multiples": 0, "extreme": 1051, "random": 3001},
}
FREEZE_DOMAIN = {FREEZE: (-8, 24), FREEZE_NEAR: (-2, 6)}


def _respread(rnd, l, moves):
    """another limb vector of the same value: +-2^29 moved between neighbouring limbs, every |limb| kept below 2^30"""
    l = list(l)
    for _ in range(moves):
        i, t = rnd.randrange(8), rnd.choice((-1, 1))
        if abs(l[i] + t * (1 << 29)) <= M30 and abs(l[i + 1] - t) <= M30:
            l[i] += t << 29; l[i + 1] -= t
    return tuple(l)


def _freeze_inputs(rnd, mod, op, cls, n):
    lo, hi = FREEZE_DOMAIN[op]
    vals = []
    if cls == "multiples":      # k p and k p +- 1 for every k the open domain (lo p, hi p) admits, and both of its ends
        for k in range(lo, hi + 1):
            vals += [v for v in (k * mod - 1, k * mod, k * mod + 1) if lo * mod < v < hi * mod]
        assert vals[0] == lo * mod + 1 and vals[-1] == hi * mod - 1
        rows = [tight(v) for v in vals] + [_respread(rnd, tight(v), 24) for v in vals for _ in range(3)]
    elif cls == "extreme":      # limbs 0..7 at +-(2^30 - 1) or alternating, the top limb whatever keeps the value inside the domain
        rows = []
        while len(rows) < n:
            kind = len(rows) % 4
            low = [M30 if kind == 0 else -M30 if kind == 1 else (M30 if (i + kind) % 2 else -M30) for i in range(8)]
            if len(rows) >= 16:
                low = [v if rnd.randrange(3) else rnd.randint(-M30, M30) for v in low]
            v = rnd.randint(lo * mod + 1, hi * mod - 1)
            top = (v - value(low)) >> 232
            e = tuple(low) + (top,)
            if lo * mod < value(e) < hi * mod:
                rows.append(e)
    else:
        rows = [_respread(rnd, tight(rnd.randint(lo * mod + 1, hi * mod - 1)), rnd.randrange(40)) for _ in range(n)]
    for e in rows:
        assert in_class(e, "T2") and lo * mod < value(e) < hi * mod
    return rows


def limb_case(field, op, cls):
    """-> (operands: tuple of lists of 9-limb tuples, as the op reads them; expected: list of 9-limb tuples)"""
    mod = FIELD_MOD[field]
    rnd = random.Random("%d/%d/%s" % (FIELD_MOD[field] & 0xffff, op, cls))      # fields 0 and 2 share their cases
    n = LIMB_CLASSES[op][cls]
    if op in (FREEZE, FREEZE_NEAR):
        a = _freeze_inputs(rnd, mod, op, cls, n)
        want = [tight(value(e) % mod) for e in a]
        assert all(in_class(w, "T1") for w in want)
        return (a,), want
    if op == NORM:
        rows = _operand_lists(rnd, (cls,), n)
        assert all(in_class(r[0], cls) for r in rows)
        return ([r[0] for r in rows],), [tight(value(r[0])) for r in rows]
    classes = {MUL: tuple(cls.split("x")), SQR: (cls,), FMMS: (cls,) * 4}[op]
    rows = _operand_lists(rnd, classes, n)
    want = []
    for r in rows:
        assert all(in_class(e, c) for e, c in zip(r, classes))
        big = [max(abs(v) for v in e) for e in r]
        v = [value(e) for e in r]
        if op == MUL:      # the header's own condition for an exact product
            assert 9 * big[0] * big[1] + 2 ** 61.2 < 2 ** 63
            want.append(predict_product(mod, v[0] * v[1]))
        elif op == SQR:
            want.append(predict_product(mod, v[0] * v[0]))
        else:
            want.append(predict_product(mod, v[0] * v[1] - v[2] * v[3]))
    return tuple([r[j] for r in rows] for j in range(len(classes))), want


def limb_params():
    return [(op, cls) for op in sorted(LIMB_CLASSES) for cls in LIMB_CLASSES[op]]


def limb_mismatches(got, want):
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if tuple(g) != tuple(w)][:5]


# ---------------------------------------------------------------- curves ----------------------------------------------------------------
# field elements are tuples of 1 (Fp) or 2 (Fp2: real, imaginary) integers
def f_add(a, b): return tuple((x + y) % P for x, y in zip(a, b))
def f_sub(a, b): return tuple((x - y) % P for x, y in zip(a, b))
def f_neg(a): return tuple(-x % P for x in a)


def f_mul(a, b):
    if len(a) == 1:
        return (a[0] * b[0] % P,)
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f_inv(a):
    if len(a) == 1:
        return (pow(a[0], -1, P),)
    ni = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * ni % P, -a[1] * ni % P)


def f_small(w, v): return (v % P,) + (0,) * (w - 1)


G1_GEN = ((1,), (2,))
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))
CURVE_B = {0: (3,), 1: f_mul((3, 0), f_inv((9, 1)))}
GEN = {0: G1_GEN, 1: G2_GEN}
DBL, MADD_EXACT, MADD_FAST, ADD, TO_AFF, PARTIAL_SUMS = range(6)
FLAG_INF, FLAG_ZZ0_FIRST, FLAG_ZZ0_LAST = 1, 2, 4


def on_curve(group, pt):
    x, y = pt
    return f_mul(y, y) == f_add(f_mul(f_mul(x, x), x), CURVE_B[group])


assert on_curve(0, G1_GEN) and on_curve(1, G2_GEN)


def ec_neg(p): return None if p is None else (p[0], f_neg(p[1]))


def ec_add(p, q):
    if p is None: return q
    if q is None: return p
    w = len(p[0])
    if p[0] == q[0]:
        if p[1] != q[1] or not any(p[1]):
            return None
        lam = f_mul(f_mul(f_small(w, 3), f_mul(p[0], p[0])), f_inv(f_add(p[1], p[1])))
    else:
        lam = f_mul(f_sub(q[1], p[1]), f_inv(f_sub(q[0], p[0])))
    x = f_sub(f_sub(f_mul(lam, lam), p[0]), q[0])
    return (x, f_sub(f_mul(lam, f_sub(p[0], x)), p[1]))


def ec_mul(k, p):
    acc = None
    for bit in bin(k)[2:]:
        acc = ec_add(acc, acc)
        if bit == "1":
            acc = ec_add(acc, p)
    return acc


def _le32(v): return int(v).to_bytes(32, "little")
def pack_f(a): return b"".join(_le32(x) for x in a)
def pack_point(w, p): return bytes(64 * w) if p is None else pack_f(p[0]) + pack_f(p[1])


def unpack_point(w, b):
    v = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(2 * w)]
    return (tuple(v[:w]), tuple(v[w:]))


_pool_cache = {}


def point_pool(group):
    """small multiples of the generator, random multiples, and their negatives: all finite, all distinct in x except P / -P"""
    if group not in _pool_cache:
        rnd = random.Random(300 + group)
        pts = [ec_mul(k, GEN[group]) for k in range(1, 13)] + [ec_mul(rnd.randrange(1, R), GEN[group]) for _ in range(12)]
        pts += [ec_mul(R - 1, GEN[group]), ec_mul(rnd.getrandbits(64), GEN[group])]
        assert all(on_curve(group, p) for p in pts) and len({p[0] for p in pts}) == len(pts) - 1      # (r-1) G = -G
        _pool_cache[group] = pts + [ec_neg(p) for p in pts[1:12]]
    return _pool_cache[group]


ALL_LIMBS = MASK * sum(1 << (29 * i) for i in range(8))      # every 29-bit digit at its maximum (< 2^232 < p)


def scales(group):
    """the scale lambda of an XYZZ operand: 1, p - 1 and values whose digits are extreme, then random ones; never 0"""
    rnd = random.Random(400 + group)
    base = [1, P - 1, 2, P - 2, ALL_LIMBS, (P - 1) // 2, (P + 1) // 2, MASK, 1 << 29, 1 << 232, (1 << 232) - 1, P - (1 << 29)] + [rnd.randrange(1, P) for _ in range(9)]
    if group == 0:
        return [(v,) for v in base]
    out = [(v, 0) for v in base[:8]] + [(0, v) for v in base[:8]] + [(P - 1, P - 1), (ALL_LIMBS, P - 1), (1, 1)]
    return out + [(rnd.randrange(P), rnd.randrange(1, P)) for _ in range(9)]


class CurveCase:
    """n elements of k points each for one op; expect(): per element (affine point or None, flags)"""

    def __init__(self, group, name, op, elems):
        self.group, self.name, self.op, self.elems = group, name, op, elems      # elems: [(points, (lam0, lam1))]
        self.w = 1 if group == 0 else 2
        self.k = len(elems[0][0])
        assert all(len(p) == self.k for p, _ in elems) and all(any(l) for _, ls in elems for l in ls)

    def packed(self):
        pts = b"".join(pack_point(self.w, p) for ps, _ in self.elems for p in ps)
        inf = bytes(p is None for ps, _ in self.elems for p in ps)
        lam = b"".join(pack_f(l) for _, ls in self.elems for l in ls)
        return pts, inf, lam, len(self.elems), self.k

    def expect(self):
        out = []
        for ps, _ in self.elems:
            flags = 0
            if self.op == DBL:
                r = ec_add(ps[0], ps[0])
            elif self.op == TO_AFF:
                r = ps[0]
            elif self.op == MADD_FAST:
                # madd<false> makes no equality tests: a step acc + P_j with P_j = +-acc leaves ZZ = 0 mod p, and it stays 0
                r = ps[0]
                for j in range(1, self.k):
                    if r is not None and r[0] == ps[j][0]:
                        flags |= FLAG_ZZ0_LAST | (FLAG_ZZ0_FIRST if j == 1 else 0)
                        break
                    r = ec_add(r, ps[j])
                if flags:
                    r = None
            else:
                r = None
                for p in ps:
                    r = ec_add(r, p)
            if r is None and not flags:
                flags = FLAG_INF
            out.append((r, flags))
        return out

    def mismatches(self, out, flags):
        bad = []
        w = self.w
        for i, (r, fl) in enumerate(self.expect()):
            got = unpack_point(w, out[64 * w * i:64 * w * (i + 1)])
            want = unpack_point(w, pack_point(w, r))
            if flags[i] != fl or got != want:
                bad.append((self.name, i, flags[i], fl, got, want))
        return bad[:3]


def curve_cases(group):
    rnd = random.Random(500 + group)
    pool, lams = point_pool(group), scales(group)
    one = f_small(1 if group == 0 else 2, 1)
    lam_pairs = [(lams[i % len(lams)], lams[(7 * i + 3) % len(lams)]) for i in range(len(lams) * 3)]

    def with_lams(lists, unit_first=True):
        """every point list under lambda = 1 and under the other scales in turn"""
        out = [(ps, (one, one)) for ps in lists] if unit_first else []
        return out + [(ps, lam_pairs[i % len(lam_pairs)]) for i, ps in enumerate(lists * 3)]

    generic = [[p, q] for i, p in enumerate(pool) for q in pool[i + 1:i + 4] if p[0] != q[0]][:60]
    same = [[p, p] for p in pool[:20]]
    opposite = [[p, ec_neg(p)] for p in pool[:20]]
    cases = []
    for op, tag in ((MADD_EXACT, "madd_exact"), (MADD_FAST, "madd_fast"), (ADD, "add")):
        cases.append(CurveCase(group, tag + "_generic", op, with_lams(generic)))
        cases.append(CurveCase(group, tag + "_same_point", op, with_lams(same)))            # exact forms must double; the fast form reports ZZ = 0
        cases.append(CurveCase(group, tag + "_opposite_points", op, with_lams(opposite)))    # exact forms give infinity
    cases.append(CurveCase(group, "add_infinity", ADD, with_lams([[None, p] for p in pool[:8]] + [[p, None] for p in pool[:8]] + [[None, None]])))
    cases.append(CurveCase(group, "madd_exact_infinity_first", MADD_EXACT, with_lams([[None, p] for p in pool[:8]])))
    cases.append(CurveCase(group, "madd_fast_infinity_first", MADD_FAST, with_lams([[None, p] for p in pool[:8]])))
    cases.append(CurveCase(group, "dbl", DBL, with_lams([[p] for p in pool] + [[None]])))
    cases.append(CurveCase(group, "to_aff", TO_AFF, with_lams([[p] for p in pool] + [[None]])))
    # accumulations with a repeat and an opposite part-way: P_j = the running sum (the exact form must double), later P_j = -sum (infinity,
    # and the accumulation goes on from there)
    for k, n in ((2, 37), (3, 37), (64, 37), (257, 21)):
        lists = []
        for e in range(n):
            ps = [rnd.choice(pool) for _ in range(k)]
            acc = None
            for j in range(k):
                if e % 3 != 2 and acc is not None and ((k <= 3 and j == k - 1) or (k > 3 and j in (k // 3, 2 * k // 3))):
                    ps[j] = acc if (e + (j > k // 2)) % 2 else ec_neg(acc)
                acc = ec_add(acc, ps[j])
            lists.append(ps)
        cases.append(CurveCase(group, "accumulate_madd_exact_%d" % k, MADD_EXACT, with_lams(lists, unit_first=False)[:n]))
        # partial sums j mod 4: mirrored lists make s0 == s1 (add must double operands whose ZZ is not 1) and s2 == -s3 (infinity)
        mirrored = []
        for e, ps in enumerate(lists):
            ps = list(ps)
            if e % 2:
                for j in range(0, k - 3, 4):
                    ps[j + 1] = ps[j]; ps[j + 3] = ec_neg(ps[j + 2])
            mirrored.append(ps)
        cases.append(CurveCase(group, "accumulate_partial_sums_%d" % k, PARTIAL_SUMS, [(ps, (one, one)) for ps in mirrored]))
    # the contract the hot path relies on: after madd<false> on P = +-Q, ZZ = 0 mod p, and still after 8 more additions
    tail = lambda i: [pool[(i + 2 + 3 * t) % len(pool)] for t in range(8)]
    sticky = [[p, p] + tail(i) for i, p in enumerate(pool[:12])] + [[p, ec_neg(p)] + tail(i) for i, p in enumerate(pool[:12])]
    cases.append(CurveCase(group, "madd_fast_zero_sticks", MADD_FAST, with_lams(sticky)))
    late = []      # generic chains, and chains whose 5th point is +- the sum so far: ZZ = 0 from there on only
    for i in range(24):
        ps = [pool[(i + 5 * t) % len(pool)] for t in range(10)]
        acc = None
        for p in ps[:5]:
            acc = ec_add(acc, p)
        if i % 3 and acc is not None:
            ps[5] = acc if i % 2 else ec_neg(acc)
        late.append(ps)
    cases.append(CurveCase(group, "madd_fast_chain", MADD_FAST, with_lams(late)))
    for c in cases:
        # an affine operand is never infinity
        assert all(p is not None for ps, _ in c.elems for p in (ps[1:] if c.op in (MADD_EXACT, MADD_FAST) else ps if c.op == PARTIAL_SUMS else []))
    return cases


# ---------------------------------------------------------------- host builds ----------------------------------------------------------------
def native_exe(name):
    """tests/native/<name>.cpp, built by g++ with the HIP headers: the device headers with their plain-C products"""
    exe = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "native", name + ".cpp")])
    return exe


def native_limb_ops(exe, field, op, operands):
    n = len(operands[0])
    ops = list(operands) + [operands[0]] * (4 - len(operands))
    payload = struct.pack("<3i", field, op, n) + b"".join(struct.pack("<%di" % (9 * n), *[l for e in o for l in e]) for o in ops)
    out = subprocess.run([exe], input=payload, capture_output=True, timeout=300, check=True).stdout
    flat = struct.unpack("<%di" % (9 * n), out)
    return [flat[9 * i:9 * i + 9] for i in range(n)]


def native_curve_ops(exe, group, op, pts, inf, lam, n, k):
    w = 64 if group == 0 else 128
    out = subprocess.run([exe], input=struct.pack("<4i", group, op, n, k) + pts + inf + lam, capture_output=True, timeout=300, check=True).stdout
    assert len(out) == w * n + n
    return out[:w * n], out[w * n:]
