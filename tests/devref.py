"""References and case tables for the per-operation tests of the device's field and curve code and of the verifier's tower
(gsc_debug_limb_ops, gsc_debug_curve_ops, gsc_debug_tower_ops; include/libprove.h).  Everything here is Python integers; nothing calls
the oracle or the library.

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

The tower section (further down) takes raw limbs as the integers they denote and compares VALUES: Fp2 by the obvious arithmetic, Fp12
by schoolbook products in Fp2[w]/(w^6 - (9+u)) with Frobenius and the exponentiations as plain powers, the Miller steps by affine
arithmetic on the twist, the whole pairing by generic lines on E(Fp12); on the limbs themselves it asserts the bounds verify_dev.hpp
documents.
"""
import functools
import hashlib
import itertools
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


# ---------------------------------------------------------------- the verifier's tower ----------------------------------------------------------------
# gsc_debug_tower_ops (include/libprove.h): raw limbs in the 2^261 Montgomery domain.  A raw integer X stands for the field element
# X / 2^261 mod p; the references below work on field elements (Fp: int, Fp2: (real, imaginary), Fp12: six Fp2, the coefficients of
# w^0..w^5 in Fp2[w] / (w^6 - (9 + u))) and know nothing of the device's formulas.
(T_RED, T_LIN, T_ADD2, T_SUB2, T_NEG2, T_CONJ2, T_MUL2, T_SQR2, T_SCALE2, T_MULXI, T_SMALL2, T_INV1, T_INV2, T_SQRT1, T_SQRT2, T_LEX_LARGE2,
 T_MUL12, T_SQR12, T_MUL_LINE, T_CONJ12, T_FROB12, T_FROB12_2, T_INV12, T_POW_X, T_FINAL_EXP, T_IS_ONE12,
 T_DBL_STEP, T_ADD_STEP, T_FROB_POINTS, T_LINES_OF) = range(30)
TOWER_NAMES = ["red", "lin", "add2", "sub2", "neg2", "conj2", "mul2", "sqr2", "scale2", "mulxi", "small2", "inv1", "inv2", "sqrt1", "sqrt2", "lex_large2",
               "mul12", "sqr12", "mul_line", "conj12", "frob12", "frob12_2", "inv12", "pow_x", "final_exp", "is_one12",
               "dbl_step", "add_step", "frob_points", "lines_of"]
TOWER_PATH1_OPS = list(range(T_MUL12, T_IS_ONE12 + 1))
TOWER_HEAVY = (T_POW_X, T_FINAL_EXP, T_LINES_OF)      # at most 16 elements per path
GROUP_COUNTS = (1, 7, 8, 9, 65)                        # path 1: one group, a wave less one, a full wave, a ragged second wave, nine waves
LINE_STEPS = 102
BN_X = 4965661367192848881
ATE_LOOP = 6 * BN_X + 2
FINAL_EXPONENT = (P ** 12 - 1) // R
MONT = 1 << 261
RINV = pow(MONT, -1, P)
XI = (9, 1)


def tower_words(path, op):
    """(words in, words out) of one element; the table of include/libprove.h"""
    win = {T_RED: 9, T_INV1: 9, T_SQRT1: 9, T_LIN: 20, T_ADD2: 36, T_SUB2: 36, T_MUL2: 36, T_FROB_POINTS: 36, T_LINES_OF: 36, T_SCALE2: 27, T_SMALL2: 19,
           T_MUL12: 216, T_MUL_LINE: 162, T_DBL_STEP: 54, T_ADD_STEP: 90}.get(op, 108 if op >= T_MUL12 else 18)
    wout = {T_RED: 9, T_LIN: 9, T_INV1: 9, T_SQRT1: 9, T_LEX_LARGE2: 0, T_IS_ONE12: 0, T_DBL_STEP: 108, T_ADD_STEP: 108, T_FROB_POINTS: 72,
            T_LINES_OF: 54 * LINE_STEPS}.get(op, (144 if path == 1 else 108) if op >= T_MUL12 else 18)
    return win, wout


# ---- Fp2 / Fp12 references ----
def f2_pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f_mul(r, r)
        if bit == "1":
            r = f_mul(r, a)
    return r


F12_ZERO, F12_ONE = ((0, 0),) * 6, ((1, 0),) + ((0, 0),) * 5


def f12_mul(a, b):
    """schoolbook in Fp2[w] / (w^6 - xi); the sums stay unreduced integers until the end"""
    t0, t1 = [0] * 11, [0] * 11
    for i, (x0, x1) in enumerate(a):
        if x0 or x1:
            for j, (y0, y1) in enumerate(b):
                t0[i + j] += x0 * y0 - x1 * y1; t1[i + j] += x0 * y1 + x1 * y0
    out = []
    for k in range(6):
        h0, h1 = (t0[k + 6], t1[k + 6]) if k < 5 else (0, 0)
        out.append(((t0[k] + 9 * h0 - h1) % P, (t1[k] + h0 + 9 * h1) % P))
    return tuple(out)


def f12_add(a, b): return tuple(f_add(x, y) for x, y in zip(a, b))
def f12_sub(a, b): return tuple(f_sub(x, y) for x, y in zip(a, b))
def f12_conj(a): return tuple(f_neg(c) if i & 1 else c for i, c in enumerate(a))      # w -> -w


@functools.lru_cache(maxsize=None)      # the GPU tests put the same elements through both paths and several group counts
def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_inv(a):
    """through the norms of the tower: N = a conj(a) lies in Fp6 = Fp2[v] / (v^3 - xi) (v = w^2), N's norm to Fp2 is N N' N'' with the two
    other roots of unity of v's minimal polynomial folded in by the adjugate below; 0 -> 0 as the device's Fermat inversions do"""
    if a == F12_ZERO:
        return F12_ZERO
    n = f12_mul(a, f12_conj(a))
    assert n[1] == n[3] == n[5] == (0, 0)
    x, y, z = n[0], n[2], n[4]      # x + y v + z v^2
    # adjugate of multiplication by N in the basis 1, v, v^2
    t0 = f_sub(f_mul(x, x), f_mul(XI, f_mul(y, z)))
    t1 = f_sub(f_mul(XI, f_mul(z, z)), f_mul(x, y))
    t2 = f_sub(f_mul(y, y), f_mul(x, z))
    d = f_inv(f_add(f_mul(x, t0), f_mul(XI, f_add(f_mul(z, t1), f_mul(y, t2)))))
    ninv = (f_mul(t0, d), (0, 0), f_mul(t1, d), (0, 0), f_mul(t2, d), (0, 0))
    r = f12_mul(f12_conj(a), ninv)
    assert f12_mul(r, a) == F12_ONE
    return r


def f12_embed(c, k):
    """c w^k for c in Fp2"""
    return tuple(c if i == k else (0, 0) for i in range(6))


# ---- the generic reduced pairing: E(Fp12): y^2 = x^3 + 3, Q untwisted, affine chord-and-tangent lines evaluated at P ----
def _e12_line_and_sum(t, q, p):
    """the line through t and q (the tangent when they are equal) at p, and t + q; points are pairs of Fp12 elements"""
    (x1, y1), (x2, y2) = t, q
    if x1 == x2:
        assert y1 == y2
        lam = f12_mul(f12_mul(f12_embed((3, 0), 0), f12_mul(x1, x1)), f12_inv(f12_add(y1, y1)))
    else:
        lam = f12_mul(f12_sub(y2, y1), f12_inv(f12_sub(x2, x1)))
    x3 = f12_sub(f12_sub(f12_mul(lam, lam), x1), x2)
    y3 = f12_sub(f12_mul(lam, f12_sub(x1, x3)), y1)
    line = f12_sub(f12_sub(p[1], y1), f12_mul(lam, f12_sub(p[0], x1)))
    return line, (x3, y3)


def pairing_reference(p1, q2):
    """e(P, Q)^((p^12 - 1) / r) for affine P in G1 and Q in G2 (on the twist) -> twelve integers as gsc.debug_pairing returns them"""
    pp = (f12_embed((p1[0][0], 0), 0), f12_embed((p1[1][0], 0), 0))
    q = (f12_embed(q2[0], 2), f12_embed(q2[1], 3))      # (x' w^2, y' w^3) lies on y^2 = x^3 + 3
    assert f12_mul(q[1], q[1]) == f12_add(f12_mul(f12_mul(q[0], q[0]), q[0]), f12_embed((3, 0), 0))
    f, t = F12_ONE, q
    for bit in bin(ATE_LOOP)[3:]:
        line, t = _e12_line_and_sum(t, t, pp)
        f = f12_mul(f12_mul(f, f), line)
        if bit == "1":
            line, t = _e12_line_and_sum(t, q, pp)
            f = f12_mul(f, line)
    q1 = (f12_pow(q[0], P), f12_pow(q[1], P))
    q2n = (f12_pow(q1[0], P), f12_sub(F12_ZERO, f12_pow(q1[1], P)))
    line, t = _e12_line_and_sum(t, q1, pp)
    f = f12_mul(f, line)
    line, t = _e12_line_and_sum(t, q2n, pp)
    f = f12_mul(f, line)
    r = f12_pow(f, FINAL_EXPONENT)
    return tuple(v for c in r for v in c)


_pairing_cache = {}


def pairing_cases():
    """[(P, Q, reduced pairing)] for P = [a]G1, Q = [b]G2: a, b from 1, 2, r - 1, a 40-bit and a 250-bit value; one pair with P = -G1"""
    if not _pairing_cache:
        rnd = random.Random(700)
        s40, s250 = rnd.getrandbits(40) | 1 << 39, rnd.getrandbits(250) | 1 << 249
        pairs = [(1, 1), (2, 1), (1, 2), (R - 1, 2), (2, R - 1), (s40, s250), (s250, s40), (s40, 1), (R - 1, s250)]
        assert pairs[3][0] == R - 1      # P = -G1
        out = []
        for a, b in pairs:
            pt, qt = ec_mul(a, G1_GEN), ec_mul(b, G2_GEN)
            out.append((pt, qt, pairing_reference(pt, qt)))
        assert out[3][0] == ec_neg(G1_GEN)
        _pairing_cache["cases"] = out
    return _pairing_cache["cases"]


# ---- raw operands ----
def to_mont(v): return v * MONT % P
def raw_value(x): return x * RINV % P
def raw2(x): return (raw_value(x[0]), raw_value(x[1]))


def is_reduced(l):
    """what products and red() return: limbs 0..7 in [0, 2^29), |value| < 2.01 p"""
    return all(0 <= v <= M29 for v in l[:8]) and 100 * abs(value(l)) < 201 * P


def is_product(l):
    """what bn254_fp29.hpp documents for Field29::mul: tight, in (-p, 2p)"""
    return all(0 <= v <= M29 for v in l[:8]) and -P < value(l) < 2 * P


def field_values(rnd, n):
    """the canonical values of tests/test_gpu_field.py::_values"""
    edge = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2 ** 29 - 1, 2 ** 29, 2 ** 232, 2 ** 232 - 1, 2 ** 253, P - 2 ** 29, ALL_LIMBS]
    return [e % P for e in edge] + [rnd.randrange(P) for _ in range(max(0, n - len(edge)))]


def _admitted(x):
    """verify_dev.hpp: every value handed to a product is tight with |value| < 5p"""
    l = tight(x)
    assert in_class(l, "T1") and abs(x) < 5 * P and value(l) == x
    return x


def raw_operands(rnd, n):
    """n raw integers: canonical Montgomery images of field_values; values just inside +-5p; sums and differences of two values just inside
    +-2.01p (the lazy sums a product may be handed); both signs, so that the top limb is negative in half of the edge cases"""
    canon = [to_mont(v) for v in field_values(rnd, 14 + n // 3)]
    top5, top2 = 5 * P - 1, (201 * P - 1) // 100
    edge5 = [top5, -top5, top5 - 1, -top5 + 1, top5 - M29, -(top5 - M29), 4 * P, -4 * P, 4 * P + 1, -4 * P - 1]
    edge5 += [s * (top5 - rnd.getrandbits(k)) for k in (8, 29, 64, 200, 232, 250) for s in (1, -1)]
    near2 = [top2, top2 - 1, top2 - rnd.getrandbits(29), top2 - rnd.getrandbits(230), top2 - rnd.getrandbits(250)]
    assert all(100 * v < 201 * P for v in near2)
    sums = [s * (a + t * b) for a in near2 for b in near2[:3] for s in (1, -1) for t in (1, -1)]
    out = canon + edge5 + sums
    while len(out) < n:
        out.append(rnd.choice((1, -1)) * (rnd.choice((4, 3, 0)) * P + rnd.randrange(P)))
    for x in out:
        _admitted(x)
    assert any(tight(x)[8] < 0 for x in out)
    rnd.shuffle(out)
    return out[:n]


def shifted(rnd, v):
    """another admitted raw integer of the field element v: its Montgomery image moved by a multiple of p towards +-5p"""
    m, k = to_mont(v), rnd.choice((4, -5, 3, -4, 0, -1))
    return _admitted(m + (-4 if k == -5 and not m else k) * P)


def _w1(x): return tight(x)
def _w2(x): return tight(x[0]) + tight(x[1])
def _w12(x): return tuple(w for c in x for w in _w2(c))
def _r1(w): return tuple(w[:9])
def _r2(w): return (tuple(w[:9]), tuple(w[9:18]))
def _v1(w): return raw_value(value(w[:9]))
def _v2(w): return (raw_value(value(w[:9])), raw_value(value(w[9:18])))
def _v12(w): return tuple(_v2(w[18 * i:18 * i + 18]) for i in range(6))


def _raw2s(rnd, n):
    a, b = raw_operands(rnd, n), raw_operands(rnd, n)
    return list(zip(a, b))


def f12_shapes(rnd):
    """field elements: 0, 1, w^k alone, every coefficient p - 1, a single non-zero coefficient in each of the 12 slots, elements of the
    cyclotomic subgroup (outputs of the easy part of the final exponentiation), a value and its conjugate, random ones"""
    rand2 = lambda: (rnd.randrange(P), rnd.randrange(P))
    rand12 = lambda: tuple(rand2() for _ in range(6))
    out = [F12_ZERO, F12_ONE] + [f12_embed((1, 0), k) for k in range(1, 6)] + [((P - 1, P - 1),) * 6]
    for k in range(6):
        out += [f12_embed((rnd.randrange(1, P), 0), k), f12_embed((0, rnd.randrange(1, P)), k)]
    for _ in range(2):
        f = rand12()
        e = f12_mul(f12_conj(f), f12_inv(f))                  # f^(p^6 - 1)
        g = f12_mul(f12_pow(e, P * P), e)                      # ^(p^2 + 1)
        assert f12_mul(g, f12_conj(g)) == F12_ONE and g != F12_ONE
        out.append(g)
    v = rand12()
    out += [v, f12_conj(v)]
    return out + [rand12() for _ in range(4)]


def f12_operands(rnd, n):
    """n Fp12 operands as 12 raw integers each: the shapes in canonical form and moved towards +-5p, then raw edge operands in every slot"""
    shapes = f12_shapes(rnd)
    out = [tuple((to_mont(c[0]), to_mont(c[1])) for c in s) for s in shapes]
    out += [tuple((shifted(rnd, c[0]), shifted(rnd, c[1])) for c in s) for s in shapes]
    k = max(n // 3, n - len(out))      # at least a third of any table, small ones included, are raw edge operands
    rnd.shuffle(out)
    out = out[:n - k]
    for _ in range(k):
        r = raw_operands(rnd, 48)
        out.append(tuple((r[2 * i], r[2 * i + 1]) for i in range(6)))
    rnd.shuffle(out)
    assert len(out) == n
    return out


# ---- the twist y^2 = x^3 + 3 / xi in Jacobian coordinates ----
def _jac_dbl(X, Y, Z):
    """(X', Y', Z' = 2YZ) of 2T and the line a yP + b xP w + c w^3 of verify_dev.hpp: a = 2YZ^3, b = -3X^2Z^2, c = 3X^3 - 2Y^2"""
    k = lambda n: (n % P, 0)
    XX, YY, ZZ = f_mul(X, X), f_mul(Y, Y), f_mul(Z, Z)
    line = (f_mul(k(2), f_mul(Y, f_mul(Z, ZZ))), f_neg(f_mul(k(3), f_mul(XX, ZZ))), f_sub(f_mul(k(3), f_mul(XX, X)), f_mul(k(2), YY)))
    m, s = f_mul(k(3), XX), f_mul(k(4), f_mul(X, YY))
    X3 = f_sub(f_mul(m, m), f_mul(k(2), s))
    Y3 = f_sub(f_mul(m, f_sub(s, X3)), f_mul(k(8), f_mul(YY, YY)))
    return (X3, Y3, f_mul(k(2), f_mul(Y, Z))), line


def _jac_add(X, Y, Z, xq, yq):
    """(X', Y', Z' = ZH) of T + Q and the line a = ZH, b = -R, c = R xQ - yQ ZH (H = xQ Z^2 - X, R = yQ Z^3 - Y)"""
    ZZ = f_mul(Z, Z)
    H, Rr = f_sub(f_mul(xq, ZZ), X), f_sub(f_mul(yq, f_mul(Z, ZZ)), Y)
    ZH = f_mul(Z, H)
    line = (ZH, f_neg(Rr), f_sub(f_mul(Rr, xq), f_mul(yq, ZH)))
    HH = f_mul(H, H); HHH = f_mul(H, HH); V = f_mul(X, HH)
    X3 = f_sub(f_sub(f_mul(Rr, Rr), HHH), f_add(V, V))
    Y3 = f_sub(f_mul(Rr, f_sub(V, X3)), f_mul(Y, HHH))
    return (X3, Y3, ZH), line


def jac_affine(X, Y, Z):
    if Z == (0, 0):
        return None
    zi = f_inv(Z); zi2 = f_mul(zi, zi)
    return (f_mul(X, zi2), f_mul(Y, f_mul(zi2, zi)))


_gamma_cache = {}


def twist_frobenius(q):
    """pi(Q) and -pi^2(Q) on the twist: the p-power Frobenius of the untwisted point, twisted back.  (x' w^2)^p = conj(x') xi^((p-1)/3) w^2 and
    (y' w^3)^p = conj(y') xi^((p-1)/2) w^3; the two powers of xi come from plain exponentiation, and the first call checks them against
    x^p computed in Fp12"""
    if not _gamma_cache:
        _gamma_cache[2], _gamma_cache[3] = f2_pow(XI, (P - 1) // 3), f2_pow(XI, (P - 1) // 2)
        x, y = G2_GEN
        assert f12_pow(f12_embed(x, 2), P) == f12_embed(f_mul((x[0], -x[1] % P), _gamma_cache[2]), 2)
        assert f12_pow(f12_embed(y, 3), P) == f12_embed(f_mul((y[0], -y[1] % P), _gamma_cache[3]), 3)
    cj = lambda a: (a[0], -a[1] % P)
    pi = lambda pt: (f_mul(cj(pt[0]), _gamma_cache[2]), f_mul(cj(pt[1]), _gamma_cache[3]))
    q1 = pi(q); q2 = pi(q1)
    return q1, (q2[0], f_neg(q2[1]))


def lines_reference(q):
    """the 102 lines of the Miller loop for Q, chained in Jacobian coordinates from T = (xQ, yQ, 1)"""
    T, out = (q[0], q[1], (1, 0)), []
    for bit in bin(ATE_LOOP)[3:]:
        T, l = _jac_dbl(*T); out.append(l)
        if bit == "1":
            T, l = _jac_add(*T, q[0], q[1]); out.append(l)
    q1, q2 = twist_frobenius(q)
    T, l = _jac_add(*T, q1[0], q1[1]); out.append(l)
    T, l = _jac_add(*T, q2[0], q2[1]); out.append(l)
    assert len(out) == LINE_STEPS
    return out


# ---- case tables: TowerCase.rows are the elements (flat tuples of int32 words); check(row, out, flag) -> None or what is wrong ----
class TowerCase:
    def __init__(self, op, rows, check):
        self.op, self.rows, self.check = op, rows, check
        assert len(rows) % 64 and all(len(r) == tower_words(0, op)[0] for r in rows)

    def mismatches(self, path, outs, flags, n=None):
        rows = self.rows if n is None else self.rows[:n]
        wout = tower_words(path, self.op)[1]
        assert len(outs) == len(flags) == len(rows) and all(len(o) == wout for o in outs)
        bad = []
        for i, (r, o, fl) in enumerate(zip(rows, outs, flags)):
            if path == 1 and wout:
                if any(o[108:]):
                    bad.append((i, "pad lanes are not zero"))
                o = o[:108]
            why = self.check(r, o, fl)
            if why:
                bad.append((i, why))
        return bad[:4]


def _fp2_out(out, want, bound=is_reduced):
    if not (bound(out[:9]) and bound(out[9:18])):
        return "bound: %r" % (out,)
    if _v2(out) != want:
        return "value: got %r, want %r" % (_v2(out), want)


def _fp12_out(out, want, bound=is_reduced):
    for i in range(6):
        why = _fp2_out(out[18 * i:18 * i + 18], want[i], bound)
        if why:
            return "w^%d %s" % (i, why)


def _is_square1(v): return v == 0 or pow(v, (P - 1) // 2, P) == 1
def _is_square2(v): return _is_square1((v[0] * v[0] + v[1] * v[1]) % P)      # the norm test


def _lex_large(v):
    c = v[1] if v[1] else v[0]
    return c > (P - 1) // 2


_tower_cache = {}


def tower_case(op):
    if op not in _tower_cache:
        _tower_cache[op] = _tower_case(op)
    return _tower_cache[op]


def _tower_case(op):
    rnd = random.Random(600 + op)
    flagless = lambda fl: "flag set" if fl else None
    if op == T_RED:
        rows = [_w1(x) for x in raw_operands(rnd, 261)]
        def check(r, o, fl):
            return flagless(fl) or (None if is_reduced(o) and _v1(o) == _v1(r) else "got %r" % (o,))
        return TowerCase(op, rows, check)
    if op == T_LIN:
        ks = [(9, -1), (1, 9), (2, 0), (3, 0), (8, 0), (1, 1), (1, -1), (-1, 0), (0, 1), (9, 9), (-9, -9), (0, 0)]
        rows = [_w1(a) + _w1(b) + ks[i % len(ks)] for i, (a, b) in enumerate(_raw2s(rnd, 261))]
        def check(r, o, fl):
            want = (r[18] * _v1(r) + r[19] * _v1(r[9:])) % P
            return flagless(fl) or (None if is_reduced(o) and _v1(o) == want else "got %r" % (o,))
        return TowerCase(op, rows, check)
    if op in (T_ADD2, T_SUB2, T_MUL2):
        rows = [_w2(a) + _w2(b) for a, b in zip(_raw2s(rnd, 261), _raw2s(rnd, 261))]
        f = {T_ADD2: f_add, T_SUB2: f_sub, T_MUL2: f_mul}[op]
        return TowerCase(op, rows, lambda r, o, fl: flagless(fl) or _fp2_out(o, f(_v2(r), _v2(r[18:]))))
    if op in (T_NEG2, T_CONJ2, T_SQR2, T_MULXI):
        rows = [_w2(a) for a in _raw2s(rnd, 261)]
        f = {T_NEG2: f_neg, T_CONJ2: lambda a: (a[0], -a[1] % P), T_SQR2: lambda a: f_mul(a, a), T_MULXI: lambda a: f_mul(a, XI)}[op]
        return TowerCase(op, rows, lambda r, o, fl: flagless(fl) or _fp2_out(o, f(_v2(r))))
    if op == T_SCALE2:
        rows = [_w2(a) + _w1(k) for a, k in zip(_raw2s(rnd, 261), raw_operands(rnd, 261))]
        def check(r, o, fl):
            k = _v1(r[18:])
            return flagless(fl) or _fp2_out(o, tuple(c * k % P for c in _v2(r)), is_product)
        return TowerCase(op, rows, check)
    if op == T_SMALL2:
        rows = [_w2(a) + ((2, 3, 8)[i % 3],) for i, a in enumerate(_raw2s(rnd, 261))]
        return TowerCase(op, rows, lambda r, o, fl: flagless(fl) or _fp2_out(o, tuple(c * r[18] % P for c in _v2(r))))
    if op == T_INV1:
        rows = [_w1(x) for x in raw_operands(rnd, 133)]
        def check(r, o, fl):
            v = _v1(r)
            return flagless(fl) or (None if is_reduced(o) and _v1(o) == (pow(v, -1, P) if v else 0) else "got %r" % (o,))
        return TowerCase(op, rows, check)
    if op == T_INV2:
        rows = [_w2(a) for a in _raw2s(rnd, 133)]
        return TowerCase(op, rows, lambda r, o, fl: flagless(fl) or _fp2_out(o, f_inv(_v2(r)) if any(_v2(r)) else (0, 0)))
    if op == T_SQRT1:
        vals = [0, 1] + [v * v % P for v in field_values(rnd, 40)] + [-v * v % P for v in field_values(rnd, 40)] + field_values(rnd, 30)
        assert sum(_is_square1(v) for v in vals) > 40 and sum(not _is_square1(v) for v in vals) > 40
        rows = [_w1(to_mont(v)) for v in vals] + [_w1(shifted(rnd, v)) for v in vals] + [_w1(x) for x in raw_operands(rnd, 33)]
        def check(r, o, fl):
            v = _v1(r)
            if fl != _is_square1(v):
                return "flag %d for %d" % (fl, v)
            if not fl:
                return None if not any(o) else "a root without the flag"
            return None if is_reduced(o) and _v1(o) ** 2 % P == v else "root %r" % (o,)
        return TowerCase(op, rows, check)
    if op == T_SQRT2:
        res = [v * v % P for v in field_values(rnd, 20) if v]
        nonres = [-v % P for v in res]      # p = 3 mod 4: -1 is no square
        rand2 = [(rnd.randrange(P), rnd.randrange(1, P)) for _ in range(20)]
        vals = [(0, 0), (1, 0)] + [(v, 0) for v in res] + [(v, 0) for v in nonres] + [f_mul(a, a) for a in rand2] + [f_mul(f_mul(a, a), XI) for a in rand2]
        vals += [(0, v) for v in res[:6]] + rand2
        assert all(_is_square1(v) for v in res) and not any(_is_square1(v) for v in nonres) and not _is_square2(XI)
        assert sum(_is_square2(v) for v in vals) > 40 and sum(not _is_square2(v) for v in vals) > 25
        rows = [_w2((to_mont(v[0]), to_mont(v[1]))) for v in vals] + [_w2((shifted(rnd, v[0]), shifted(rnd, v[1]))) for v in vals] + [_w2(a) for a in _raw2s(rnd, 21)]
        def check(r, o, fl):
            v = _v2(r)
            if fl != _is_square2(v):
                return "flag %d for %r" % (fl, v)
            if not fl:
                return None if not any(o) else "a root without the flag"
            return None if is_reduced(o[:9]) and is_reduced(o[9:]) and f_mul(_v2(o), _v2(o)) == v else "root %r" % (o,)
        return TowerCase(op, rows, check)
    if op == T_LEX_LARGE2:
        # lex_large compares the CANONICAL integer (out of the Montgomery domain) with (p - 1) / 2
        h = (P - 1) // 2
        vals = [(a, b) for a in (0, 1, h, h + 1, P - 1) for b in (0, 1, h, h + 1, P - 1)] + [(rnd.randrange(P), rnd.randrange(P)) for _ in range(40)] + [(rnd.randrange(P), 0) for _ in range(20)]
        rows = [_w2((to_mont(v[0]), to_mont(v[1]))) for v in vals] + [_w2((shifted(rnd, v[0]), shifted(rnd, v[1]))) for v in vals] + [_w2(a) for a in _raw2s(rnd, 31)]
        return TowerCase(op, rows, lambda r, o, fl: None if fl == _lex_large(_v2(r)) else "flag %d for %r" % (fl, _v2(r)))
    if op in (T_MUL12, T_SQR12, T_MUL_LINE, T_CONJ12, T_FROB12, T_FROB12_2, T_INV12, T_POW_X, T_FINAL_EXP):
        n = {T_MUL12: 101, T_SQR12: 101, T_MUL_LINE: 101, T_CONJ12: 101, T_FROB12: 67, T_FROB12_2: 67, T_INV12: 67, T_POW_X: 13, T_FINAL_EXP: 13}[op]
        a = f12_operands(rnd, n)
        if op == T_MUL12:
            b = f12_operands(rnd, n)
            rows = [_w12(x) + _w12(y) for x, y in zip(a, b)]
            return TowerCase(op, rows, lambda r, o, fl: flagless(fl) or _fp12_out(o, f12_mul(_v12(r), _v12(r[108:]))))
        if op == T_MUL_LINE:
            cs = [_raw2s(rnd, n) for _ in range(3)]
            rows = [_w12(x) + _w2(cs[0][i]) + _w2(cs[1][i]) + _w2(cs[2][i]) for i, x in enumerate(a)]
            def check(r, o, fl):
                c0, c1, c3 = _v2(r[108:]), _v2(r[126:]), _v2(r[144:])
                return flagless(fl) or _fp12_out(o, f12_mul(_v12(r), (c0, c1, (0, 0), c3, (0, 0), (0, 0))))
            return TowerCase(op, rows, check)
        rows = [_w12(x) for x in a]
        if op == T_CONJ12:
            def check(r, o, fl):      # the even coefficients pass through as they are
                if any(o[36 * i:36 * i + 18] != r[36 * i:36 * i + 18] for i in range(3)):
                    return "an even coefficient changed"
                return flagless(fl) or _fp12_out(o, f12_conj(_v12(r)), lambda l: in_class(l, "T1"))
            return TowerCase(op, rows, check)
        if op == T_FROB12_2:      # coefficient 0 passes through; the others are products that scale2 returns unreduced
            return TowerCase(op, rows, lambda r, o, fl: flagless(fl) or ("coefficient 0 changed" if o[:18] != r[:18] else
                                                                         "bound" if not all(is_product(o[9 * i:9 * i + 9]) for i in range(2, 12)) else
                                                                         None if _v12(o) == f12_pow(_v12(r), P * P) else "value"))
        f = {T_SQR12: lambda x: f12_mul(x, x), T_FROB12: lambda x: f12_pow(x, P), T_INV12: f12_inv, T_POW_X: lambda x: f12_pow(x, BN_X),
             T_FINAL_EXP: lambda x: f12_pow(x, FINAL_EXPONENT)}[op]
        def check(r, o, fl):
            if op == T_INV12 and _v12(r) != F12_ZERO and f12_mul(_v12(o), _v12(r)) != F12_ONE:
                return "a * inv(a) != 1"
            return flagless(fl) or _fp12_out(o, f(_v12(r)))
        return TowerCase(op, rows, check)
    if op == T_IS_ONE12:
        one, zero = to_mont(1), 0
        base = [(one, zero)] + [(zero, zero)] * 5
        elems = []      # (12 raw integers as six pairs, is it one)
        for wave in range(8):      # path 1: wave j of eight groups holds its one element that is not 1 at group position j
            for pos in range(8):
                e = [tuple(shifted(rnd, raw_value(x)) if wave % 2 else x for x in c) for c in base]
                if pos == wave:
                    s = rnd.randrange(12)
                    c = list(e[s // 2]); c[s % 2] += 1; e[s // 2] = tuple(c)
                elems.append((tuple(e), pos != wave))
        for s in range(12):        # a stray 1 in each of the 12 Fp slots: the raw integer 1, and the field element 1
            for stray in (1, one):
                e = [list(c) for c in base]
                e[s // 2][s % 2] += stray
                elems.append((tuple(tuple(c) for c in e), False))
        elems += [(tuple((shifted(rnd, 1), shifted(rnd, 0)) if i == 0 else (shifted(rnd, 0), shifted(rnd, 0)) for i in range(6)), True) for _ in range(7)]
        assert len(elems) == 64 + 24 + 7 and sum(1 for _, w in elems if not w) == 8 + 24
        want = {_w12(e): w for e, w in elems}
        for e, w in elems:
            assert (tuple(raw2(c) for c in e) == F12_ONE) == w
        return TowerCase(op, [_w12(e) for e, _ in elems], lambda r, o, fl: None if bool(fl) == want[tuple(r)] else "flag %d" % fl)
    # ---- Miller steps ----
    pool = point_pool(1)
    lam = [l for l in scales(1) if l != (0, 0)]
    def jac(i):      # point i of the pool under a scale: (x l^2, y l^3, l)
        (x, y), l = pool[i % len(pool)], lam[(5 * i + 1) % len(lam)] if i % 4 else (1, 0)
        l2 = f_mul(l, l)
        return (f_mul(x, l2), f_mul(y, f_mul(l2, l)), l)
    rep = lambda i, v: (to_mont(v[0]), to_mont(v[1])) if i % 3 == 0 else (shifted(rnd, v[0]), shifted(rnd, v[1]))
    def step_check(r, o, want_t, want_line):
        if not all(is_reduced(o[9 * i:9 * i + 9]) for i in range(12)):
            return "bound"
        got_t = jac_affine(_v2(o), _v2(o[18:]), _v2(o[36:]))
        if got_t != want_t:
            return "T': got %r, want %r" % (got_t, want_t)
        got_line = (_v2(o[54:]), _v2(o[72:]), _v2(o[90:]))
        return None if got_line == want_line else "line: got %r, want %r" % (got_line, want_line)
    if op == T_DBL_STEP:
        rows = [_w2(rep(i, T[0])) + _w2(rep(i + 1, T[1])) + _w2(rep(i + 2, T[2])) for i, T in ((i, jac(i)) for i in range(101))]
        def check(r, o, fl):
            T = (_v2(r), _v2(r[18:]), _v2(r[36:]))
            a = jac_affine(*T)
            return flagless(fl) or step_check(r, o, ec_add(a, a), _jac_dbl(*T)[1])
        return TowerCase(op, rows, check)
    if op == T_ADD_STEP:
        rows = []
        for i in range(101):
            T, q = jac(i), pool[(3 * i + 7) % len(pool)]
            if pool[i % len(pool)][0] == q[0]:
                q = pool[(3 * i + 8) % len(pool)]
            assert pool[i % len(pool)][0] != q[0]      # the Miller loop never adds T = +-Q
            rows.append(_w2(rep(i, T[0])) + _w2(rep(i + 1, T[1])) + _w2(rep(i + 2, T[2])) + _w2(rep(i + 1, q[0])) + _w2(rep(i, q[1])))
        def check(r, o, fl):
            T, q = (_v2(r), _v2(r[18:]), _v2(r[36:])), (_v2(r[54:]), _v2(r[72:]))
            return flagless(fl) or step_check(r, o, ec_add(jac_affine(*T), q), _jac_add(*T, *q)[1])
        return TowerCase(op, rows, check)
    qs = [ec_mul(k, G2_GEN) for k in (1, 2, R - 1, rnd.getrandbits(40), rnd.getrandbits(250))]
    if op == T_FROB_POINTS:
        qs = qs + pool[:28]
        rows = [_w2(rep(i, q[0])) + _w2(rep(i + 1, q[1])) for i, q in enumerate(qs)]
        def check(r, o, fl):
            q1, q2 = twist_frobenius((_v2(r), _v2(r[18:])))
            return flagless(fl) or _fp2_out(o, q1[0]) or _fp2_out(o[18:], q1[1]) or _fp2_out(o[36:], q2[0]) or _fp2_out(o[54:], q2[1])
        return TowerCase(op, rows, check)
    assert op == T_LINES_OF
    qs = qs + qs[:4] + pool[12:16]
    rows = [_w2(rep(i // 5, q[0])) + _w2(rep(i // 5 + 1, q[1])) for i, q in enumerate(qs)]
    def check(r, o, fl):
        want = lines_reference((_v2(r), _v2(r[18:])))
        for s in range(LINE_STEPS):
            w = o[54 * s:54 * s + 54]
            if not all(is_reduced(w[9 * i:9 * i + 9]) for i in range(6)):
                return "step %d: bound" % s
            if (_v2(w), _v2(w[18:]), _v2(w[36:])) != want[s]:
                return "step %d: line" % s
        return flagless(fl)
    return TowerCase(op, rows, check)


def _self_check_jacobian():
    """the chained Jacobian model above against affine arithmetic, once"""
    T = (G2_GEN[0], G2_GEN[1], (1, 0))
    T2, _ = _jac_dbl(*T)
    assert jac_affine(*T2) == ec_add(G2_GEN, G2_GEN)
    T3, _ = _jac_add(*T2, *G2_GEN)
    assert jac_affine(*T3) == ec_mul(3, G2_GEN)


_self_check_jacobian()


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


def native_tower_ops(exe, path, op, rows, wout=None):
    """tests/native/tower_check.cpp: paths 0 and 1 as the hook, 2 and 3 the whole pairing (serial / lane-sliced) -> (outs, flags)"""
    n = len(rows)
    wout = tower_words(path, op)[1] if wout is None else wout
    payload = struct.pack("<3i", path, op, n) + struct.pack("<%di" % (len(rows[0]) * n), *[w for r in rows for w in r])
    out = subprocess.run([exe], input=payload, capture_output=True, timeout=300, check=True).stdout
    assert len(out) == 4 * wout * n + n
    flat = struct.unpack("<%di" % (wout * n), out[:4 * wout * n])
    return [flat[wout * i:wout * (i + 1)] for i in range(n)], list(out[4 * wout * n:])


def native_curve_ops(exe, group, op, pts, inf, lam, n, k):
    w = 64 if group == 0 else 128
    out = subprocess.run([exe], input=struct.pack("<4i", group, op, n, k) + pts + inf + lam, capture_output=True, timeout=300, check=True).stdout
    assert len(out) == w * n + n
    return out[:w * n], out[w * n:]


# ---------------------------------------------------------------- the MSM kernels ----------------------------------------------------------------
# gsc_debug_msm (include/libprove.h).  Bases are P_k = b_k G with b_k chosen by the test, so the sum of column p is (sum_k s_kp b_k mod r) G: ONE
# scalar multiplication per column whatever the number of bases, and the point at infinity exactly when that integer is 0.  The multiplication is
# Jacobian integer arithmetic over a fixed-window table of G (test_msm_model_host.py holds it against ec_mul).  The digit layouts are modelled
# from the text of csrc/kernels.hpp, so that a case cannot pass by silently taking a slow path.
HALF_R = (R - 1) // 2
MSM_FLAT_ESCAPE, MSM_GROUP_ENTRIES, MSM_FEW_PROOFS, WS_PLANE_WIDE = -32768, 3280, 32, -128
KIND_BIT, KIND_NARROW, KIND_WIDE = 0, 1, 2


def jac_double(w, T):
    """2T for T = (X, Y, Z) on y^2 = x^3 + b, or None for the point at infinity"""
    if T is None or not any(T[1]):
        return None
    X, Y, Z = T
    k = lambda n: f_small(w, n)
    XX, YY = f_mul(X, X), f_mul(Y, Y)
    m, s = f_mul(k(3), XX), f_mul(k(4), f_mul(X, YY))
    X3 = f_sub(f_mul(m, m), f_add(s, s))
    return (X3, f_sub(f_mul(m, f_sub(s, X3)), f_mul(k(8), f_mul(YY, YY))), f_mul(k(2), f_mul(Y, Z)))


def jac_madd(w, T, q):
    """T + q for Jacobian T (or None) and affine q; equal points double, opposite points give None"""
    if T is None:
        return (q[0], q[1], f_small(w, 1))
    X, Y, Z = T
    ZZ = f_mul(Z, Z)
    H, Rr = f_sub(f_mul(q[0], ZZ), X), f_sub(f_mul(q[1], f_mul(Z, ZZ)), Y)
    if not any(H):
        return jac_double(w, T) if not any(Rr) else None
    HH = f_mul(H, H); HHH = f_mul(H, HH); V = f_mul(X, HH)
    X3 = f_sub(f_sub(f_mul(Rr, Rr), HHH), f_add(V, V))
    return (X3, f_sub(f_mul(Rr, f_sub(V, X3)), f_mul(Y, HHH)), f_mul(Z, H))


def jac_to_affine(T):
    if T is None:
        return None
    zi = f_inv(T[2]); zi2 = f_mul(zi, zi)
    return (f_mul(T[0], zi2), f_mul(T[1], f_mul(zi2, zi)))


_gen_tables = {}
GEN_WINDOW = 8


def _gen_table(group):
    """table[j][d - 1] = d 2^(8 j) G, affine, for the 32 byte positions of a scalar"""
    if group not in _gen_tables:
        w = 1 if group == 0 else 2
        rows, base = [], GEN[group]
        for _ in range(256 // GEN_WINDOW):
            row, acc = [base], (base[0], base[1], f_small(w, 1))
            for _d in range(2, 1 << GEN_WINDOW):
                acc = jac_madd(w, acc, base)
                row.append(jac_to_affine(acc))
            rows.append(row)
            base = jac_to_affine(jac_madd(w, acc, base))      # 2^8 times the row's base
        _gen_tables[group] = rows
    return _gen_tables[group]


def gen_mul(group, k):
    """(k mod r) G as an affine point, None for the point at infinity"""
    w, acc, k = (1 if group == 0 else 2), None, k % R
    for j, row in enumerate(_gen_table(group)):
        d = (k >> (GEN_WINDOW * j)) & ((1 << GEN_WINDOW) - 1)
        if d:
            acc = jac_madd(w, acc, row[d - 1])
    return jac_to_affine(acc)


def raw_point(group, p):
    """a finite point as gsc_debug_msm takes it: big-endian X | Y, in G2 the imaginary part first"""
    be = lambda v: int(v).to_bytes(32, "big")
    if group == 0:
        return be(p[0][0]) + be(p[1][0])
    return be(p[0][1]) + be(p[0][0]) + be(p[1][1]) + be(p[1][0])


def msm_windows(c):
    """csrc/kernels.hpp msm_windows: the fewest windows whose top one takes the last carry: floor((r-1) / 2^(c (nwin-1))) + 1 <= 2^(c-1) - 1"""
    nwin = 1
    while ((R - 1) >> (c * (nwin - 1))) + 1 > (1 << (c - 1)) - 1:
        nwin += 1
    return nwin


def sign_normalise(s):
    """(|s|, negated): the representative of s in [-(r-1)/2, (r-1)/2]"""
    return (R - s, True) if s > HALF_R else (s, False)


def signed_digits(mag, c, n, negated):
    """n signed c-bit digits of the magnitude mag, each in [-D, D - 1], D = 2^(c-1); for a negated scalar the digits are negated and the split
    threshold moves by one (signed_digit_step of csrc/msm_dev.hpp)"""
    Dh, carry, out = 1 << (c - 1), 0, []
    for _ in range(n):
        raw = (mag & ((1 << c) - 1)) + carry
        mag >>= c
        if raw >= Dh + (1 if negated else 0):
            raw -= 1 << c; carry = 1
        else:
            carry = 0
        out.append(-raw if negated else raw)
    assert mag == 0 and carry == 0 and all(-Dh <= d < Dh for d in out)
    return out


def _i16x8(vals):
    assert len(vals) == 8
    return struct.pack("<8h", *vals)


def win_digit_words(scalars, rows, batch, c, mont):
    """k_recode's output: digits[(j noct + o) batch + p] = the eight digits of window j of the bases 8o .. 8o+7 (int16; at c = 17 int32, two words per
    index); scalars[row * batch + p]; rows: the scalar row of every base the buffer is laid out for"""
    nwin, noct = msm_windows(c), (len(rows) + 7) // 8
    dig = {}
    for k, row in enumerate(rows):
        for p in range(batch):
            s = scalars[row * batch + p]
            mag, neg = sign_normalise(s) if mont else (s, False)
            dig[k, p] = signed_digits(mag, c, nwin, neg)
    out = bytearray()
    zero = [0] * nwin
    for j in range(nwin):
        for o in range(noct):
            for p in range(batch):
                e = [dig.get((8 * o + i, p), zero)[j] for i in range(8)]
                out += struct.pack("<8i", *e) if c > 16 else _i16x8(e)
    return bytes(out)


class FlatPlan:
    """The flat layout of csrc/msm_layout.hpp, stated again: [bit groups][narrow rows][padding to an octet][window octets of the expanded wide bases].
    Bits that do not fill an octet become narrow rows of length 2 in front of the narrow ones; padding repeats the first base on the zero row; a wide
    base becomes ceil(nwv / 8) octets of (base, window) pairs at shift cv q, row length 2^(cv-1); slots past the nwv windows have shift 0, length 1."""

    def __init__(self, bits, narrow, narrow_len, wide, rows, zero_row, uniform=False, expand_cv=0, expand_max=0, expand_c=0):
        bits, narrow, narrow_len, wide = list(bits), list(narrow), list(narrow_len), list(wide)
        self.src, self.shift, self.frows, self.len, self.octwin, self.nbit, self.nexpanded, self.cv, self.wide, self.nflat = [], [], [], [], [], 0, 0, 0, wide, 0
        if uniform and expand_cv <= 0:
            return
        keep = len(bits) - len(bits) % 8
        narrow, narrow_len = bits[keep:] + narrow, [2] * (len(bits) - keep) + narrow_len
        bits = bits[:keep]
        self.src = bits + narrow
        self.frows = [rows[i] for i in self.src]
        self.len = [1] * len(bits) + narrow_len
        while len(self.src) % 8:
            self.src.append(self.src[0]); self.frows.append(zero_row); self.len.append(1)
        self.shift = [0] * len(self.src)
        self.octwin = [-1] * (len(self.src) // 8)
        self.nbit = len(bits)
        if wide and (expand_cv > 0 or len(wide) <= expand_max):
            self.cv = expand_cv if expand_cv > 0 else expand_c
            nwv = msm_windows(self.cv)
            for wb in wide:
                for q in range(8 * ((nwv + 7) // 8)):
                    self.src.append(wb); self.frows.append(rows[wb])
                    self.shift.append(self.cv * q if q < nwv else 0); self.len.append(1 << (self.cv - 1) if q < nwv else 1)
                    if q % 8 == 0:
                        self.octwin.append(q)
            self.nexpanded, self.wide = len(wide), []
        self.nflat = len(self.src)


def sort_bases(status, rows, cls, uniform, bit_groups, margin, max_bits):
    """msm_sort_bases: what the calibration classes make of a key's bases -> (bits, narrow, narrow_len, wide)"""
    bits, narrow, narrow_len, wide = [], [], [], []
    for i, st in enumerate(status):
        if st == 2:
            continue
        k = 255 if uniform or rows[i] >= len(cls) else cls[rows[i]]
        if uniform or bit_groups <= 0 or k == 255 or k + margin > max_bits:
            wide.append(i)
        elif k <= 1:
            bits.append(i)
        else:
            narrow.append(i); narrow_len.append(1 << max(0, k + margin))
    return bits, narrow, narrow_len, wide


def flat_digit_words(plan, scalars, batch, mont, group_ok, nproofs=0, plane=None, plane_rows=0, plane_stride=0):
    """k_recode_flat's (nproofs = 0) or k_recode_flat_few's output -> (digits, gok).  digits[o batch + p] = eight int16; a bit group whose columns are
    all ternary — over the wave of 64 columns, or (latency kernel) in the one column — and whose group_ok is set carries the balanced-ternary value in
    slot 0 and gok 1, else ordinary values: the sign-normalised scalar, or MSM_FLAT_ESCAPE from 2^15 on.  Window octets carry the digits
    octwin .. octwin + 7 of one scalar.  gok[o (batch / 64) + wave], in the latency kernel gok[o 32 + p]; what no thread writes stays zero."""
    noct, ng, few = plan.nflat // 8, plan.nbit // 8, nproofs > 0
    digits = [[None] * batch for _ in range(noct)]
    gok = bytearray(ng * (MSM_FEW_PROOFS if few else batch // 64))
    cols = range(nproofs) if few else range(batch)

    def entry(row, p):      # the byte plane's entry for (row, p), or WS_PLANE_WIDE
        if plane is None or row >= plane_rows:
            return WS_PLANE_WIDE
        v = plane[((p >> 6) * plane_stride + row) * 64 + (p & 63)]
        return v - 256 if v > 127 else v

    def value(row, p):      # the scalar of (row, p) as an integer mod r
        t = entry(row, p)
        return scalars[row * batch + p] if t == WS_PLANE_WIDE else t % R

    for o in range(noct):
        rows = plan.frows[8 * o:8 * o + 8]
        if plan.octwin[o] >= 0:
            for p in cols:
                mag, neg = sign_normalise(value(rows[0], p))
                nw = max(msm_windows(plan.cv), plan.octwin[o] + 8)
                digits[o][p] = signed_digits(mag, plan.cv, nw, neg)[plan.octwin[o]:plan.octwin[o] + 8]
            continue
        assert mont, "canonical scalars reach window octets only"
        waves = [[p] for p in cols] if few else [list(range(64 * g, 64 * g + 64)) for g in range(batch // 64)]
        for wi, wave in enumerate(waves):
            all_plane = plane is not None and all(entry(r, p) != WS_PLANE_WIDE for r in rows for p in wave)
            vals = {p: [sign_normalise(value(r, p)) for r in rows] for p in wave}
            tern = all(m <= 1 for p in wave for m, _ in vals[p])
            if o < ng:
                # with every entry in the plane the values are ternary by construction; otherwise the kernel tests the 32-byte elements
                ok = (True if all_plane else tern) and group_ok[o] != 0
                if few:
                    gok[o * MSM_FEW_PROOFS + wave[0]] = ok
                else:
                    gok[o * (batch // 64) + wi] = ok
                if ok:
                    for p in wave:
                        digits[o][p] = [sum((-m if n else m) * 3 ** i for i, (m, n) in enumerate(vals[p]))] + [0] * 7
                    continue
            for p in wave:
                digits[o][p] = [MSM_FLAT_ESCAPE if m >= 1 << 15 else (-m if n else m) for m, n in vals[p]]
    out = bytearray()
    for o in range(noct):
        for p in range(batch):
            out += _i16x8(digits[o][p] if digits[o][p] is not None else [0] * 8)
    return bytes(out), bytes(gok)


def group_tabulates(bs):
    """group_ok of a bit group: 0 when some signed subset sum of its bases, other than the empty one, is the point at infinity (k_build_subset
    meets every such sum on its way through the table)"""
    return 0 if any(any(ts) and sum(t * b for t, b in zip(ts, bs)) % R == 0 for ts in itertools.product((-1, 0, 1), repeat=len(bs))) else 1


_point_cache = {}


def base_point(group, b):
    if (group, b) not in _point_cache:
        _point_cache[group, b] = raw_point(group, gen_mul(group, b))
    return _point_cache[group, b]


class MsmCase:
    """One call of gsc_debug_msm and everything the test holds it against.  b[k]: the discrete logarithm of base k; kind / rowlen / rows per base;
    scalars[row * batch + p] integers below r.  expect: info-block entries the route must show."""

    def __init__(self, group, name, b, kind, rows, scalars, n_rows, c, rowlen=None, cv=0, mont=1, batch=64, nproofs=0, per_flat=0, per_win=0, digit_rows=None,
                 plane=None, plane_rows=0, plane_stride=0, expect=None):
        self.group, self.name, self.b, self.kind, self.rows, self.scalars, self.n_rows, self.c = group, name, list(b), list(kind), list(rows), list(scalars), n_rows, c
        self.rowlen = list(rowlen) if rowlen else [0] * len(self.b)
        self.cv, self.mont, self.batch, self.nproofs, self.per_flat, self.per_win, self.digit_rows = cv, mont, batch, nproofs, per_flat, per_win, digit_rows
        self.plane, self.plane_rows, self.plane_stride, self.expect = plane, plane_rows, plane_stride, dict(expect or {})
        self.zero_row = n_rows - 1
        assert len(self.scalars) == n_rows * batch and all(0 <= s < R for s in self.scalars) and not any(self.scalars[self.zero_row * batch:])
        assert all(0 < x < R for x in self.b) and len(self.kind) == len(self.rows) == len(self.b)
        idx = lambda kd: [k for k, x in enumerate(self.kind) if x == kd]
        self.plan = FlatPlan(idx(KIND_BIT), idx(KIND_NARROW), [self.rowlen[k] for k in idx(KIND_NARROW)], idx(KIND_WIDE), self.rows, self.zero_row, False, cv)
        self.ncols = nproofs or batch

    def points(self):
        return b"".join(base_point(self.group, x) for x in self.b)

    def value(self, row, p):
        if self.plane is not None and row < self.plane_rows:
            v = self.plane[((p >> 6) * self.plane_stride + row) * 64 + (p & 63)]
            v = v - 256 if v > 127 else v
            if v != WS_PLANE_WIDE:
                return v % R
        return self.scalars[row * self.batch + p]

    def exponents(self):
        return [sum(self.value(r, p) * x for r, x in zip(self.rows, self.b)) % R for p in range(self.ncols)]

    def expected(self):
        """(coordinates, infinity flags) of every column, as the hook returns them"""
        w = 1 if self.group == 0 else 2
        pts = [gen_mul(self.group, e) for e in self.exponents()]
        return b"".join(pack_point(w, p) for p in pts), bytes(p is None for p in pts)

    def group_ok(self):
        return bytes(group_tabulates([self.b[k] for k in self.plan.src[8 * o:8 * o + 8]]) for o in range(self.plan.nbit // 8))

    def flat_model(self):
        return flat_digit_words(self.plan, self.scalars, self.batch, self.mont, self.group_ok(), self.nproofs, self.plane, self.plane_rows, self.plane_stride)

    def win_model(self):
        rows = self.digit_rows if self.digit_rows else [self.rows[k] for k in self.plan.wide]
        return win_digit_words(self.scalars, rows, self.batch, self.c, self.mont) if self.plan.wide else b""

    def call(self, gsc):
        return gsc.debug_msm(self.group, self.points(), self.kind, self.rowlen, self.rows, self.scalars, self.n_rows, self.zero_row, self.c, self.cv, self.mont, self.batch,
                             self.nproofs, self.per_flat, self.per_win, self.digit_rows, self.plane, self.plane_rows, self.plane_stride)


def windowed_patterns(c, mont, rnd, n):
    """n scalars for a windowed base: 0, 1, r - 1, (r -+ 1) / 2; every digit D - 1 / D / D + 1 (the carry chain, the int16 minimum at c = 16, the moved
    threshold of a negated scalar); only the top window; 2^(c j) - 1; random values.  mont = 1 scalars are sign-normalised by the kernel, so the
    digit patterns are given as magnitudes and as their negatives."""
    nwin, Dh = msm_windows(c), 1 << (c - 1)
    vals = [0, 1, R - 1, HALF_R, HALF_R + 1]
    for w in (Dh - 1, Dh, Dh + 1):
        for bound in ((HALF_R, R - 1) if mont else (R - 1,)):
            top = nwin - 1
            while sum(w << (c * j) for j in range(top)) > bound:
                top -= 1
            v = sum(w << (c * j) for j in range(top))
            vals += [v, R - v] if mont and v else [v]
    top = 1 << (c * (nwin - 1))
    vals += [top, R - top] if top < R else []
    vals += [(1 << (c * j)) - 1 for j in (1, 2, nwin // 2, nwin - 1) if (1 << (c * j)) - 1 < R]
    vals += [R - ((1 << (c * j)) - 1) for j in (1, nwin - 1)]
    vals = [v % R for v in vals]
    while len(vals) < n:
        vals.append(rnd.randrange(R))
    return vals


FLAT_EDGES = (0, 1, -1, 32767, -32767, 32768, -32768, HALF_R, HALF_R + 1, 2, -2)


def flat_patterns(rowlen, rnd, n):
    """n scalars for a flat base with a row of rowlen entries: 0, +-1, +-rowlen (the row's last entry), +-(rowlen + 1) (beyond the row: multiplied out),
    +-32767 (the largest value that is no escape), +-32768 and full-width values (escapes)"""
    vals = list(FLAT_EDGES) + [rowlen, -rowlen, rowlen + 1, -rowlen - 1, rowlen - 1]
    vals = [v % R for v in vals]
    while len(vals) < n:
        vals.append(rnd.choice((rnd.randrange(R), rnd.randrange(-rowlen, rowlen + 1) % R, rnd.randrange(-40000, 40000) % R)))
    return vals


def _matrix(cols_of_base, batch, n_extra_rows=1):
    """scalars[row][p] from one list of per-column values per base (row k = base k), plus zero rows"""
    out = []
    for col in cols_of_base:
        assert len(col) == batch
        out += col
    return out + [0] * (batch * n_extra_rows)


def _rot(vals, k, batch):
    return [vals[(p + 5 * k) % len(vals)] for p in range(batch)]


def _b_list(rnd, n):
    return [rnd.randrange(1, R) for _ in range(n)]


def msm_cases(group):
    """the case table of tests/test_gpu_msm.py; tests/test_msm_model_host.py proves its internal consistency on a CPU first"""
    rnd = random.Random(900 + group)
    cases = []

    def windowed(name, c, nb, mont, batch=64, expect=None, b=None, cols=None, **kw):
        b = b or _b_list(rnd, nb)
        pats = windowed_patterns(c, mont, rnd, batch)
        cols = cols or [_rot(pats, k, batch) for k in range(nb)]
        cases.append(MsmCase(group, name, b, [KIND_WIDE] * nb, range(nb), _matrix(cols, batch), nb + 1, c, mont=mont, batch=batch, expect=expect, **kw))

    # ---- windowed geometry: nbases 1, 7, 8, 9, 64, 65 and 8 q + 3; c = 4, 6, 15, 16, 17; both kinds of scalars ----
    for nb, mont in ((1, 1), (7, 0), (8, 1), (9, 0), (64, 1), (65, 0)):
        windowed("win_c6_n%d_mont%d" % (nb, mont), 6, nb, mont, per_win=8, expect={3: nb, 4: 43, 7: (nb + 7) // 8, 8: 8})
    windowed("win_c4_n65_engine_slices", 4, 65, 1, expect={3: 65})                                  # per = 0: msm_slices
    windowed("win_c15_n19_per8", 15, 19, 1, per_win=8, expect={7: 3, 4: 17})                        # a ragged last octet in a ragged last slice
    windowed("win_c15_n67_per64", 15, 67, 0, per_win=64, expect={7: 2})
    for mont in (0, 1):
        windowed("win_c16_n9_mont%d" % mont, 16, 9, mont, per_win=8, expect={4: 16, 7: 2})          # digit -D = the int16 minimum
        windowed("win_c17_n24_mont%d" % mont, 17, 24, mont, per_win=8, batch=128, expect={4: 15, 7: 3})   # two words per digit octet
    windowed("win_c16_n65_batch128", 16, 65, 1, per_win=64, batch=128, expect={7: 2})
    windowed("win_c17_n9_few5", 17, 9, 1, nproofs=5, expect={7: 1, 8: 512})
    # ---- reductions: 8 and 9 slices (the tail branch of xcd_slice), 65 slices: two butterfly levels; by-proof then butterfly ----
    windowed("win_c8_n64_8slices", 8, 64, 1, per_win=8, expect={7: 8, 26: 1, 27: 8, 28: 0})
    windowed("win_c8_n72_9slices", 8, 72, 0, per_win=8, expect={7: 9, 26: 1, 27: 9, 28: 0})
    windowed("win_c8_n520_butterfly_twice", 8, 520, 1, per_win=8, expect={4: 32, 7: 65, 26: 2, 27: 65, 28: 0, 29: 2, 30: 0})
    windowed("win_c6_n520_by_proof", 6, 520, 1, per_win=8, expect={4: 43, 7: 65, 26: 2, 27: 65, 28: 1, 29: 3, 30: 0})
    # ---- latency kernels: 1, 5, 32 columns; 63, 64, 65, 129 bases in one slice of 512 and cut by 64 ----
    for nb, npr, per in ((63, 1, 0), (64, 5, 0), (65, 32, 0), (129, 5, 0), (63, 32, 64), (64, 1, 64), (65, 5, 64), (129, 32, 64)):
        windowed("win_few_c6_n%d_p%d_per%d" % (nb, npr, per), 6, nb, (nb + npr) & 1, nproofs=npr, per_win=per,
                 expect={7: (nb + 63) // 64 if per else 1, 8: per or 512, 44: npr})
    windowed("win_few_c16_n65_p5", 16, 65, 1, nproofs=5, per_win=64, expect={7: 2})
    # ---- digits laid out for more bases than are walked: recode 40, walk the first 19 ----
    for npr in (0, 5):
        pats = windowed_patterns(6, 1, rnd, 64)
        cols = [_rot(pats, k, 64) for k in range(40)]
        cases.append(MsmCase(group, "win_digit_bases_40_walk_19_p%d" % npr, _b_list(rnd, 19), [KIND_WIDE] * 19, range(19), _matrix(cols, 64), 41, 6, per_win=8, nproofs=npr,
                             digit_rows=list(range(40)), expect={3: 19, 46: 5, 7: 3}))
    # ---- collisions in the windowed kernel: P + P at the head of a slice (madd<false> leaves ZZ = 0: the repair), P + (-P) midway ----
    b0 = rnd.randrange(1, R)
    pats = windowed_patterns(6, 1, rnd, 64)
    tail = [_rot(pats, k, 64) for k in range(2, 11)]
    windowed("win_collision_same_base", 6, 11, 1, b=[b0, b0] + _b_list(rnd, 9), cols=[pats, pats] + tail, per_win=8)
    windowed("win_collision_opposite_base", 6, 11, 1, b=[b0, R - b0] + _b_list(rnd, 9), cols=[pats, pats] + tail, per_win=8)
    # a column whose sum is the point at infinity (the last base's scalar cancels the others), and the all-zero column
    bs = _b_list(rnd, 9)
    cols = [_rot(pats, k, 64) for k in range(8)]
    cols.append([(-sum(cols[k][p] * bs[k] for k in range(8)) * pow(bs[8], -1, R)) % R if p % 2 else rnd.randrange(R) for p in range(64)])
    for k in range(9):
        cols[k][0] = 0
    windowed("win_sum_is_infinity", 16, 9, 0, b=bs, cols=cols, per_win=8)

    # ---- flat: ordinary values against rows of 1, 2, 5 and 256 entries; slices of 8 (65 of them: two butterfly levels) and the engine's own ----
    def flat(name, kinds, lens, cols, batch=64, b=None, n_extra=1, **kw):
        nb = len(kinds)
        cases.append(MsmCase(group, name, b or _b_list(rnd, nb), kinds, range(nb), _matrix(cols, batch, n_extra), nb + n_extra, kw.pop("c", 6), rowlen=lens, batch=batch, **kw))

    for nb, per, exp in ((1, 0, {0: 8}), (7, 8, {5: 1}), (9, 8, {5: 2, 0: 16}), (64, 8, {5: 8, 9: 1}), (65, 64, {5: 2}), (520, 8, {5: 65, 9: 2, 10: 65, 11: 0, 12: 2})):
        lens = [(1, 2, 5, 256)[k % 4] for k in range(nb)]
        flat("flat_narrow_n%d_per%d" % (nb, per), [KIND_NARROW] * nb, lens, [_rot(flat_patterns(lens[k], rnd, 64), k, 64) for k in range(nb)], per_flat=per, expect=exp)
    # ---- bit groups: v = 3280 (the table's last entry), -3280, only t_7, all zero, random ternary; 7 bits (all demoted), 9 bits (one demoted) ----
    def ternary_cols(nb, batch):
        cols = [[rnd.choice((0, 1, R - 1)) for _ in range(batch)] for _ in range(nb)]
        for k in range(nb):
            cols[k][0], cols[k][1], cols[k][2], cols[k][3] = 1, R - 1, (1 if k % 8 == 7 else 0), 0
            cols[k][4] = R - 1 if k % 8 == 7 else 0
        return cols
    for nb in (7, 8, 9, 16):
        flat("bits_n%d" % nb, [KIND_BIT] * nb, None, ternary_cols(nb, 64), expect={1: nb - nb % 8, 0: (nb + 7) // 8 * 8})
    # one wave entirely ternary; in the other a single column holds a 2 in one wire: gok = [1, 0], and still the right sums
    cols = ternary_cols(16, 128)
    cols[11][64 + 37] = 2
    flat("bits_one_wave_not_ternary", [KIND_BIT] * 16, None, cols, batch=128, expect={1: 16})
    # the colliding pair inside a bit group: its subset sums hit the point at infinity, group_ok = 0, the group is walked base by base
    for tag, b1 in (("same", b0), ("opposite", R - b0)):
        flat("bits_collision_%s_base" % tag, [KIND_BIT] * 16, None, ternary_cols(16, 64), b=[b0, b1] + _b_list(rnd, 14), expect={1: 16})
    # the same pairs in narrow rows at the head of a slice, equal scalars: the ZZ = 0 repair of the flat kernel; later bases follow
    cols = [_rot(flat_patterns(5, rnd, 64), 0, 64)] * 2 + [_rot(flat_patterns(5, rnd, 64), k, 64) for k in range(2, 11)]
    for tag, b1 in (("same", b0), ("opposite", R - b0)):
        flat("flat_collision_%s_base" % tag, [KIND_NARROW] * 11, [5] * 11, cols, b=[b0, b1] + _b_list(rnd, 9), per_flat=8)
    bs = _b_list(rnd, 9)
    cols = [_rot(flat_patterns(5, rnd, 64), k, 64) for k in range(8)]
    cols.append([(-sum(cols[k][p] * bs[k] for k in range(8)) * pow(bs[8], -1, R)) % R if p % 2 else 3 for p in range(64)])
    for k in range(9):
        cols[k][0] = 0
    flat("flat_sum_is_infinity", [KIND_NARROW] * 9, [5] * 9, cols, b=bs, per_flat=8)
    # ---- flat latency kernels: 1, 64 and 65 octets; 1, 5, 32 columns ----
    for noct, npr in ((1, 1), (64, 5), (65, 32)):
        nb = 8 * noct
        kinds = [KIND_BIT] * 16 + [KIND_NARROW] * (nb - 16) if nb > 16 else [KIND_NARROW] * nb
        lens = [(1, 2, 5, 256)[k % 4] for k in range(nb)]
        cols = [_rot(flat_patterns(lens[k], rnd, 64), k, 64) for k in range(nb)]
        if nb > 16:
            cols[:16] = ternary_cols(16, 64)
            cols[9][3] = 5      # one column of group 1 is not ternary: its gok is 0 beside the other columns' 1
        flat("flat_few_oct%d_p%d" % (noct, npr), kinds, lens, cols, nproofs=npr, expect={45: noct, 5: (noct + 63) // 64, 44: npr})
    # ---- a set with every part: bit groups, narrow rows and wide bases — windowed (Horner with the flat sum as addend) or expanded ----
    def mixed(name, nwide, batch=64, wide_vals=None, **kw):
        c = kw.pop("c", 6)
        kinds = [KIND_BIT] * 9 + [KIND_NARROW] * 5 + [KIND_WIDE] * nwide
        lens = [0] * 9 + [2, 5, 256, 1, 5] + [0] * nwide
        cols = ternary_cols(9, batch) + [_rot(flat_patterns(lens[k], rnd, batch), k, batch) for k in range(9, 14)]
        wp = wide_vals or windowed_patterns(kw.get("cv") or c, 1, rnd, batch)
        cols += [_rot(wp, k, batch) for k in range(nwide)]
        flat(name, kinds, lens, cols, batch=batch, c=c, **kw)
    mixed("mixed_horner_addend", 9, per_win=8, per_flat=8, expect={43: 1, 1: 8, 3: 9})
    mixed("mixed_horner_addend_c16_batch128", 3, batch=128, c=16, expect={43: 1})
    mixed("mixed_horner_addend_few", 9, nproofs=5, expect={43: 1, 44: 5})
    # expanded wide wires: cv = 8 (32 windows: four full octets), cv = 15 (17 windows: seven padding slots whose digits must be 0)
    edge = [R - 1, HALF_R, HALF_R + 1, 0, 1]
    mixed("mixed_expanded_cv8", 2, cv=8, wide_vals=edge + windowed_patterns(8, 1, rnd, 64), expect={2: 2, 3: 0, 47: 8, 0: 16 + 2 * 32})
    mixed("mixed_expanded_cv15", 2, cv=15, wide_vals=edge + windowed_patterns(15, 1, rnd, 64), expect={2: 2, 47: 15, 0: 16 + 2 * 24})
    mixed("mixed_expanded_cv15_few", 2, cv=15, nproofs=5, wide_vals=edge + windowed_patterns(15, 1, rnd, 64), expect={2: 2, 44: 5})
    # canonical scalars reach the flat kernels through all-window sets only (the latency layout of the quotient bases)
    for npr in (0, 32):
        pats = edge + windowed_patterns(8, 0, rnd, 64)
        cases.append(MsmCase(group, "expanded_canonical_cv8_p%d" % npr, _b_list(rnd, 3), [KIND_WIDE] * 3, range(3), _matrix([_rot(pats, k, 64) for k in range(3)], 64), 4, 6, cv=8, mont=0,
                             nproofs=npr, expect={2: 3, 0: 96, 1: 0}))
    # ---- the byte plane: entries 0, 1, -1 and WS_PLANE_WIDE; the 32-byte rows the plane covers hold OTHER valid values ----
    for batch, npr in ((128, 0), (64, 5)):
        nb = 24
        kinds = [KIND_BIT] * 16 + [KIND_NARROW] * 8
        lens = [0] * 16 + [5] * 8
        cols = [[rnd.randrange(R) for _ in range(batch)] for _ in range(nb)]      # what a kernel reading the wrong source would use
        stride, prow = nb + 3, nb - 2                                             # the last two narrow rows lie outside the plane
        plane = bytearray((batch // 64) * stride * 64)
        for r in range(prow):
            for p in range(batch):
                wide_here = (r == 5 and p >= 64) or (r >= 16 and (p + r) % 3 == 0)      # group 0 of the second wave; some narrow entries
                t = WS_PLANE_WIDE if wide_here else rnd.choice((0, 1, -1))
                plane[((p >> 6) * stride + r) * 64 + (p & 63)] = t & 0xFF
                if wide_here:
                    cols[r][p] = rnd.choice((0, 1, R - 1)) if r < 16 and p % 2 else flat_patterns(5, rnd, 24)[(p + r) % 24]
        for r in range(prow, nb):
            cols[r] = _rot(flat_patterns(5, rnd, batch), r, batch)
        flat("plane_batch%d_p%d" % (batch, npr), kinds, lens, cols, batch=batch, nproofs=npr, plane=bytes(plane), plane_rows=prow, plane_stride=stride, expect={1: 16})
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


_msm_case_cache = {}


def msm_case_table(group):
    if group not in _msm_case_cache:
        _msm_case_cache[group] = {c.name: c for c in msm_cases(group)}
    return _msm_case_cache[group]


MSM_CASE_NAMES = None


def msm_case_names():
    global MSM_CASE_NAMES
    if MSM_CASE_NAMES is None:
        MSM_CASE_NAMES = list(msm_case_table(0))
        assert MSM_CASE_NAMES == list(msm_case_table(1))
    return MSM_CASE_NAMES


# ---------------------------------------------------------------- proof assembly ----------------------------------------------------------------
# gsc_debug_assemble (include/libprove.h).  Every input point is a known multiple of the generator, so every output is one: tmp[0] = (s a) G,
# tmp[1] = (r b1) G, Krs = (k + z + s a + r b1 [+ c]) G, and the point at infinity exactly when that integer is 0 mod r.  A point is carried as its
# discrete logarithm, None for the point at infinity.  The scalar multiplications are modelled twice: the batch kernel as the plain product, the
# latency kernel lane by lane from the words glv_split hands it (glv_words is glv.hpp's arithmetic in Python integers;
# test_assemble_model_host.py holds it against the C++).  `variant` names a WRONG kernel, for the sensitivity check of the table.
GLV_LAMBDA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd
GLV_BETA = 0x59e26bcea0d48bacd4f263f1acdb5c4f5763473177fffffe
GLV_A1 = 9931322734385697763
GLV_B1_ABS = 147946756881789319000765030803803410728
GLV_A2 = 147946756881789319010696353538189108491
GLV_G1, GLV_G2 = (GLV_A1 << 384) // R, (GLV_B1_ABS << 384) // R
FR_MONT = (1 << 256) % R
ASSEMBLE_VARIANTS = ("rs_exchanged", "neg_exchanged", "straddle_ignored", "q25_ignored", "batch_from_bit_252", "beta_on_first_half", "c_ignored",
                     "flag_shift_wrong", "flagged_part_zeroed")
ASSEMBLE_SETS = ("a", "b1", "k", "z", "b2", "c", "d", "pok")
STRADDLES = (6, 12, 19, 25)


def expand_message_xmd48(msg, dst):
    """RFC 9380 expand_message_xmd with SHA-256, 48 bytes out"""
    dst = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + (48).to_bytes(2, "big") + b"\0" + dst).digest()
    b1 = hashlib.sha256(b0 + b"\x01" + dst).digest()
    b2 = hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b1)) + b"\x02" + dst).digest()
    return (b1 + b2)[:48]


def commitment_challenge(cpts64):
    """k_challenge_from_point: hash_to_field of the commitment's 64 bytes, DST "bsb22-commitment" """
    return int.from_bytes(expand_message_xmd48(cpts64, b"bsb22-commitment"), "big") % R


def glv_halves(k):
    """glv.hpp glv_split: (k1, k2) signed, k = k1 + k2 lambda mod r"""
    c1, c2 = (k * GLV_G1) >> 384, (k * GLV_G2) >> 384
    return k - c1 * GLV_A1 - c2 * GLV_A2, c1 * GLV_B1_ABS - c2 * GLV_A1


def glv_words(k):
    """the GlvSplit record of k: (five words of |k1|, five words of |k2|, neg)"""
    k1, k2 = glv_halves(k)
    assert abs(k1) < 1 << 130 and abs(k2) < 1 << 130
    words = lambda v: tuple((abs(v) >> (32 * i)) & 0xFFFFFFFF for i in range(5))
    return words(k1), words(k2), (1 if k1 < 0 else 0) | (2 if k2 < 0 else 0)


def glv_record(k, rec=None):
    k1, k2, neg = glv_words(k) if rec is None else rec
    return struct.pack("<11I", *k1, *k2, neg)


def glv_chosen(k1, k2, neg):
    """a GlvSplit record from chosen magnitudes below 2^130, and the scalar it stands for"""
    assert 0 <= k1 < 1 << 130 and 0 <= k2 < 1 << 130 and 0 <= neg <= 3
    words = lambda v: tuple((v >> (32 * i)) & 0xFFFFFFFF for i in range(5))
    return (words(k1), words(k2), neg), ((-k1 if neg & 1 else k1) + (-k2 if neg & 2 else k2) * GLV_LAMBDA) % R


def glv_chunks(words, variant=None):
    """the 26 five-bit chunks k_fin_scalarmul_few's lanes cut from five words"""
    out = []
    for q in range(26):
        o = 5 * q
        w, sh = o >> 5, o & 31
        chunk = words[w] >> sh
        if sh > 27 and variant != "straddle_ignored":
            chunk |= (words[w + 1] << (32 - sh)) & 0xFFFFFFFF
        out.append(0 if variant == "q25_ignored" and q == 25 else chunk & 31)
    return out


def latency_product(k, a, variant=None, rec=None):
    """the discrete logarithm of what k_fin_scalarmul_few's wave leaves for the point a G and the halves of the scalar k (rec: a GlvSplit record
    given instead of glv_split's): lanes 0..25 own the chunks of k1 on 2^(5q) P, lanes 32..57 those of k2 on phi(2^(5q) P) = lambda 2^(5q) P,
    each half negated by its bit of neg; the other lanes hold chunk 0"""
    k1w, k2w, neg = glv_words(k) if rec is None else rec
    if variant == "neg_exchanged":
        neg = (neg >> 1) | ((neg & 1) << 1)
    total = 0
    for second, words in ((False, k1w), (True, k2w)):
        phi = second != (variant == "beta_on_first_half")
        sign = -1 if (neg >> (1 if second else 0)) & 1 else 1
        for q, chunk in enumerate(glv_chunks(words, variant)):
            total += sign * chunk * (a << (5 * q)) * (GLV_LAMBDA if phi else 1)
    return total % R


def batch_product(k, a, variant=None):
    """k_fin_scalarmul: double-and-add over bits 253..0"""
    return (k & ((1 << (253 if variant == "batch_from_bit_252" else 254)) - 1)) * a % R


@functools.lru_cache(maxsize=None)
def _dlog_point(group, e):
    return None if e is None else gen_mul(group, e)


def _le_point(group, e):
    return pack_point(1 if group == 0 else 2, _dlog_point(group, e))


def _dsum(*es):
    es = [e for e in es if e is not None]
    return (sum(es) % R or None) if es else None


class AssembleCase:
    """Columns of one gsc_debug_assemble call.  A column: the discrete logarithms a, b1, k, z, c, d, pok (G1) and b2 (G2), None = infinity; r, s,
    mask; name."""

    def __init__(self, cols):
        self.cols = list(cols)
        self.batch = len(self.cols)

    def rotated(self, by):
        return AssembleCase(self.cols[by:] + self.cols[:by])

    def scalars(self):
        return [c[key] for c in self.cols for key in ("r", "s")]

    def rs(self):
        return b"".join(_le32(c["r"]) + _le32(c["s"]) for c in self.cols)

    def mask(self):
        return b"".join(_le32(c["mask"]) for c in self.cols)

    def sets(self, has_c=True, has_commit=True, unit_scales=False):
        """the point sets as the hook takes them: raw big-endian points (zeros at infinity), infinity bytes, big-endian scales"""
        out = {}
        for j, name in enumerate(ASSEMBLE_SETS):
            if (name == "c" and not has_c) or (name in ("d", "pok") and not has_commit):
                continue
            group = 1 if name == "b2" else 0
            sc = scales(group)
            pts, inf, lam = [], bytearray(), []
            for p, col in enumerate(self.cols):
                e = col[name]
                pts.append(bytes(128 if group else 64) if e is None else raw_point(group, _dlog_point(group, e)))
                inf.append(1 if e is None else 0)
                l = f_small(2 if group else 1, 1) if unit_scales else sc[(5 * p + 3 * j + 1) % len(sc)]
                lam.append(b"".join(int(v).to_bytes(32, "big") for v in reversed(l)))
            out[name] = (b"".join(pts), bytes(inf), b"".join(lam))
        return out

    def expected(self, nproofs=0, has_c=True, has_commit=True, fill=0xA5, variant=None, halves=None):
        """every output of the hook, byte for byte.  nproofs != 0: the latency kernel wrote Ar, its flag and tmp of the first nproofs columns only;
        k_fin_combine ran over the whole batch with tmp = infinity in the others.  halves: the records [column][s, r] the kernel got as glv_in"""
        B = self.batch
        out, flags = bytearray([fill]) * (256 * B), bytearray(B)
        tmp, tmp_inf = bytearray(128 * B), bytearray(2 * B)
        cpts, commit, W, mask_out = bytearray(128 * B), bytearray(32 * B), bytearray(128 * B), bytearray(32 * B)
        product = functools.partial(latency_product if nproofs else batch_product, variant=variant)
        assert halves is None or len(halves) == nproofs

        def flag(p, bit):
            q = (p & ~3) | ((p + 1) & 3) if variant == "flag_shift_wrong" else p
            if q < B:
                flags[q] |= bit

        def part(p, off, size, group, e, bit):
            if e is None:
                flag(p, bit)
                if variant == "flagged_part_zeroed":
                    out[256 * p + off:256 * p + off + size] = bytes(size)
            else:
                out[256 * p + off:256 * p + off + size] = _le_point(group, e)

        for p, col in enumerate(self.cols):
            r, s = col["r"], col["s"]
            for row, v in enumerate((r, s, -r * s % R, 0)):
                W[32 * (row * B + p):32 * (row * B + p) + 32] = _le32(v * FR_MONT % R)
            mask_out[32 * p:32 * p + 32] = _le32(col["mask"] * FR_MONT % R)
            if variant == "rs_exchanged":
                r, s = s, r
            t = [None, None]
            if not nproofs or p < nproofs:
                part(p, 0, 64, 0, col["a"], 1)
                rec = [{}, {}] if halves is None else [{"rec": h} for h in (halves[p][::-1] if variant == "rs_exchanged" else halves[p])]
                t = [None if col["a"] is None else product(s, col["a"], **rec[0]) or None, None if col["b1"] is None else product(r, col["b1"], **rec[1]) or None]
            for role in (0, 1):
                tmp[64 * (role * B + p):64 * (role * B + p) + 64] = _le_point(0, t[role])
                tmp_inf[role * B + p] = 1 if t[role] is None else 0
            part(p, 64, 128, 1, col["b2"], 2)
            part(p, 192, 64, 0, _dsum(col["k"], col["z"], t[0], t[1], col["c"] if has_c and variant != "c_ignored" else None), 4)
            if has_commit:
                for at, e, bit in ((p, col["d"], 8), (B + p, col["pok"], 16)):
                    if e is None:
                        flag(p, bit)
                    else:
                        cpts[64 * at:64 * at + 64] = raw_point(0, _dlog_point(0, e))
                commit[32 * p:32 * p + 32] = _le32(commitment_challenge(bytes(cpts[64 * p:64 * p + 64])) * FR_MONT % R)
        res = {"out": bytes(out), "flags": bytes(flags), "tmp": bytes(tmp), "tmp_inf": bytes(tmp_inf), "W": bytes(W), "mask_out": bytes(mask_out)}
        if has_commit:
            res.update(cpts=bytes(cpts), commit=bytes(commit))
        if nproofs:
            res["glv"] = b"".join(glv_record(c[key], halves and halves[p][i]) for p, c in enumerate(self.cols[:nproofs]) for i, key in enumerate(("s", "r")))
        return res


def glv_compose(k1, k2):
    return (k1 + k2 * GLV_LAMBDA) % R


def assemble_scalars():
    """(the edge values, the values built from chosen halves)"""
    rnd = random.Random(1201)
    lam = GLV_LAMBDA
    fixed = [0, 1, 2, R - 1, R - 2, HALF_R, HALF_R + 1, 1 << 253, (1 << 253) + 1, lam, lam - 1, lam + 1, R - lam, lam * lam % R, 1 << 127, (1 << 128) - 1, 1 << 128]
    a, b = rnd.getrandbits(120) | 1 << 119, rnd.getrandbits(120) | 1 << 119
    built = [glv_compose(a, b), glv_compose(a, -b), glv_compose(-a, b), glv_compose(-a, -b), glv_compose(0, b), glv_compose(a, 0),
             glv_compose((1 << 125) - 1, (1 << 125) - 1), glv_compose((1 << 130) - 1, (1 << 130) - 1)]
    for q in range(26):      # one non-zero chunk at position q of one half; the top position takes a value the split keeps below 2^127
        c = (31, 1, 16, 21, 10)[q % 5] if q < 25 else 3
        built += [glv_compose(c << (5 * q), 0), glv_compose(0, -(c << (5 * q)) if q & 1 else c << (5 * q))]
    # the straddling positions with all five bits set, in both halves at once, under each pair of signs
    for i, q in enumerate(STRADDLES):
        v = (31 if q < 25 else 3) << (5 * q)
        built.append(glv_compose(-v if i & 1 else v, -v if i & 2 else v))
    return fixed, built


def assemble_halves():
    """32 columns of chosen halves [s, r] for glv_in: what k_fin_scalarmul_few's contract admits and glv_split never returns, too.  Every chunk 31
    under each pair of signs; a zero half, also with its sign bit set; one non-zero chunk at each of the 26 positions of each half, the top one
    (bits 125..129, the fifth word) included; random 130-bit magnitudes under each pair of signs."""
    rnd = random.Random(1203)
    top = (1 << 130) - 1
    recs = [glv_chosen(top, top, neg) for neg in range(4)]
    recs += [glv_chosen(0, rnd.getrandbits(130), 0), glv_chosen(rnd.getrandbits(130), 0, 0), glv_chosen(0, rnd.getrandbits(130), 3), glv_chosen(rnd.getrandbits(130), 0, 3)]
    for q in range(26):
        c = (31, 1, 16, 21, 10)[q % 5] if q < 25 else 31
        recs += [glv_chosen(c << (5 * q), 0, q & 3), glv_chosen(0, c << (5 * q), (q + 1) & 3)]
    recs += [glv_chosen(rnd.getrandbits(130) | 1 << 129, rnd.getrandbits(130) | 1 << 129, neg) for neg in range(4)]
    assert len(recs) == 64
    return [(recs[2 * p][0], recs[2 * p + 1][0]) for p in range(32)]


def assemble_columns(n=64):
    """The case table: one pattern per column.  Flagged columns sit at p = 4 g + g mod 4 (one per 32-bit flag word, at each byte position in turn), with
    clean columns around them; n = 67 adds three columns in a partly used flag word, each flagged differently."""
    assert n in (64, 67)
    rnd = random.Random(1202)
    fixed, built = assemble_scalars()
    nz = lambda: rnd.randrange(1, R)
    ordinary = [rnd.getrandbits(250), nz(), nz(), rnd.getrandbits(64), nz(), rnd.getrandbits(250), nz()] + [nz() for _ in range(6)]
    pool = built + ordinary
    assert len(fixed) == 17 and len(pool) == 17 + 60
    r_list = fixed + [fixed[(5 * i + 3) % 17] for i in range(17, 34)] + pool[17:77:2]
    s_list = pool[:17] + fixed + pool[18:77:2]
    assert len(r_list) == 64 and len(s_list) == 64
    cols = []
    for p in range(64):
        col = {key: nz() for key in ASSEMBLE_SETS}
        col.update(r=r_list[p], s=s_list[p], mask=(0, 1, R - 1)[p] if p < 3 else nz(), name="generic")
        cols.append(col)

    def pattern(p, name, **kw):
        cols[p].update(kw, name=name)
        return cols[p]

    sa_rb = lambda c: (c["s"] * c["a"] + c["r"] * c["b1"]) % R
    # flagged in every mode
    c = pattern(0, "Ar, Bs and Krs at infinity", a=None, b2=None, c=None); c["z"] = R - c["k"]; assert c["r"] == 0
    pattern(5, "A at infinity", a=None)
    pattern(10, "B2 at infinity", b2=None)
    pattern(15, "all at infinity", **{key: None for key in ASSEMBLE_SETS})
    # flagged in some modes
    pattern(16, "D at infinity", d=None)
    pattern(21, "Pok at infinity", pok=None)
    c = pattern(26, "K + Z = -(sA + rB1)"); c["z"] = (-sa_rb(c) - c["k"]) % R
    c = pattern(31, "K + Z + sA + rB1 = -C"); c["c"] = (-sa_rb(c) - c["k"] - c["z"]) % R
    # clean
    c = pattern(1, "K = Z"); c["z"] = c["k"]
    c = pattern(2, "K = -Z"); c["z"] = R - c["k"]
    c = pattern(3, "sA = rB1"); c["s"] = c["r"]; c["b1"] = c["a"]
    c = pattern(4, "sA = -rB1"); c["b1"] = -c["s"] * c["a"] * pow(c["r"], -1, R) % R
    c = pattern(6, "K + Z = sA + rB1"); c["z"] = (sa_rb(c) - c["k"]) % R
    c = pattern(7, "K + Z + sA + rB1 = C"); c["c"] = (sa_rb(c) + c["k"] + c["z"]) % R
    pattern(8, "C at infinity", c=None)
    pattern(9, "B1 at infinity", b1=None)
    pattern(11, "K at infinity", k=None)
    pattern(12, "Z at infinity", z=None)
    c = pattern(17, "s = 0 with A finite"); assert c["s"] == 0
    c = pattern(30, "r = 0"); assert c["r"] == 0
    for c in cols:
        assert all(c[key] is None or 0 < c[key] < R for key in ASSEMBLE_SETS) and 0 <= c["r"] < R and 0 <= c["s"] < R
    if n == 67:
        for name, kw in (("A at infinity", {"a": None}), ("B2 at infinity", {"b2": None}), ("D and Krs at infinity", {"d": None, "k": None, "z": None, "c": None, "s": 0, "r": 0})):
            col = {key: nz() for key in ASSEMBLE_SETS}
            col.update(r=nz(), s=nz(), mask=nz(), name=name)
            col.update(kw)
            cols.append(col)
    return cols


_assemble_cache = {}


def assemble_table(n=64):
    if n not in _assemble_cache:
        _assemble_cache[n] = AssembleCase(assemble_columns(n))
    return _assemble_cache[n]
