"""The witness solver in plain Python integers mod r, a builder for small synthetic constraint systems, and the case table of
tests/test_gpu_solver.py (the hook gsc_debug_solve, include/libprove.h).

  * Circuit: add a coefficient, r1c(L, R, O), nbits(expr, n), lookup(table, exprs), count(rows, queries), randomize(n), commit(wires); it emits the
    hook's description — the fields of gnark's R1CS file.  Wires are numbered as gnark numbers them: the constant, the public,
    the secret, then the internal wires in the order they are created.
  * solve(): the sequential solver of SURVEY.md App. C as oracle/r1cs.c states it, walking the instructions in file order.  Per column it returns
    (W, A, B, C) or the index of the first failing instruction.  tests/test_solver_model_host.py holds it against the oracle on the shipped circuits.
  * check(): independent of solve() — every L(w) R(w) == O(w) evaluated directly, nBits outputs recombining to their input, lookup outputs equal to
    the table entry, counts summing to the number of queries.
  * schedule(): the level schedule of the device program restated (csrc/formats.hpp SolverProgram::sched), to name the op a status word means.
  * small_flag(): which values break a prediction of the small-integer path (csrc/wit_small.hpp).
An expression is a list of (coefficient value, wire) pairs; wire CONST stands for the constant term."""
import functools
import random

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)
CONST = 0xFFFFFFFF
HINT_NBITS, HINT_COUNT, HINT_RANDOMIZE, HINT_BSB22 = 4115454955, 2138922168, 1774611027, 4156202267
BP_HINT, BP_R1C, BP_LOOKUP = 0, 1, 2
HALF = (R - 1) // 2
P253 = 1 << 253


def to_mont_bytes(v):
    return (v % R * MONT % R).to_bytes(32, "little")


def from_mont_bytes(b):
    """-> (the value times 2^-256, the stored integer)"""
    x = int.from_bytes(b, "little")
    return x * MONT_INV % R, x


class Circuit:
    def __init__(self, n_public=0, n_secret=0):
        self.n_public, self.n_secret = 1 + n_public, n_secret
        self.coeffs = [0, 1, 2, R - 1, R - 2]
        self.calldata, self.blueprint, self.constraint_off, self.wire_off = [], [], [], []
        self.bp_kind, self.bp_entries = [BP_HINT, BP_R1C], [[], []]
        self.n_wires = self.n_public + n_secret
        self.n_constraints = 0
        self.has_commitment, self.commit_wire, self.commit_private = False, 0, []

    # ---- building ----
    def inputs(self):
        return list(range(1, self.n_public + self.n_secret))

    def coeff(self, v, fresh=False):
        v %= R
        if not fresh and v in self.coeffs:
            return self.coeffs.index(v)
        self.coeffs.append(v)
        return len(self.coeffs) - 1

    def wire(self):
        self.n_wires += 1
        return self.n_wires - 1

    def _expr(self, e):
        out = [len(e)]
        for c, w in e:
            out += [self.coeff(c), w]
        return out

    def _emit(self, bp, words, coff=0, woff=0):
        self.calldata += [len(words) + 1] + words
        self.blueprint.append(bp); self.constraint_off.append(coff); self.wire_off.append(woff)
        return len(self.blueprint) - 1

    def r1c(self, L, R_, O):
        words = [len(L), len(R_), len(O)]
        for e in (L, R_, O):
            for c, w in e:
                words += [self.coeff(c), w]
        self.n_constraints += 1
        return self._emit(1, words, self.n_constraints - 1, self.n_wires)

    def mul(self, L, R_, coeff=1, extra=()):
        """a producing constraint solved in O: L * R == extra + coeff * new -> the new wire"""
        w = self.wire()
        self.r1c(L, R_, list(extra) + [(coeff, w)])
        return w

    def _hint(self, hid, ins, nout):
        o0 = self.n_wires
        self.n_wires += nout
        words = [hid, len(ins)]
        for e in ins:
            words += self._expr(e)
        self._emit(0, words + [o0, o0 + nout], 0, o0)
        return list(range(o0, o0 + nout))

    def nbits(self, e, n):
        return self._hint(HINT_NBITS, [e], n)

    def randomize(self, n):
        return self._hint(HINT_RANDOMIZE, [], n)

    def commit(self, wires):
        self.has_commitment, self.commit_private, self.commit_wire = True, list(wires), self.n_wires
        return self._hint(HINT_BSB22, [[(1, CONST)]] + [[(1, w)] for w in wires], 1)[0]

    def table(self, values):
        assert len(values) == 256
        ent = []
        for v in values:
            ent += [1, self.coeff(v), CONST]
        self.bp_kind.append(BP_LOOKUP); self.bp_entries.append(ent)
        return len(self.bp_kind) - 1

    def lookup(self, table, exprs):
        o0 = self.n_wires
        self.n_wires += len(exprs)
        words = [256, len(exprs)]
        for e in exprs:
            words += self._expr(e)
        self._emit(table, words, 0, o0)
        return list(range(o0, o0 + len(exprs)))

    def count(self, rows, queries):
        """rows: (index, value) constants; queries: (index expression, value expression) -> one count wire per row"""
        ins = [[(len(rows), CONST)], [(2, CONST)]]
        for i, v in rows:
            ins += [[(i, CONST)], [(v, CONST)]]
        for qi, qv in queries:
            ins += [qi, qv]
        return self._hint(HINT_COUNT, ins, len(rows))

    def desc(self):
        return {"n_public": self.n_public, "n_secret": self.n_secret, "n_internal": self.n_wires - self.n_public - self.n_secret, "n_constraints": self.n_constraints,
                "calldata": list(self.calldata), "blueprint": list(self.blueprint), "constraint_off": list(self.constraint_off), "wire_off": list(self.wire_off),
                "bp_kind": list(self.bp_kind), "bp_entries": [list(e) for e in self.bp_entries], "coeff": [c * MONT % R for c in self.coeffs],
                "has_commitment": self.has_commitment, "commit_wire": self.commit_wire, "commit_private": list(self.commit_private)}


# ---- reading a description ----
def desc_coeffs(desc):
    return [c * MONT_INV % R for c in desc["coeff"]]


def instructions(desc):
    """-> per instruction a dict: kind ('r1c', 'nbits', 'count', 'randomize', 'commit', 'lookup') and its parts; expressions as (cid, wire) lists"""
    cd, out, q, i = desc["calldata"], [], 0, 0

    def expr(at):
        n = cd[at]
        return [(cd[at + 1 + 2 * k], cd[at + 2 + 2 * k]) for k in range(n)], at + 1 + 2 * n
    while q < len(cd):
        end = q + cd[q]
        kind = desc["bp_kind"][desc["blueprint"][i]]
        if kind == BP_R1C:
            n, at, sides = cd[q + 1:q + 4], q + 4, []
            for s in range(3):
                sides.append([(cd[at + 2 * k], cd[at + 2 * k + 1]) for k in range(n[s])]); at += 2 * n[s]
            assert at == end
            out.append({"kind": "r1c", "L": sides[0], "R": sides[1], "O": sides[2], "row": desc["constraint_off"][i]})
        elif kind == BP_HINT:
            hid, nin, at, ins = cd[q + 1], cd[q + 2], q + 3, []
            for _ in range(nin):
                e, at = expr(at); ins.append(e)
            o0, o1 = cd[at], cd[at + 1]
            assert at + 2 == end
            name = {HINT_NBITS: "nbits", HINT_COUNT: "count", HINT_RANDOMIZE: "randomize", HINT_BSB22: "commit"}[hid]
            out.append({"kind": name, "ins": ins, "o0": o0, "nout": o1 - o0})
        else:
            nent, nin, at, ins = cd[q + 1], cd[q + 2], q + 3, []
            for _ in range(nin):
                e, at = expr(at); ins.append(e)
            assert at == end
            out.append({"kind": "lookup", "ins": ins, "o0": desc["wire_off"][i], "nent": nent, "table": desc["bp_entries"][desc["blueprint"][i]]})
        q, i = end, i + 1
    return out


class Unsatisfied(Exception):
    pass


def solve_column(desc, ins, coef, inputs, mask=0, commit=0):
    """inputs: the values of wires 0 .. n_public + n_secret - 1 -> (W, A, B, C), or the index of the first failing instruction"""
    nw = desc["n_public"] + desc["n_secret"] + desc["n_internal"]
    W = list(inputs) + [None] * (nw - len(inputs))
    A, B, C = [None] * desc["n_constraints"], [None] * desc["n_constraints"], [None] * desc["n_constraints"]

    def ev(e):
        acc = 0
        for cid, w in e:
            acc += coef[cid] if w == CONST else coef[cid] * W[w]
        return acc % R
    for ii, it in enumerate(ins):
        try:
            k = it["kind"]
            if k == "r1c":
                acc, loc = [0, 0, 0], None
                for s, e in enumerate((it["L"], it["R"], it["O"])):
                    for cid, w in e:
                        if w == CONST:
                            acc[s] += coef[cid]
                        elif W[w] is None:
                            if loc:
                                raise Unsatisfied
                            loc = (s, w, cid)
                        else:
                            acc[s] += coef[cid] * W[w]
                a, b, c = (x % R for x in acc)
                if loc is None:
                    if a * b % R != c:
                        raise Unsatisfied
                else:
                    s, uw, uc = loc
                    wire = 0
                    if s == 2:
                        wire, c = (a * b - c) % R, a * b % R
                    else:
                        known, part = (b, a) if s == 0 else (a, b)
                        if known:
                            wire = (c * pow(known, -1, R) - part) % R
                            part = (part + wire) % R
                            a, b = (part, b) if s == 0 else (a, part)
                        elif a * b % R != c:
                            raise Unsatisfied
                    W[uw] = wire * pow(coef[uc], -1, R) % R
                A[it["row"]], B[it["row"]], C[it["row"]] = a, b, c
            elif k == "nbits":
                v = ev(it["ins"][0])
                for j in range(it["nout"]):
                    W[it["o0"] + j] = (v >> j) & 1 if j < 256 else 0
            elif k == "count":
                vals = [ev(e) for e in it["ins"]]
                nt, nv = vals[0], vals[1]
                if nv == 0 or nt != it["nout"] or len(vals) < 2 + nt * nv or (len(vals) - 2 - nt * nv) % nv:
                    raise Unsatisfied
                first = {}
                for t in range(nt):      # a query counts for the first table row it equals
                    first.setdefault(tuple(vals[2 + t * nv:2 + (t + 1) * nv]), t)
                cnt, bad = [0] * nt, False
                for qy in range((len(vals) - 2 - nt * nv) // nv):
                    qr = tuple(vals[2 + nt * nv + qy * nv:2 + nt * nv + (qy + 1) * nv])
                    if qr in first:
                        cnt[first[qr]] += 1
                    else:
                        bad = True
                for j in range(nt):
                    W[it["o0"] + j] = cnt[j]
                if bad:
                    raise Unsatisfied
            elif k == "randomize":
                for j in range(it["nout"]):
                    W[it["o0"] + j] = mask % R
            elif k == "commit":
                for j in range(it["nout"]):
                    W[it["o0"] + j] = commit % R
            else:
                for j, e in enumerate(it["ins"]):
                    v = ev(e)
                    if v >= it["nent"]:
                        raise Unsatisfied
                    at = 0
                    for _ in range(v):
                        at += 1 + 2 * it["table"][at]
                    ent = it["table"][at:at + 1 + 2 * it["table"][at]]
                    W[it["o0"] + j] = ev([(ent[1 + 2 * t], ent[2 + 2 * t]) for t in range(ent[0])])
        except Unsatisfied:
            return ii
    assert None not in W and None not in A
    return W, A, B, C


def solve(desc, columns, masks=None, commits=None):
    ins, coef = instructions(desc), desc_coeffs(desc)
    return [solve_column(desc, ins, coef, [1] + list(col), masks[p] if masks else 0, commits[p] if commits else 0) for p, col in enumerate(columns)]


def check(desc, W, A, B, C):
    """the independent checker of one satisfied column: raises AssertionError"""
    coef = desc_coeffs(desc)
    val = lambda e: sum(coef[cid] * (1 if w == CONST else W[w]) for cid, w in e) % R
    for it in instructions(desc):
        k = it["kind"]
        if k == "r1c":
            a, b, c = val(it["L"]), val(it["R"]), val(it["O"])
            assert a * b % R == c and (A[it["row"]], B[it["row"]], C[it["row"]]) == (a, b, c), it
        elif k == "nbits":
            bits, n = W[it["o0"]:it["o0"] + it["nout"]], it["nout"]
            assert all(b in (0, 1) for b in bits) and not any(bits[256:])
            assert sum(b << j for j, b in enumerate(bits[:256])) == val(it["ins"][0]) % (1 << min(n, 256))
        elif k == "lookup":
            for j, e in enumerate(it["ins"]):
                v = val(e)
                assert v < 256 and W[it["o0"] + j] == coef[it["table"][3 * v + 1]]
        elif k == "count":
            nt = it["nout"]
            assert sum(W[it["o0"]:it["o0"] + nt]) == (len(it["ins"]) - 2 - 2 * nt) // 2
            vals = [val(e) for e in it["ins"]]
            hits = {}
            for q in range(2 + 2 * nt, len(vals), 2):
                hits[vals[q], vals[q + 1]] = hits.get((vals[q], vals[q + 1]), 0) + 1
            rows = [(vals[2 + 2 * t], vals[3 + 2 * t]) for t in range(nt)]
            assert len(set(rows)) == nt and all(W[it["o0"] + t] == hits.get(rows[t], 0) for t in range(nt))


# ---- the device program's level schedule, restated ----
LONG_OP_WORDS = 48


def schedule(desc):
    """-> (order, levels): order[i] = the instruction at schedule index i; levels: per level (kind, [instructions], n_long)"""
    ins = instructions(desc)
    nw = desc["n_public"] + desc["n_secret"] + desc["n_internal"]
    level = [0] * (desc["n_public"] + desc["n_secret"]) + [None] * (nw - desc["n_public"] - desc["n_secret"])
    ops = []
    for ii, it in enumerate(ins):
        k, reads, makes = it["kind"], [], []
        if k == "r1c":
            words, unknown = 8, None
            for e in (it["L"], it["R"], it["O"]):
                for cid, w in e:
                    if w != CONST and level[w] is None and unknown is None:
                        unknown = w
                    else:
                        words += 2
                        reads.append(w)
            makes = [] if unknown is None else [unknown]
        else:
            exprs = it["ins"][2:] if k == "count" else [] if k in ("randomize", "commit") else it["ins"]
            reads = [w for e in exprs for _, w in e]
            words = {"nbits": 3, "count": 5, "lookup": 4, "randomize": 3, "commit": 3}[k] + sum(1 + 2 * len(e) for e in exprs)
            if k == "commit":
                reads = list(desc["commit_private"])
            makes = list(range(it["o0"], it["o0"] + (it["nout"] if k != "lookup" else len(it["ins"]))))
        lv = max([level[w] for w in reads if w != CONST] + [0])
        for w in makes:
            level[w] = lv + 1
        ops.append((lv, words, k))
    nlev = max(o[0] for o in ops) + 1 if ops else 0
    levels = []
    for l in range(nlev):
        gen = [i for i, o in enumerate(ops) if o[0] == l and o[2] not in ("count", "commit")]
        cnt = [i for i, o in enumerate(ops) if o[0] == l and o[2] == "count"]
        com = [i for i, o in enumerate(ops) if o[0] == l and o[2] == "commit"]
        for kind, group in ((0, gen), (1, cnt), (0, com)):
            if group:
                group = sorted(group, key=lambda i: -ops[i][1])      # stable: file order among equals
                nlong = 0 if kind else sum(1 for i in group if ops[i][1] > LONG_OP_WORDS)
                levels.append((kind, group, nlong))
    return [i for _, g, _ in levels for i in g], levels


# ---- the small-integer path ----
def small_flag(desc, classes, sol):
    """the misprediction word of one satisfied column: 1 when a wire predicted in {-1, 0, 1} (class <= 1) is not, a row predicted narrow is not, or
    an nBits input is negative as an integer (gnark's hint takes the bits of r + s)"""
    W, A, B, C = sol
    cw, ca, cb, cc = classes
    sgn = lambda v: v - R if v > HALF else v
    if any(cw[w] <= 1 and sgn(W[w]) not in (-1, 0, 1) for w in range(len(W))):
        return 1
    for rows, cl in ((A, ca), (B, cb), (C, cc)):
        if any(cl[i] <= 1 and sgn(rows[i]) not in (-1, 0, 1) for i in range(len(rows))):
            return 1
    coef = desc_coeffs(desc)
    for it in instructions(desc):
        if it["kind"] == "nbits" and sum(sgn(coef[cid]) * sgn(1 if w == CONST else W[w]) for cid, w in it["ins"][0]) < 0:
            return 1
    return 0


# ---- column patterns ----
EDGE = [0, 1, 2, R - 1, R - 2, HALF, P253]


def pattern_columns(name, n_in, batch, kinds):
    """one input vector per column.  kinds[j] says what input wire j + 1 holds over the columns:
       'bit'  0 / 1 in every column        'tern' -1 / 0 / 1          'mix'  columns alternate between 0, 1 and the edge / random values
       'wide' edge and random values       'nz'   like wide, never 0  or a list of values taken round-robin"""
    rng = random.Random("gsc-solver:" + name)
    cols = [[0] * n_in for _ in range(batch)]
    for j in range(n_in):
        k = kinds[j] if j < len(kinds) else kinds[-1]
        for p in range(batch):
            if isinstance(k, (list, tuple)):
                v = k[p % len(k)]
            elif k == "bit":
                v = rng.randrange(2)
            elif k == "tern":
                v = rng.choice([0, 1, R - 1])
            elif k == "mix":
                v = [0, 1, EDGE[(p // 3 + j) % len(EDGE)], rng.randrange(R)][(p + j) % 4]
            elif k == "nz":
                v = [1, 2, R - 1, R - 2, HALF, P253, rng.randrange(1, R)][(p + j) % 7]
            else:
                v = EDGE[(p + j) % len(EDGE)] if (p + j) % 3 else rng.randrange(R)
            cols[p][j] = v % R
    return cols


class Case:
    def __init__(self, name, build, batch=64, nproofs=0, workgroups=0, mode=0, classes=None, expect_flag=None, expect_fail=False, masks=False):
        self.name, self.build, self.batch, self.nproofs, self.workgroups, self.mode = name, build, batch, nproofs, workgroups, mode
        self.classes, self.expect_flag, self.expect_fail, self.masks = classes, expect_flag, expect_fail, masks

    @functools.lru_cache(maxsize=None)
    def made(self):
        c, cols = self.build(self.batch)
        desc = c.desc()
        rng = random.Random("gsc-solver-mask:" + self.name)
        masks = [rng.randrange(R) for _ in range(self.batch)] if self.masks else None
        commits = [rng.randrange(R) for _ in range(self.batch)] if self.masks else None
        return desc, cols, masks, commits

    @functools.lru_cache(maxsize=None)
    def reference(self):
        desc, cols, masks, commits = self.made()
        return solve(desc, cols, masks, commits)

    def ncols(self):
        return self.nproofs or self.batch

    def class_vectors(self):
        """mode 1: classes(circuit description, reference) -> (class_w, class_a, class_b, class_c)"""
        return self.classes(self.made()[0], self.reference())

    def call(self, gsc, fill=0xA5):
        desc, cols, masks, commits = self.made()
        n_in = desc["n_public"] + desc["n_secret"]
        in_W = b"".join(to_mont_bytes(1 if w == 0 else cols[p][w - 1]) for w in range(n_in) for p in range(self.batch))
        mb = b"".join(to_mont_bytes(v) for v in masks) if masks else None
        cb = b"".join(to_mont_bytes(v) for v in commits) if commits else None
        return gsc.debug_solve(desc, in_W, self.batch, self.nproofs, self.workgroups, self.mode, mb, cb, self.class_vectors() if self.mode == 1 else None, fill)


def classes_from_reference(desc, ref, wide_rows=()):
    """the calibration's answer on these columns: 0 = bit, 1 = also -1, 255 = wide; wide_rows: constraint rows predicted wide whatever they hold"""
    sat = [s for s in ref if not isinstance(s, int)]
    sgn = lambda v: v - R if v > HALF else v

    def cls(vals):
        vals = [sgn(v) for v in vals]
        return 0 if all(v in (0, 1) for v in vals) else 1 if all(v in (-1, 0, 1) for v in vals) else 255
    out = []
    for k in range(4):
        n = len(sat[0][k])
        out.append([cls([s[k][i] for s in sat]) for i in range(n)])
    for i in wide_rows:
        out[1][i] = out[2][i] = out[3][i] = 255
    return tuple(out)


# ---- circuits ----
def _terms(c, wires, n, coeffs=(1, 1, R - 1, 2, R - 2, 1, 7, 1)):
    """n terms over the given wires (and now and then the constant), coefficients mostly +-1"""
    out = []
    for k in range(n):
        w = wires[k % len(wires)] if k % 11 != 10 else CONST
        out.append((coeffs[k % len(coeffs)], w))
    return out


def circ_expr_len(n, kinds=("bit", "bit", "mix", "bit", "wide", "bit", "bit", "mix")):
    def build(batch):
        c = Circuit(2, 10)
        x = c.inputs()
        e = lambda shift: _terms(c, x[shift:] + x[:shift], n)
        y, z = [(1, x[0])], [(3, x[4]), (1, CONST)]
        # the expression as L, as R and as O of a producing constraint, then of a check over the same wires
        a = c.mul(e(0), z)
        c.r1c(e(0), z, [(1, a)])
        b = c.mul(y, e(1), coeff=R - 1)
        c.r1c(y, e(1), [(R - 1, b)])
        d = c.mul(y, z, coeff=5, extra=e(2))
        c.r1c(y, z, e(2) + [(5, d)])
        c.r1c(e(3), [(1, CONST)], e(3))                      # a check whose O is the expression itself
        return c, pattern_columns("expr_len_%d" % n, 12, batch, kinds)
    return build


def circ_window_straddle(k):
    """a short expression ahead of a long one, so that the long one's terms begin 49 + k words after the op's header"""
    def build(batch):
        c = Circuit(1, 11)
        x = c.inputs()
        off = 49 + k
        if off % 2:      # [hdr, loc, row, wire, coeff | nL, L .. | nR, R ..]: R's terms begin at 7 + 2 nL
            nl = (off - 7) // 2
            L, Rr, O = _terms(c, x, nl), _terms(c, x[3:] + x[:3], 40), []
            w = c.mul(L, Rr)
            c.r1c(L, Rr, [(1, w)])
        else:            # O's terms begin at 8 + 2 (nL + nR)
            nl = (off - 8) // 2 - 1
            L, Rr, O = _terms(c, x, nl), [(1, x[2])], _terms(c, x[5:] + x[:5], 40)
            w = c.mul(L, Rr, extra=O)
            c.r1c(L, Rr, O + [(1, w)])
        return c, pattern_columns("straddle_%d" % k, 12, batch, ("bit", "mix", "bit", "wide", "bit"))
    return build


def circ_coeff_ids(batch):
    c = Circuit(1, 5)
    b0, w0, b1, w1, m = c.inputs()[:5]
    g1, g2 = 0x123456789ABCDEF0123, R - 12345
    for cf in (0, 1, 2, R - 1, R - 2, g1, g2, HALF, P253):
        L = [(cf, b0), (cf, w0), (cf, CONST), (cf, m)]
        t = c.mul(L, [(1, CONST)])
        c.r1c([(1, t)], [(cf, b1), (1, CONST)], [(cf, c.mul([(1, t)], [(1, b1)])), (1, t)])
        c.r1c([(cf, w1), (cf, b1)], [(cf, CONST)], [(cf * cf, w1), (cf * cf, b1)])
    return c, pattern_columns("coeff_ids", 6, batch, ("bit", "wide", "bit", "wide", "mix"))


def circ_general_mixed(batch):
    c = Circuit(0, 12)
    x = c.inputs()
    for slow in (1, 2, 5, 8):
        e = [(0xABCDEF123 + 17 * k, x[k]) for k in range(slow)] + [(1, x[k]) for k in range(slow, 10)]
        t = c.mul(e, [(1, CONST)])
        c.r1c([(1, t)], [(2, CONST)], [(2 * cf, w) for cf, w in e])
    return c, pattern_columns("general_mixed", 12, batch, ("mix",))


def circ_long_op_split(batch):
    c = Circuit(1, 13)
    x = c.inputs()
    e130 = _terms(c, x, 130)
    y = [(1, x[1]), (1, CONST)]
    a = c.mul(e130, y)                                     # the long expression in L, in R, in O
    b = c.mul(y, e130, coeff=R - 1)
    d = c.mul(y, [(1, x[3])], extra=e130)
    c.r1c(e130, e130, [(1, c.mul(e130, e130))])
    bits = c.nbits(e130, 20)                                # a long nBits
    t = c.table([(7 * i + 3) % R for i in range(256)])
    byte = lambda j: [(1 << i, x[(i + j) % 8 + 4]) for i in range(8)]     # the input's bit wires 5 .. 12: a value below 256
    outs = c.lookup(t, [byte(j) for j in range(16)])        # a long lookup: only wave 0 works
    c.r1c([(1, a), (1, b), (1, d)], [(1, CONST)], [(1, a), (1, b), (1, d)])
    c.r1c([(1, outs[0]), (1, bits[0])], [(1, CONST)], [(1, outs[0]), (1, bits[0])])
    return c, pattern_columns("long_op_split", 14, batch, ("mix", "wide", "mix", "wide") + ("bit",) * 10)


def circ_level_mix(batch):
    c = Circuit(0, 12)
    x = c.inputs()
    for j in range(3):
        c.mul(_terms(c, x[j:] + x[:j], 60 + j), [(1, x[j])])
    for j in range(13):
        c.mul([(1, x[j % 12]), (j + 1, CONST)], [(1, x[(j + 5) % 12])], coeff=(1 if j % 2 else R - 1))
    return c, pattern_columns("level_mix", 12, batch, ("bit", "mix", "wide"))


def circ_ab_select(batch):
    c = Circuit(0, 6)
    bit_a, bit_b, wide_a, wide_b, mix_a, mix_b = c.inputs()
    for a, b in ((wide_a, bit_b), (bit_a, wide_b), (bit_a, bit_b), (mix_a, mix_b), (wide_a, wide_b), (mix_a, bit_b), (bit_a, mix_b)):
        t = c.mul([(1, a)], [(1, b)])
        c.r1c([(1, a)], [(1, b)], [(1, t)])
        c.r1c([(1, a), (1, CONST)], [(1, b), (R - 1, CONST)], [(1, t), (R - 1, a), (1, b), (R - 1, CONST)])
    return c, pattern_columns("ab_select", 6, batch, ("bit", "bit", "wide", "wide", "mix", "mix"))


def circ_solve_side(side):
    def build(batch):
        c = Circuit(0, 5)
        x, k, o, m, b = c.inputs()
        for uc in (1, R - 1, 0x1234567, HALF):
            w = c.wire()
            part = [(2, x), (1, CONST)]
            if side == "O":
                c.r1c([(1, x), (1, m)], [(1, k)], [(1, o), (uc, w)])
            elif side == "L":
                c.r1c(part + [(uc, w)], [(1, k)], [(1, o), (3, b)])
            else:
                c.r1c([(1, k)], part + [(uc, w)], [(1, o), (3, b)])
            c.r1c([(1, w)], [(1, w)], [(1, c.mul([(1, w)], [(1, w)]))])
        return c, pattern_columns("solve_" + side, 5, batch, ("wide", "nz", "wide", "mix", "bit"))
    return build


def circ_divide_known_zero(which, holds):
    """(part + w) * k == o with the known factor k zero in one lane, in half of them, in all: the wire stays 0 and the constraint must hold already"""
    def build(batch):
        c = Circuit(0, 4)
        x, k, o, y = c.inputs()
        w = c.wire()
        c.r1c([(1, x), (1, w)], [(1, k)], [(1, o)])
        w2 = c.wire()
        c.r1c([(1, k)], [(1, y), (R - 1, w2)], [(1, o)])
        c.r1c([(1, w), (1, w2)], [(1, CONST)], [(1, w), (1, w2)])      # neighbours read the solved wires
        cols = pattern_columns("divzero", 4, batch, ("wide", "nz", "wide", "wide"))
        zero = lambda p: p % 64 == 37 if which == "one_lane" else p % 2 == 0 if which == "half" else True
        for p in range(batch):
            if zero(p):
                cols[p][1] = 0
                # x * 0 == o holds only for o = 0; the failing variant breaks it in a few of the zero lanes (at most a quarter of the columns)
                cols[p][2] = 5 if not holds and (which == "one_lane" or p % 8 == 0) else 0
        return c, cols
    return build


def circ_divide_values(batch):
    c = Circuit(0, 3)
    x, k, o = c.inputs()
    for j in range(3):
        w = c.wire()
        c.r1c([(j + 1, x), (1, w)], [(1, k)], [(1, o), (j, CONST)])
        w2 = c.wire()
        c.r1c([(1, k)], [(R - 1, w2), (j, CONST)], [(1, o), (1, w)])
    return c, pattern_columns("divide_values", 3, batch, ("wide", [1, R - 1, P253, 0x1F2E3D4C5B6A79881726354, 2, HALF, R - 2], "wide"))


def circ_nbits(n):
    def build(batch):
        c = Circuit(0, 2)
        x, y = c.inputs()
        bits = c.nbits([(1, x)], n)
        b2 = c.nbits([(1, x), (1, y), (R - 1, y)], n)
        c.r1c([(1, bits[0]), (1, b2[n - 1])], [(1, CONST)], [(1, bits[0]), (1, b2[n - 1])])
        vals = [0, 1, (1 << n) - 1, 1 << n, R - 1, (1 << n) + 5, HALF, P253, (1 << (n - 1)), R - 2]
        return c, pattern_columns("nbits_%d" % n, 2, batch, ([v % R for v in vals], "wide"))
    return build


def circ_lookup(batch):
    c = Circuit(0, 3)
    v, w, b = c.inputs()
    t1 = c.table([(i * i + 1) % R for i in range(256)])
    t2 = c.table([R - 1 - i for i in range(256)])
    o1 = c.lookup(t1, [[(1, v)], [(1, w), (1, b)]])
    o2 = c.lookup(t2, [[(1, w)], [(255, b)], [(1, w), (1, b)]])      # (v is read by one op only: a refused value fails one instruction)
    c.r1c([(1, o1[0]), (1, o2[2])], [(1, o1[1])], [(1, c.mul([(1, o1[0]), (1, o2[2])], [(1, o1[1])]))])
    cols = pattern_columns("lookup", 3, batch, ([0, 255, 17, 128], [254, 0, 3], "bit"))
    for p, bad in ((5, 256), (21, R - 1), (40, 1 << 32), (63, 257)):      # refused values in chosen lanes
        for q in range(p, batch, 64):
            cols[q][0] = bad
    return c, cols


def circ_count(nrows, nq, how="spread"):
    def build(batch):
        c = Circuit(0, 4)
        i0, v0, i1, v1 = c.inputs()
        rows = [(i, (5 * i + 2) % R) for i in range(nrows)]
        bits = c.nbits([(1, i1)], 8)                      # a generic level ahead of the count level, another behind it
        qs = []
        for k in range(nq):
            if how == "one_row" or k % 3 == 0:
                qs.append(([(1, i0)], [(1, v0)]))
            elif k % 3 == 1:
                qs.append(([(1 << j, b) for j, b in enumerate(bits)], [(1, v1)]))
            else:
                qs.append(([(k % nrows, CONST)], [((5 * (k % nrows) + 2) % R, CONST)]))
        outs = c.count(rows, qs)
        c.r1c([(1, w) for w in outs], [(1, CONST)], [(nq, CONST)])
        cols = []
        for p in range(batch):
            a, b = (p * 7) % nrows, (p * 3 + 1) % nrows
            cols.append([a, 5 * a + 2, b, 5 * b + 2])
        if how == "bad" and nq:
            for p, (idx, val) in ((3, (nrows, 5 * nrows + 2)), (17, (R - 1, 2)), (30, (0, 3)), (44, (nrows - 1, 5 * nrows + 2))):
                for q in range(p, batch, 64):
                    cols[q][0], cols[q][1] = idx % R, val % R
        return c, cols
    return build


def circ_randomize_commit(nout):
    def build(batch):
        c = Circuit(1, 3)
        pub, x, y, z = c.inputs()
        r = c.randomize(nout)
        t = c.mul([(1, r[0]), (1, x)], [(1, r[nout - 1]), (1, y)])
        cw = c.commit([x, y, t])
        u = c.mul([(1, cw), (1, z)], [(1, t), (1, pub)])           # a constraint reading the committed wire, after it
        c.r1c([(1, u)], [(1, CONST)], [(1, u)])
        return c, pattern_columns("randomize_commit", 4, batch, ("wide", "mix", "bit", "wide"))
    return build


def circ_status(batch):
    """two failing checks in different levels and one failing lookup: columns fail at different ones (and one at two, the earlier of which counts)"""
    c = Circuit(0, 5)
    x, y, e1, e2, v = c.inputs()
    t = c.table(list(range(256)))
    a = c.mul([(1, x)], [(1, y)])
    c.r1c([(1, x)], [(1, y)], [(1, e1)])                  # check 1 (level 0): e1 == x y
    b = c.mul([(1, a)], [(1, x)])
    lo = c.lookup(t, [[(1, v)]])
    c.r1c([(1, b)], [(1, CONST)], [(1, e2)])              # check 2 (level 2): e2 == x x y
    c.r1c([(1, lo[0])], [(1, CONST)], [(1, v)])
    cols = pattern_columns("status", 5, batch, ("wide", "wide", "bit", "bit", [3, 200, 255, 0]))
    for p in range(batch):
        xx, yy = cols[p][0], cols[p][1]
        cols[p][2], cols[p][3] = xx * yy % R, xx * xx * yy % R
        q = p % 64
        if q in (4, 33):
            cols[p][2] = (cols[p][2] + 1) % R
        if q in (9, 33, 50):
            cols[p][3] = (cols[p][3] + 1) % R
        if q in (12, 61):
            cols[p][4] = 256 + q
    return c, cols


def circ_depth(depth):
    def build(batch):
        c = Circuit(0, 3)
        x, y, z = c.inputs()
        a, b = x, y
        for l in range(depth):
            a, b = c.mul([(1, a), (1, z)], [(1, b)]), c.mul([(1, b), (l + 1, CONST)], [(1, a)], coeff=R - 1)
        return c, pattern_columns("depth", 3, batch, ("wide", "mix", "bit"))
    return build


def circ_few_terms(T, cut):
    """one op of T = nL + nR + nO terms: the cuts between L, R and O on, before and after lanes 63 / 64 and terms 191 / 192 (cut = -1, 0, 1)"""
    def build(batch):
        c = Circuit(0, 14)
        x = c.inputs()
        if T == 0:
            c.r1c([], [], [])
            return c, pattern_columns("few_terms_0", 14, batch, ("mix",))
        n_l = max(0, min(T - 1, (T // 2 if T <= 7 else 63 if T <= 64 else 64) + cut))
        n_o = 0 if T <= 64 else max(0, min(T - n_l - 1, T - 192 + cut if T > 192 else (T - n_l) // 2))
        n_r = T - n_l - n_o - 1
        L, Rr, O = _terms(c, x, n_l), _terms(c, x[4:] + x[:4], n_r), _terms(c, x[9:] + x[:9], n_o)
        w = c.mul(L, Rr, extra=O)                          # the solved wire's term is not in the op: T - 1 terms there ...
        c.r1c(L, Rr, O + [(1, w)])                         # ... and T here
        return c, pattern_columns("few_terms_%d" % T, 14, batch, ("bit", "mix", "bit", "wide", "bit", "bit", "mix"))
    return build


def circ_few_6_7(batch):
    c = Circuit(0, 9)
    x = c.inputs()
    for n in (5, 6, 7, 8):      # read lane by lane up to 6 terms, the butterfly from 7
        for sides in ((n, 1, 1), (1, n, 1), (1, 1, n), (n, 1, n), (n, n, n)):
            L, Rr, O = (_terms(c, x[j:] + x[:j], m) for j, m in enumerate(sides))
            w = c.mul(L, Rr, extra=O)
            c.r1c(L, Rr, O + [(1, w)])
    return c, pattern_columns("few_6_7", 9, batch, ("mix", "bit", "wide"))


def circ_few_long_sides(batch):
    c = Circuit(0, 12)
    x = c.inputs()
    for sides in ((96, 1, 33), (96, 1, 1), (1, 70, 1), (40, 30, 20), (64, 64, 64), (1, 1, 100)):
        L, Rr, O = (_terms(c, x[j:] + x[:j], m) for j, m in enumerate(sides))
        w = c.mul(L, Rr, extra=O)
        c.r1c(L, Rr, O + [(1, w)])
    return c, pattern_columns("few_long_sides", 12, batch, ("bit", "mix", "bit", "bit", "wide"))


def circ_few_hard_lanes(batch):
    """general coefficients on wide values at chosen term positions: a product needed in slot 0, in slot 2, in two slots, in none"""
    c = Circuit(0, 8)
    x = c.inputs()
    g = 0x55AA55AA55AA1
    for hard in ((3,), (130,), (3, 70, 130), (), (0, 63, 64, 127, 128, 191)):
        L = [((g + k) if k in hard else 1, x[0] if k in hard else x[1 + k % 3]) for k in range(192)]
        w = c.mul(L, [(1, x[4])])
        c.r1c(L, [(1, x[4])], [(1, w)])
    return c, pattern_columns("few_hard", 8, batch, ("wide", "bit", "bit", "bit", "mix"))


def circ_few_deferred(batch):
    """checks (loc = 0) in early levels, one of them failing in one column; the last level is a count level"""
    c = Circuit(0, 4)
    x, y, e, i0 = c.inputs()
    a = c.mul([(1, x)], [(1, y)])
    c.r1c([(1, x)], [(1, y)], [(1, e)])                   # deferred; fails where e != x y
    b = c.mul([(1, a)], [(1, a)])
    c.r1c([(1, a)], [(1, a)], [(1, b)])                   # deferred
    d = c.mul([(1, b)], [(1, x)])
    bits = c.nbits([(1, i0), (1, d), (R - 1, d)], 2)      # (reads the deepest wire: the count level is the last one)
    c.count([(i, i + 10) for i in range(4)], [([(1, bits[0]), (2, bits[1])], [(1, bits[0]), (2, bits[1]), (10, CONST)]), ([(1, i0)], [(1, i0), (10, CONST)])])
    cols = pattern_columns("few_deferred", 4, batch, ("wide", "wide", "bit", [0, 1, 2, 3]))
    for p in range(batch):
        cols[p][2] = cols[p][0] * cols[p][1] % R
    cols[1][2] = (cols[1][2] + 1) % R
    return c, cols


def circ_few_last_op(batch):
    """the op whose terms end the term list: nothing but the pad behind them"""
    c = Circuit(0, 6)
    x = c.inputs()
    a = c.mul([(1, x[0])], [(1, x[1])])
    L = _terms(c, x + [a], 191)
    c.mul(L, [(1, x[2])], extra=[(1, a)])
    return c, pattern_columns("few_last_op", 6, batch, ("mix", "wide", "bit"))


# small-integer circuits: every wire in {-1, 0, 1}
def circ_small_levels(width):
    """helper products, then ONE level of `width` producing constraints out = +-(L R - O) with one and two terms per side and coefficients
    1, -1, 2^27, then a level reading them; every wire stays in {-1, 0, 1}"""
    def build(batch):
        c = Circuit(1, 7)
        x = c.inputs()
        n = len(x)
        h = {}
        for j in range(n):      # level 0: the products the two-term forms subtract again
            a, b, d = x[j], x[(j + 1) % n], x[(j + 2) % n]
            h[j] = (c.mul([(1, a)], [(1, b)]), c.mul([(1, d)], [(1, b)]), c.mul([(1, a)], [(1, d)]))
        cur = []
        for k in range(width):
            j = k % n
            a, b, d = x[j], x[(j + 1) % n], x[(j + 2) % n]
            ab, db, ad = h[j]
            form = k % 5
            if form == 0:        # (every form reads a helper, so that the level holds exactly `width` items)
                cur.append(c.mul([(1, ab)], [(1, d)]))
            elif form == 1:
                cur.append(c.mul([(1, db)], [(1, a)], coeff=R - 1))
            elif form == 2:      # (a + d) b - d b
                cur.append(c.mul([(1, a), (1, d)], [(1, b)], extra=[(1, db)]))
            elif form == 3:      # a (b + d) - a d, negated
                cur.append(c.mul([(1, a)], [(1, b), (1, d)], coeff=R - 1, extra=[(1, ad)]))
            else:                # 2^27 a b - (2^27 - 1) a b
                cur.append(c.mul([(1 << 27, a)], [(1, b)], extra=[((1 << 27) - 1, ab)]))
        for k in range(min(width, 3)):
            w = c.mul([(1, cur[k])], [(1, cur[(k + 1) % len(cur)])])
            c.r1c([(1, w)], [(1, w)], [(1, c.mul([(1, w)], [(1, w)]))])
        return c, pattern_columns("small_levels_%d" % width, 8, batch, ("tern", "bit", "tern"))
    return build


def circ_small_nbits(nout, nterms, n_sums=1):
    def build(batch):
        c = Circuit(0, 12)
        x = c.inputs()
        outs = []
        for s in range(n_sums):
            # a sum of nterms bit-valued terms with coefficients 2^k kept below 2^nout ... wide enough to fill nout bits
            e = [(1 << ((k + s) % min(nout, 52)), x[(k + s) % 12]) for k in range(nterms)]
            outs.append(c.nbits(e, nout))
        c.r1c([(1, outs[0][0])], [(1, outs[-1][nout - 1])], [(1, c.mul([(1, outs[0][0])], [(1, outs[-1][nout - 1])]))])
        return c, pattern_columns("small_nbits_%d_%d" % (nout, nterms), 12, batch, ("bit",))
    return build


def circ_small_rows(batch):
    """check rows of 130 terms (an add32-style sum against its bits), predicted wide or narrow by the case"""
    c = Circuit(0, 12)
    x = c.inputs()
    e = [(1 << (k % 10), x[k % 12]) for k in range(96)]
    bits = c.nbits(e, 20)
    c.r1c(e + [(0, x[0])] * 1, [(1, CONST)], [(1 << j, b) for j, b in enumerate(bits)] + [(0, x[1])] * 13)      # 97 + 1 + 33 terms, the row is wide
    z = c.mul([(1, x[0])], [(1, x[1])])
    c.r1c([(1, x[k % 12]) for k in range(64)] + [(R - 1, x[k % 12]) for k in range(64)] + [(1, z), (1, CONST)], [(1, CONST)], [(1, z), (1, CONST)])      # 130 terms, the row is 0 / 1 / 2
    return c, pattern_columns("small_rows", 12, batch, ("bit",))


def circ_small_refusal(what):
    def build(batch):
        c = Circuit(0, 3)
        x, y, z = c.inputs()
        if what == "division":
            w = c.wire(); c.r1c([(1, w)], [(1, x)], [(1, y)])
        elif what == "lookup":
            c.lookup(c.table([i % 2 for i in range(256)]), [[(1, x)]])
        elif what == "coefficient 2":
            c.mul([(1, x)], [(1, y)], coeff=2)
        else:
            c.nbits([(1, x), (2, y)], 63)
        return c, pattern_columns("small_refusal", 3, batch, ([1], [1], [1]))
    return build


def circ_small_mispredict(what):
    """the calibration saw {-1, 0, 1} everywhere; one column then holds an input wire of 2, solves a wire to 2, has a narrow row of 2, or a negative nBits sum"""
    def build(batch):
        c = Circuit(0, 5)
        x, y, z, u, v = c.inputs()
        c.mul([(1, x), (1, y)], [(1, z)])                                     # (x + y) z
        c.r1c([(1, x), (1, u)], [(1, CONST)], [(1, x), (1, u)])               # a row of value x + u
        c.nbits([(1, x), (R - 1, v), (R - 1, v)], 3)                          # x - 2 v
        cols = [[p % 2, 0, 1, 0, 0] for p in range(batch)]
        p = 37 % batch
        if what == "input":
            cols[p] = [2, 0, 0, 0, 0]
        elif what == "solved":
            cols[p] = [1, 1, 1, 0, 0]
        elif what == "row":
            cols[p] = [1, 0, 1, 1, 0]
        else:
            cols[p] = [0, 0, 1, 0, 1]
        return c, cols
    return build


def circ_small_unsat(batch):
    c = Circuit(0, 3)
    x, y, e = c.inputs()
    a = c.mul([(1, x)], [(1, y)])
    c.r1c([(1, x)], [(1, y)], [(1, e)])
    c.r1c([(1, a)] + [(1, x), (R - 1, x)] * 5, [(1, CONST)], [(1, e)])
    cols = pattern_columns("small_unsat", 3, batch, ("bit", "tern", "bit"))
    for p in range(batch):
        cols[p][2] = cols[p][0] * cols[p][1] % R
    for p in (6, 41):
        cols[p][2] = (cols[p][2] + 1) % R if cols[p][2] != 1 else 0
    return c, cols


def _predict_narrow_everything(desc, ref):
    cw, ca, cb, cc = classes_from_reference(desc, ref)
    return cw, [0] * len(ca), [0] * len(cb), [0] * len(cc)


def _predict_inputs_only(desc, ref):
    """the calibration saw {-1, 0, 1} everywhere (it never met the column that breaks it)"""
    n_w = desc["n_public"] + desc["n_secret"] + desc["n_internal"]
    return [1] * n_w, [1] * desc["n_constraints"], [1] * desc["n_constraints"], [1] * desc["n_constraints"]


@functools.lru_cache(maxsize=None)
def case_table():
    t = []
    add = lambda *a, **k: t.append(Case(*a, **k))
    # ---- generic batch ----
    for n in (0, 1, 7, 8, 9, 16, 17, 33, 130):
        add("expr_len_%d" % n, circ_expr_len(n))
    add("expr_len_9_b2112", circ_expr_len(9), batch=2112)
    for k in range(16):
        add("expr_window_straddle_%d" % k, circ_window_straddle(k))
    add("coeff_ids", circ_coeff_ids)
    add("general_coeff_mixed_lanes", circ_general_mixed)
    add("long_op_split", circ_long_op_split)
    add("level_mix", circ_level_mix)
    add("ab_select", circ_ab_select)
    for s in "OLR":
        add("solve_" + s, circ_solve_side(s))
    for which in ("one_lane", "half", "all"):
        add("divide_known_zero_%s_holds" % which, circ_divide_known_zero(which, True))
        add("divide_known_zero_%s_fails" % which, circ_divide_known_zero(which, False), expect_fail=True)
    add("divide_values", circ_divide_values)
    for n in (1, 8, 62, 64, 65, 254, 256, 300):
        add("nbits_%d" % n, circ_nbits(n))
    add("lookup", circ_lookup, expect_fail=True)
    for nrows, nq in ((1, 1), (2, 7), (255, 8), (256, 9), (256, 0), (256, 1025)):
        add("count_%d_rows_%d_queries" % (nrows, nq), circ_count(nrows, nq))
    add("count_one_row", circ_count(256, 9, "one_row"))
    add("count_bad_queries", circ_count(255, 8, "bad"), expect_fail=True)
    add("randomize_commit_1", circ_randomize_commit(1), masks=True)
    add("randomize_commit_70", circ_randomize_commit(70), masks=True)
    add("status_first_failure", circ_status, expect_fail=True)
    add("depth_40", circ_depth(40))
    # ---- resident path ----
    few = [("expr_len_17", circ_expr_len(17), {}), ("expr_len_130", circ_expr_len(130), {}), ("coeff_ids", circ_coeff_ids, {}), ("general_coeff_mixed_lanes", circ_general_mixed, {}),
           ("long_op_split", circ_long_op_split, {}), ("ab_select", circ_ab_select, {}), ("solve_L", circ_solve_side("L"), {}), ("solve_R", circ_solve_side("R"), {}),
           ("solve_O", circ_solve_side("O"), {}), ("divide_known_zero_half_holds", circ_divide_known_zero("half", True), {}),
           ("divide_known_zero_half_fails", circ_divide_known_zero("half", False), {"expect_fail": True}), ("divide_values", circ_divide_values, {}),
           ("nbits_65", circ_nbits(65), {}), ("nbits_300", circ_nbits(300), {}), ("lookup", circ_lookup, {"expect_fail": True}),
           ("count_256_rows_1025_queries", circ_count(256, 1025), {}), ("count_2_rows_7_queries", circ_count(2, 7), {}), ("count_bad_queries", circ_count(255, 8, "bad"), {"expect_fail": True}),
           ("randomize_commit_70", circ_randomize_commit(70), {"masks": True}), ("status_first_failure", circ_status, {"expect_fail": True}),
           ("few_6_7", circ_few_6_7, {}), ("few_long_sides", circ_few_long_sides, {}), ("few_hard_lanes", circ_few_hard_lanes, {}),
           ("few_deferred_check", circ_few_deferred, {"expect_fail": True}), ("few_last_op_terms", circ_few_last_op, {})]
    shapes = [(1, 1), (2, 17), (3, 0), (32, 0), (32, 17), (2, 0)]
    for i, (name, build, kw) in enumerate(few):
        # (a case that expects failures needs them among its first nproofs columns, and in no more than a quarter of those)
        for np_, wg in ((32, 0), (32, 17)) if kw.get("expect_fail") else (shapes[i % len(shapes)], shapes[(i + 3) % len(shapes)]):
            add("few_p%d_wg%d_%s" % (np_, wg, name), build, nproofs=np_, workgroups=wg, **kw)
    for T in (0, 6, 7, 64, 65, 191, 192, 193, 400):
        for cut in (-1, 0, 1):
            np_, wg = shapes[(T + cut) % len(shapes)]
            add("few_terms_%d_cut%+d_p%d_wg%d" % (T, cut, np_, wg), circ_few_terms(T, cut), nproofs=np_, workgroups=wg)
    for wg in (1, 17):
        add("few_depth_40_wg%d" % wg, circ_depth(40), nproofs=3, workgroups=wg)
    # ---- small-integer path ----
    for width in (1, 8, 9, 128, 129):
        add("small_levels_%d" % width, circ_small_levels(width), mode=1, classes=classes_from_reference, expect_flag=0)
    for nout, nterms in ((1, 1), (9, 32), (10, 33), (62, 130)):
        add("small_nbits_%d_from_%d" % (nout, nterms), circ_small_nbits(nout, nterms), mode=1, classes=classes_from_reference, expect_flag=0)
    add("small_nbits_17_sums", circ_small_nbits(9, 40, 17), mode=1, classes=classes_from_reference, expect_flag=0)
    add("small_rows_wide", circ_small_rows, mode=1, classes=classes_from_reference, expect_flag=0)
    add("small_rows_predicted_narrow", circ_small_rows, mode=1, classes=_predict_narrow_everything, expect_flag=1)
    for what in ("input", "solved", "row", "negative"):
        add("small_mispredict_" + what, circ_small_mispredict(what), mode=1, classes=_predict_inputs_only, expect_flag=1)
    add("small_unsatisfied", circ_small_unsat, mode=1, classes=classes_from_reference, expect_flag=0, expect_fail=True)
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return {c.name: c for c in t}


def small_refusals():
    return {"division": (circ_small_refusal("division"), "divides"), "lookup": (circ_small_refusal("lookup"), "other than a constraint or an nBits hint"),
            "coefficient 2": (circ_small_refusal("coefficient 2"), "coefficient other than +-1"), "63 outputs": (circ_small_refusal("63 outputs"), "more than 62 outputs")}


def malformed_descriptions():
    """the refusal list: name -> (description, the builder's message, or None when the hook's tables or the device refuse it)"""
    out = {}
    c = Circuit(0, 2); w = c.wire(); c.nbits([(1, w)], 2); c.r1c([(1, w)], [(1, CONST)], [(1, 1)])
    out["a read of an unsolved wire"] = (c.desc(), "solver: instruction reads an unsolved wire")
    c = Circuit(0, 2); w1, w2 = c.wire(), c.wire(); c.r1c([(1, w1)], [(1, w2)], [(1, 1)])
    out["two unknowns in a constraint"] = (c.desc(), "solver: more than one wire to instantiate")
    c = Circuit(0, 2); t = c.table(list(range(256))); c.lookup(t, [[(1, 1)]]); d = c.desc(); d["bp_entries"][t] = d["bp_entries"][t][:255 * 3]
    out["a lookup blueprint without 256 entries"] = (d, "solver: lookup table is not 256 constant entries")
    c = Circuit(0, 2); c._hint(HINT_COUNT, [[(2, CONST)], [(2, CONST)], [(0, CONST)], [(5, CONST)], [(1, 1)], [(6, CONST)], [(1, 2)], [(5, CONST)]], 2)
    out["a non-constant count table row"] = (c.desc(), "solver: countHint table rows must be constants")
    c = Circuit(0, 2); c.mul([(1, 1)], [(1, 2)]); d = c.desc(); d["coeff"][2] = 3 * MONT % R
    out["coefficient ids 0..4 wrong"] = (d, None)
    c = Circuit(0, 2); c.count([(i + 1, i) for i in range(3)], [([(1, 1)], [(1, 2)])])
    out["an index column that is not 0..n-1"] = (c.desc(), None)
    return out


def case_names(mode=None, resident=None):
    return [n for n, c in case_table().items() if (mode is None or c.mode == mode) and (resident is None or bool(c.nproofs) == resident)]
