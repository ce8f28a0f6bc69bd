"""tests/solver_model.py on a CPU, before tests/test_gpu_solver.py trusts it on the device:

 1. the independent checker passes on every satisfied column of every case, and at most a quarter of a case's columns are unsatisfied;
 2. the Python reference reproduces the ORACLE's W, A, B, C on the shipped ChaCha20-V3 and AES-128 circuits (and the KAT hashes), from the
    description tests/native/solver_desc_dump.cpp writes for gnark's R1CS files: all six instruction kinds pinned to gnark through the oracle;
 3. build_solver_program, build_few_program and build_small_program (csrc/formats.cpp, csrc/wit_small.cpp) run on every case's description in that
    harness; the three layouts they emit — the word stream level by level, the 8-word descriptors with their term lists, the small program's
    items — are replayed here with plain integers, one column at a time, and every wire and row is held against the reference: a builder bug shows
    here, a kernel bug in the GPU test;
 4. the malformed descriptions of the GPU test's refusal list go through the builders in the same program compiled with
    -fsanitize=address,undefined: each throws its message and nothing else."""
import hashlib
import os
import struct
import subprocess

import pytest

import solver_model as M
from conftest import ROOT, KAT, golden_bytes

CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")
R = M.R
SOURCES = [os.path.join(ROOT, "tests", "native", "solver_desc_dump.cpp"), os.path.join(CSRC, "wit_small.cpp"), os.path.join(CSRC, "formats.cpp")]


def _compile(name, extra):
    exe = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe] + extra + SOURCES)
    return exe


@pytest.fixture(scope="module")
def harness():
    return _compile("solver_desc_dump", ["-O2"])


@pytest.fixture(scope="module")
def harness_san():
    return _compile("solver_desc_dump_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---- the harness's files ----
def _vec(v):
    return struct.pack("<I", len(v)) + struct.pack("<%dI" % len(v), *v)


def desc_words(desc, classes=None):
    coef = M.desc_coeffs(desc)
    small = [c if c < (1 << 62) else c - R if R - c < (1 << 62) else None for c in coef]
    out = struct.pack("<6I", desc["n_public"], desc["n_secret"], desc["n_internal"], desc["n_constraints"], 1 if desc["has_commitment"] else 0, desc["commit_wire"])
    out += _vec(desc["calldata"]) + _vec(desc["blueprint"]) + _vec(desc["constraint_off"]) + _vec(desc["wire_off"])
    out += _vec(desc["bp_kind"]) + _vec([len(e) for e in desc["bp_entries"]]) + _vec([w for e in desc["bp_entries"] for w in e])
    out += _vec([(c >> (32 * k)) & 0xFFFFFFFF for c in desc["coeff"] for k in range(8)]) + _vec(desc["commit_private"])
    nw = desc["n_public"] + desc["n_secret"] + desc["n_internal"]
    cw, ca, cb, cc = classes or ([255] * nw, [255] * desc["n_constraints"], [255] * desc["n_constraints"], [255] * desc["n_constraints"])
    out += _vec(cw) + _vec(ca) + _vec(cb) + _vec(cc) + _vec([0 if s is None else 1 for s in small])
    out += _vec([(s or 0) & 0xFFFFFFFF for s in small]) + _vec([((s or 0) >> 32) & 0xFFFFFFFF for s in small])
    return out


class Words:
    def __init__(self, b):
        self.w, self.i = struct.unpack("<%dI" % (len(b) // 4), b), 0

    def u(self):
        self.i += 1
        return self.w[self.i - 1]

    def vec(self):
        n = self.u()
        self.i += n
        return list(self.w[self.i - n:self.i])

    def vec64(self):
        n = self.u()
        self.i += 2 * n
        v = self.w[self.i - 2 * n:self.i]
        return [(lambda x: x - (1 << 64) if x >> 63 else x)(v[2 * k] | (v[2 * k + 1] << 32)) for k in range(n)]


def read_desc(b):
    w = Words(b)
    d = dict(zip(("n_public", "n_secret", "n_internal", "n_constraints"), (w.u(), w.u(), w.u(), w.u())))
    d["has_commitment"], d["commit_wire"] = bool(w.u()), w.u()
    for k in ("calldata", "blueprint", "constraint_off", "wire_off", "bp_kind"):
        d[k] = w.vec()
    lens, flat, limbs = w.vec(), w.vec(), w.vec()
    d["bp_entries"], at = [], 0
    for n in lens:
        d["bp_entries"].append(flat[at:at + n]); at += n
    d["coeff"] = [sum(limbs[8 * i + k] << (32 * k) for k in range(8)) for i in range(len(limbs) // 8)]
    d["commit_private"] = w.vec()
    return d


def build_layouts(harness, tmp_path, desc, classes=None):
    """-> (return code, stdout, layouts or None)"""
    src, dst = tmp_path / "desc.bin", tmp_path / "layouts.bin"
    src.write_bytes(desc_words(desc, classes))
    out = subprocess.run([harness, "build", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    if out.returncode:
        return out.returncode, out.stdout + out.stderr, None
    w = Words(dst.read_bytes())
    L = dict(zip(("n_levels", "commit_level", "n_ops", "n_inversions", "n_tables"), (w.u(), w.u(), w.u(), w.u(), w.u())))
    for k in ("words", "lookup_coeff", "sched", "level_kind", "level_long", "count_ops", "few_ops", "few_terms", "few_level_start", "few_count_ops", "few_count_qoff", "few_count_first"):
        L[k] = w.vec()
    for k in ("small_ok", "rows_per_group", "scratch_row", "small_levels", "max_slots", "n_rtiny", "n_rgen"):
        L[k] = w.u()
    for k in ("levels", "tiny", "parts", "bits", "twire"):
        L[k] = w.vec()
    L["tcoef"] = w.vec64()
    for k in ("rtiny", "rgen", "rtwire"):
        L[k] = w.vec()
    L["rtcoef"] = w.vec64()
    for k in ("cls_a", "cls_b", "cls_c"):
        L[k] = w.vec()
    assert w.i == len(w.w)
    return 0, out.stdout, L


# ---- integer replays of the three layouts (the op semantics: csrc/formats.hpp) ----
OP_R1C, OP_NBITS, OP_COUNT, OP_LOOKUP, OP_RANDOMIZE, OP_COMMIT = 1, 2, 3, 4, 5, 6


class Replay:
    def __init__(self, desc, L, inputs, mask, commit):
        self.coef, self.L = M.desc_coeffs(desc), L
        nw = desc["n_public"] + desc["n_secret"] + desc["n_internal"]
        self.W = [1] + list(inputs) + [None] * (nw - 1 - len(inputs))
        self.A, self.B, self.C = ([None] * desc["n_constraints"] for _ in range(3))
        self.mask, self.commit, self.status = mask, commit, None

    def fail(self, i):
        self.status = i if self.status is None else min(self.status, i)

    def term(self, cid, wid):
        return self.coef[cid] * (1 if wid == M.CONST else self.W[wid])

    def expr(self, q):
        w, n = self.L["words"], self.L["words"][q]
        return sum(self.term(w[q + 1 + 2 * k], w[q + 2 + 2 * k]) for k in range(n)) % R, q + 1 + 2 * n

    def r1c(self, i, loc, row, uw, uc, a, b, c):
        if loc == 0:
            if a * b % R != c:
                self.fail(i)
        else:
            wire = 0
            if loc == 3:
                wire, c = (a * b - c) % R, a * b % R
            else:
                known, part = (b, a) if loc == 1 else (a, b)
                if known:
                    wire = (c * pow(known, -1, R) - part) % R
                    part = (part + wire) % R
                elif a * b % R != c:
                    self.fail(i)
                a, b = (part, b) if loc == 1 else (a, part)
            self.W[uw] = wire * pow(self.coef[uc], -1, R) % R
        self.A[row], self.B[row], self.C[row] = a, b, c

    def lookup(self, i, out, table, v):
        if v >= 256:
            self.fail(i)
        self.W[out] = self.coef[self.L["lookup_coeff"][256 * table + (v & 255)]]

    def count(self, i, at):
        w = self.L["words"]
        o0, ntab, nq = w[at + 1], w[at + 2], w[at + 4]
        cnt, q = [0] * ntab, at + 5 + 6 * ntab
        for _ in range(nq):
            x0, q = self.expr(q)
            x1, q = self.expr(q)
            if x0 < ntab and x1 == self.coef[w[at + 5 + 6 * x0 + 4]]:
                cnt[x0] += 1
            else:
                self.fail(i)
        self.W[o0:o0 + ntab] = cnt

    def words(self):
        """the word stream, level by level, as k_solver / k_solver_count walk it; status: the schedule index"""
        w, sched = self.L["words"], self.L["sched"]
        nlev = sched[0]
        lstart, ops = sched[1:nlev + 2], sched[nlev + 2:]
        for lev in range(nlev):
            done = []
            for i in range(lstart[lev], lstart[lev + 1]):
                at = ops[i]
                op, nwords = w[at] & 0xFF, w[at] >> 8
                assert (op == OP_COUNT) == bool(self.L["level_kind"][lev])
                assert (nwords > M.LONG_OP_WORDS and not self.L["level_kind"][lev]) == (i - lstart[lev] < self.L["level_long"][lev])
                before = list(self.W)
                if op == OP_R1C:
                    a, q = self.expr(at + 5); b, q = self.expr(q); c, q = self.expr(q)
                    self.r1c(i, w[at + 1], w[at + 2], w[at + 3], w[at + 4], a, b, c)
                elif op == OP_NBITS:
                    v, q = self.expr(at + 3)
                    for k in range(w[at + 2]):
                        self.W[w[at + 1] + k] = (v >> k) & 1 if k < 256 else 0
                elif op == OP_LOOKUP:
                    q = at + 4
                    for e in range(w[at + 2]):
                        v, q = self.expr(q)
                        self.lookup(i, w[at + 1] + e, w[at + 3], v)
                elif op == OP_COUNT:
                    self.count(i, at); q = at + nwords
                else:
                    assert op in (OP_RANDOMIZE, OP_COMMIT)
                    self.W[w[at + 1]:w[at + 1] + w[at + 2]] = [self.mask if op == OP_RANDOMIZE else self.commit] * w[at + 2]
                    q = at + 3
                assert q == at + nwords, (op, q, at, nwords)
                done += [k for k in range(len(before)) if before[k] is None and self.W[k] is not None]
            assert len(done) == len(set(done))      # the ops of a level are independent
        return self

    def few(self):
        """the 8-word descriptors and term lists, as k_solver_few walks them, and the count levels by FewProgram::count_ops / count_qoff"""
        L = self.L
        ops, terms, ls = L["few_ops"], L["few_terms"], L["few_level_start"]
        for lev in range(L["n_levels"]):
            if L["level_kind"][lev]:
                assert ls[lev] == ls[lev + 1]
                for k in range(L["few_count_first"][lev], L["few_count_first"][lev + 1]):
                    at, qb, nq = L["few_count_ops"][4 * k:4 * k + 3]
                    assert nq == L["words"][at + 4]
                    q = at + 5 + 6 * L["words"][at + 2]
                    for j in range(nq):      # count_qoff: where every query starts
                        assert L["few_count_qoff"][qb + j] == q
                        q += 1 + 2 * L["words"][q]; q += 1 + 2 * L["words"][q]
                    self.count(0, at)
                continue
            for i in range(ls[lev], ls[lev + 1]):
                d = ops[8 * i:8 * i + 8]
                op, t0 = d[0] & 0xFF, d[4]
                s = lambda a, n: sum(self.term(terms[2 * (t0 + a + k)], terms[2 * (t0 + a + k) + 1]) for k in range(n)) % R
                if op == OP_R1C:
                    self.r1c(i, d[0] >> 8, d[1], d[2], d[3], s(0, d[5]), s(d[5], d[6]), s(d[5] + d[6], d[7]))
                elif op == OP_NBITS:
                    v = s(0, d[5])
                    for k in range(d[2]):
                        self.W[d[1] + k] = (v >> k) & 1 if k < 256 else 0
                elif op == OP_LOOKUP:
                    self.lookup(i, d[1], d[2], s(0, d[5]))
                else:
                    assert op in (OP_RANDOMIZE, OP_COMMIT)
                    self.W[d[1]:d[1] + d[2]] = [self.mask if op == OP_RANDOMIZE else self.commit] * d[2]
        assert len(terms) >= 2 * 192 and not any(terms[-512:]) and not any(ops[-8:])      # the pads the kernel may fetch
        return self

    def small(self):
        """the small program's items on plain integers: chain levels, then rows -> (flag, W, A, B, C, failed rows)"""
        L = self.L
        sgn = lambda v: v - R if v > M.HALF else v
        n_in = sum(1 for v in self.W if v is not None)
        W8, flag = [0] * L["rows_per_group"], 0
        for k in range(n_in):
            v = sgn(self.W[k])
            flag |= v not in (-1, 0, 1)
            W8[k] = v if v in (-1, 0, 1) else 0
        i32 = lambda x: x - (1 << 32) if x >> 31 else x

        def tiny(d):
            v = [W8[x] for x in d[2:8]]
            c = [i32(x) for x in d[8:14]]
            return c[0] * v[0] + c[1] * v[1], c[2] * v[2] + c[3] * v[3], c[4] * v[4] + c[5] * v[5]
        for l in range(L["small_levels"]):
            t0, t1, p0, p1, b0, b1 = L["levels"][6 * l:6 * l + 6]
            assert (t1 - t0) % 8 == 0
            new, sums = {}, {}
            for i in range(t0, t1):
                d = L["tiny"][16 * i:16 * i + 16]
                a, b, c = tiny(d)
                w = a * b - c
                if d[0] & 0x100:
                    w = -w
                if not d[0] & 1:
                    assert d[1] == L["scratch_row"] and w == 0
                flag |= w not in (-1, 0, 1)
                new[d[1]] = w
            for i in range(p0, p1):
                slot, first, chunks = L["parts"][4 * i:4 * i + 3]
                assert chunks <= 4
                sums[slot] = sum(L["tcoef"][first + k] * W8[L["twire"][first + k]] for k in range(8 * chunks))
            for i in range(b0, b1):
                out, sl, bb = L["bits"][4 * i:4 * i + 3]
                s = sum(sums[(sl & 0xFFFF) + k] for k in range(sl >> 16))
                flag |= s < 0
                for b in range(bb >> 8):
                    new[out + b] = (s >> ((bb & 0xFF) + b)) & 1
            for k, v in new.items():
                W8[k] = v if v in (-1, 0, 1) else 0
        rows, failed = {}, []
        items = [(L["rtiny"][16 * i], L["rtiny"][16 * i + 1], tiny(L["rtiny"][16 * i:16 * i + 16])) for i in range(L["n_rtiny"]) if L["rtiny"][16 * i] & 1]
        for i in range(L["n_rgen"]):
            fl, cidx, tt, ch = L["rgen"][8 * i], L["rgen"][8 * i + 1], L["rgen"][8 * i + 2], L["rgen"][8 * i + 3:8 * i + 6]
            vals = []
            for n in ch:
                vals.append(sum(L["rtcoef"][tt + k] * W8[L["rtwire"][tt + k]] for k in range(8 * n))); tt += 8 * n
            items.append((fl, cidx, tuple(vals)))
        for fl, cidx, (a, b, c) in items:
            if a * b != c:
                failed.append(cidx)
            for v, shift in ((a, 16), (b, 18), (c, 20)):
                flag |= not (fl >> shift) & 1 and v not in (-1, 0, 1)
            assert cidx not in rows
            rows[cidx] = (a % R, b % R, c % R)
            assert ((fl >> 16) & 1, (fl >> 18) & 1, (fl >> 20) & 1) == (L["cls_a"][cidx], L["cls_b"][cidx], L["cls_c"][cidx])
        n = len(self.A)
        assert sorted(rows) == list(range(n))
        return int(flag), [v % R for v in W8[:len(self.W)]], [rows[i][0] for i in range(n)], [rows[i][1] for i in range(n)], [rows[i][2] for i in range(n)], failed


# ---- 1. the checker and the table's own conditions ----
@pytest.mark.parametrize("name", M.case_names())
def test_checker_passes_on_every_satisfied_column(name):
    case = M.case_table()[name]
    desc, cols, masks, commits = case.made()
    ref = case.reference()
    assert len(cols) == case.batch and case.batch % 64 == 0
    bad = [p for p in range(case.ncols()) if isinstance(ref[p], int)]
    assert 4 * len(bad) <= case.ncols(), "more than a quarter of the columns are unsatisfied"
    assert bool(bad) == case.expect_fail, "a case that expects no failure has none in the reference (and the other way round)"
    for p, sol in enumerate(ref):
        if not isinstance(sol, int):
            M.check(desc, *sol)
            assert all(0 <= v < R for part in sol for v in part)
    if case.mode == 1 and case.expect_flag is not None:
        cls = case.class_vectors()
        flags = [M.small_flag(desc, cls, s) for s in ref if not isinstance(s, int)]
        assert max(flags) == case.expect_flag


def test_case_table_is_what_the_issue_lists():
    names = M.case_names()
    assert len(names) >= 150 and len(set(names)) == len(names)
    t = M.case_table()
    assert any(c.batch == 2112 and c.made()[0]["calldata"] and len(c.made()[0]["blueprint"]) <= 60 for c in t.values())
    assert {c.nproofs for c in t.values()} >= {0, 1, 2, 3, 32} and {c.workgroups for c in t.values() if c.nproofs} == {0, 1, 17}
    for width in (1, 8, 9, 128, 129):      # the small path's level of `width` items
        assert len(M.schedule(t["small_levels_%d" % width].made()[0])[1][1][1]) == width
    nw = max(c.made()[0]["n_public"] + c.made()[0]["n_secret"] + c.made()[0]["n_internal"] for c in t.values())
    assert nw <= 700, nw      # every case is small (the largest: two nBits hints of 300 outputs)


# ---- 2. the reference against the oracle ----
def _oracle_columns(oracle, harness, tmp_path, name, cipher, stmts):
    src, dst = tmp_path / name, tmp_path / (name + ".desc")
    src.write_bytes(golden_bytes(name))
    subprocess.check_call([harness, "dump", str(src), str(dst)])
    desc = read_desc(dst.read_bytes())
    cs = oracle.R1CS(golden_bytes(name))
    be = lambda b: [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(len(b) // 32)]
    out = []
    for key, nonce, counter, pt in stmts:
        aes = cipher != "chacha20"
        rc, _ct, W, A, B, C = cs.solve(cipher, key, nonce, counter, pt, mask=(7).to_bytes(32, "big") if aes else None, commit=(9).to_bytes(32, "big") if aes else None)
        assert rc == 0
        out.append((W, A, B, C, be(W), be(A), be(B), be(C)))
    return desc, out


def test_reference_reproduces_the_oracle_on_chacha20(oracle, harness, tmp_path):
    desc, sols = _oracle_columns(oracle, harness, tmp_path, "r1cs.chacha20", "chacha20", [(KAT["key"], KAT["nonce"], KAT["counter"], KAT["input"])])
    Wb, Ab, Bb, Cb, W, A, B, C = sols[0]
    n_in = desc["n_public"] + desc["n_secret"]
    got = M.solve(desc, [W[1:n_in]])[0]
    assert not isinstance(got, int) and list(got[0]) == W and (got[1], got[2], got[3]) == (A, B, C)
    be = lambda v: b"".join(x.to_bytes(32, "big") for x in v)
    assert hashlib.sha256(be(got[0])).hexdigest() == KAT["sha256_W"]
    assert hashlib.sha256(be(got[1]) + be(got[2]) + be(got[3])).hexdigest() == KAT["sha256_abc"]
    M.check(desc, *got)
    kinds = {it["kind"] for it in M.instructions(desc)}
    assert kinds == {"r1c", "nbits"}


def test_reference_reproduces_the_oracle_on_aes128(oracle, harness, tmp_path):
    stmt = (bytes(range(16)), bytes(range(12)), 5, bytes(range(64)))
    desc, sols = _oracle_columns(oracle, harness, tmp_path, "r1cs.aes128", "aes-128-ctr", [stmt])
    Wb, Ab, Bb, Cb, W, A, B, C = sols[0]
    n_in = desc["n_public"] + desc["n_secret"]
    got = M.solve(desc, [W[1:n_in]], masks=[7], commits=[9])[0]
    assert not isinstance(got, int) and list(got[0]) == W and (got[1], got[2], got[3]) == (A, B, C)
    M.check(desc, *got)
    assert {it["kind"] for it in M.instructions(desc)} == {"r1c", "nbits", "count", "randomize", "commit", "lookup"}      # all six kinds, pinned to gnark


# ---- 3. the builders on the host ----
@pytest.mark.parametrize("name", M.case_names())
def test_builders_layouts_replay_to_the_reference(harness, tmp_path, name):
    case = M.case_table()[name]
    desc, cols, masks, commits = case.made()
    ref = case.reference()
    classes = case.class_vectors() if case.mode == 1 else None
    rc, text, L = build_layouts(harness, tmp_path, desc, classes)
    assert rc == 0, text
    order, levels = M.schedule(desc)
    # the model's restatement of the schedule is the builder's
    nlev = L["sched"][0]
    assert nlev == len(levels) == L["n_levels"] and L["level_kind"] == [k for k, _, _ in levels] and L["level_long"] == [n for _, _, n in levels]
    assert [L["sched"][1 + l + 1] - L["sched"][1 + l] for l in range(nlev)] == [len(g) for _, g, _ in levels]
    for p in list(range(min(case.batch, 64))):
        args = (desc, L, cols[p], masks[p] if masks else 0, commits[p] if commits else 0)
        for route in ("words", "few"):
            r = getattr(Replay(*args), route)()
            if isinstance(ref[p], int):
                assert r.status is not None
                if route == "words":
                    assert r.status == order.index(ref[p]), (p, r.status, ref[p])
            else:
                assert r.status is None and (r.W, r.A, r.B, r.C) == tuple(list(x) for x in ref[p]), (route, p)
        if case.mode == 1:
            assert L["small_ok"] == 1, text
            flag, W, A, B, C, failed = Replay(*args).small()
            if isinstance(ref[p], int):
                assert failed
            elif M.small_flag(desc, classes, ref[p]):
                assert flag == 1
            else:
                assert flag == 0 and not failed and (W, A, B, C) == tuple(list(x) for x in ref[p]), p


def test_small_program_refusals(harness, tmp_path):
    for what, (build, why) in M.small_refusals().items():
        c, cols = build(64)
        desc = c.desc()
        nw = c.n_wires
        rc, text, L = build_layouts(harness, tmp_path, desc, ([1] * nw, [1] * c.n_constraints, [1] * c.n_constraints, [1] * c.n_constraints))
        assert rc == 0 and L["small_ok"] == 0 and why in text, (what, text)


# ---- 4. the refusal list under the sanitizers ----
def test_malformed_descriptions_throw_under_sanitizers(harness_san, tmp_path):
    good = M.case_table()["status_first_failure"].made()[0]
    rc, text, L = build_layouts(harness_san, tmp_path, good)
    assert rc == 0, text
    for what, (desc, why) in M.malformed_descriptions().items():
        if why is None:
            continue      # refused by the hook or on the device, not by a builder
        rc, text, L = build_layouts(harness_san, tmp_path, desc)
        assert rc == 3 and text.strip() == "REFUSED: " + why, (what, rc, text)


def test_hook_is_exported_and_bound():
    import re
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    assert " T gsc_debug_solve\n" in syms and "extern int gsc_debug_solve(" in header and "struct gsc_debug_solve_args {" in header
    import gsc_loader
    g = gsc_loader.load()
    assert "gsc_debug_solve" in g.EXPORTS and callable(g.debug_solve)
    # the ctypes structure follows the header's field order
    fields = [f[0] for f in g.DebugSolveArgs._fields_]
    body = header[header.index("struct gsc_debug_solve_args {"):]
    body = body[:body.index("};")]
    assert re.findall(r"(\w+)\s*[,;]", body) == fields
    for txt in ("INTEGRATION.md", "DESIGN.md"):
        assert "gsc_debug_solve" in open(os.path.join(ROOT, txt)).read(), txt
