"""Host-only proof (no GPU) of tests/quot_routes_model.py, the reference and case tables of tests/test_gpu_quot_routes.py: the coset product
against O(n^2) polynomial evaluation, values_for as its inverse, the recoding identities for every width and every chosen scalar, the bulk
recoder against the integer one, the digit buffer's index arithmetic against tests/native/quot_index_check.cpp, and the tile condition of every
case table (which branch of the first quotient kernel each wave takes).  Then the hook's boundary: exported, declared, wrapped, refused without
GSC_ENABLE_TEST_HOOKS."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import quot_routes_model as Q

R = Q.R
N_CONSTRAINTS_CHACHA = Q.N_CONSTRAINTS_CHACHA      # the GPU test asserts that the engine reports this count; any m above n/4 gives every wave a row below m


@pytest.mark.parametrize("L", [4, 6])
def test_coset_product_against_naive_evaluation(L):
    n = 1 << L; rng = random.Random(L)
    zeta, w, _, _ = Q.roots(L)
    for m in (n, n - 3, 1):
        a = [rng.randrange(R) for _ in range(m)]; b = [rng.choice((0, 1, R - 1, rng.randrange(R))) for _ in range(m)]

        def coeffs(v):      # Lagrange interpolation on the roots of unity, the slow way: c_k = n^-1 sum_i v_i w^(-ik)
            w_inv, n_inv = pow(w, R - 2, R), pow(n, R - 2, R)
            return [sum(v[i] * pow(w_inv, i * k, R) for i in range(len(v))) * n_inv % R for k in range(n)]
        ca, cb = coeffs(a), coeffs(b)
        for i in range(n):      # the polynomial really interpolates ...
            x = pow(w, i, R)
            assert sum(c * pow(x, k, R) for k, c in enumerate(ca)) % R == (a[i] if i < m else 0)
        want = []
        for i in range(n):      # ... and d_i is the product of the two at zeta w^i, in the kernels' 2^261 domain
            x = zeta * pow(w, i, R) % R
            want.append(sum(c * pow(x, k, R) for k, c in enumerate(ca)) * sum(c * pow(x, k, R) for k, c in enumerate(cb)) % R * pow(2, 261, R) % R)
        assert Q.coset_product(a, b, L) == want


@pytest.mark.parametrize("L", [4, 10])
def test_values_for_inverts_the_coset_product(L):
    n = 1 << L; rng = random.Random(10 + L)
    sp = Q.special_scalars()
    T = [sp[i % len(sp)] if i % 3 else rng.randrange(R) for i in range(n)]
    a = Q.values_for(T, L)
    assert all(0 <= v < R for v in a) and Q.coset_product(a, [1] * n, L) == T


def test_msm_windows_restated():
    assert [Q.msm_windows(c) for c in (17, 16, 15, 8, 4)] == [15, 16, 17, 32, 64]      # tests/native/quot_index_check.cpp, csrc/kernels.hpp
    assert max(Q.DIGIT_WIDTHS) <= Q.MSM_MAX_WINDOW == 17


@pytest.mark.parametrize("c", sorted(set(Q.DIGIT_WIDTHS) | {4, 13, 15}))
def test_recoding_identities(c):
    rng = random.Random(c)
    D = 1 << (c - 1)
    scalars = Q.special_scalars() + [rng.randrange(R) for _ in range(200)] + [rng.randrange(1 << rng.randrange(1, 254)) for _ in range(200)]
    seen_min = False
    for T in scalars:
        d = Q.recode(T, c)
        assert len(d) == Q.msm_windows(c) and all(-D <= x < D for x in d) and sum(x << (c * j) for j, x in enumerate(d)) == T
        seen_min |= -D in d
    assert seen_min                                                        # the digit -2^(c-1) is among the chosen cases
    assert Q.recode(D, c)[:2] == [-D, 1] and Q.recode(D - 1, c)[:2] == [D - 1, 0] and Q.recode((1 << c) - 1, c)[:2] == [-1, 1]
    # 2^253 - 1: the carry runs through every window that holds bits; never / always carrying scalars do what their names say
    top = 253 // c
    assert Q.recode((1 << 253) - 1, c)[:top] == [-1] + [0] * (top - 1)
    assert all(x == D - 1 for x in Q.recode(Q.never_carries(c), c)[:top]) and all(x < 0 for x in Q.recode(Q.always_carries(c), c)[:top])
    # the bulk recoder is the same function
    got = Q.recode_columns(Q.le_bytes(scalars), c)
    assert got.shape == (Q.msm_windows(c), len(scalars))
    assert [list(map(int, got[:, i])) for i in range(len(scalars))] == [Q.recode(T, c) for T in scalars]


@pytest.fixture(scope="module")
def kernel_positions(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("quot_index") / "quot_index_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "quot_index_check.cpp")])
    out = subprocess.run([exe, "dump"], capture_output=True, text=True, timeout=120, check=True).stdout
    return [tuple(map(int, l.split())) for l in out.splitlines()]


def test_digit_buffer_index_arithmetic(kernel_positions):
    assert {L for L, _, _, _ in kernel_positions} == {15, 16, 17}
    for L, t, index, header in kernel_positions:      # the kernel's thread arithmetic, and kernels.hpp's own function
        assert Q.quot_digit_index(L, t) == index == header
    for L in (15, 16, 17):
        assert sorted(Q.quot_digit_index(L, np.arange(1 << L)).tolist()) == list(range(1 << L))
    # a synthetic buffer written the way the kernel writes it (k_ntt.hip, EVAL == 2): thread (g, u4) puts element kq of window j into half mq & 1 of
    # octet mq >> 1, mq = g G/4 + u4; digits_of must hand digit (j, index) back
    L = 15; n = 1 << L; Lhi = (L + 1) // 2; Llo = L - Lhi; G = 1 << Lhi
    for c in (17, 8):
        nwin = Q.msm_windows(c); noct = n // 8
        words = np.zeros((nwin * noct * 64, 8), dtype=np.int32 if c > 16 else np.int16)
        col = 37
        for g in (0, 1, 77, (1 << Llo) - 1):
            for u4 in (0, 1, 2, G // 4 - 1):
                for j in (0, 3, nwin - 1):
                    mq = g * (G // 4) + u4; at = (j * noct + (mq >> 1)) * 64 + col
                    for kq in range(4):
                        index = ((u4 + kq * (G // 4)) << Llo) + g
                        words[at, 4 * (mq & 1) + kq] = (index * 7 + j) % 251 - 125
        dg = Q.digits_of(words.tobytes(), L, c, col)
        assert dg.shape == (nwin, n)
        for g in (0, 1, 77, (1 << Llo) - 1):
            for u4 in (0, 1, 2, G // 4 - 1):
                for j in (0, 3, nwin - 1):
                    for kq in range(4):
                        index = ((u4 + kq * (G // 4)) << Llo) + g
                        assert dg[j, index] == (index * 7 + j) % 251 - 125
        assert np.count_nonzero(Q.digits_of(words.tobytes(), L, c, col + 1)) == 0


def _check_table(tb, L, ms):
    n = 1 << L
    assert len(tb["a"]) == len(tb["b"]) == 64 and all(c.tern.size == n for c in tb["a"] + tb["b"]) and len(tb["special"]) <= 8
    reached = set()
    for m in ms:
        want = tb["want"].get(m, tb["want"].get(None))
        assert want is not None and len(want) == 16
        br = [Q.wave_branches(tb[k], L, m) for k in ("a", "b")]
        for tile in range(16):
            for k in range(2):
                if want[tile][k] is not None:
                    assert Q.meets(br[k][tile], want[tile][k]), (m, tile, "ab"[k], want[tile][k], int(br[k][tile].sum()))
        for c in tb["special"]:      # what a reference-checked column's waves reach with plain = 1
            for k in range(2):
                s = int(br[k][c // 4].sum())
                reached |= ({"mixed"} if s else set()) | ({"small"} if s < br[k][c // 4].size else set())
    return reached


def test_planes_and_columns():
    vals = [0, 1, R - 1, 2, R - 2, 5]
    plane, wide = Q.planes_of(vals)
    assert plane.tolist() == [0, 1, -1, Q.WIDE, Q.WIDE, Q.WIDE] and wide == {3: 2, 4: R - 2, 5: 5}
    col = Q.Col(plane, wide)
    assert col.values(6) == vals and col.values(4) == vals[:4]
    assert col.plane(4).tolist() == [0, 1, -1, Q.WIDE, Q.WIDE, Q.WIDE]      # rows >= m are marked wide
    assert [int.from_bytes(r.tobytes(), "big") for r in col.be(6)] == vals
    full = Q.Col(np.zeros(6, np.int8), all_wide=R - 1)
    assert full.values(3) == [R - 1] * 3 and (full.plane(3) == Q.WIDE).all() and int.from_bytes(full.be(2)[1].tobytes(), "big") == R - 1


def test_case_tables_meet_the_tile_condition():
    L = 15; n = 1 << L
    assert _check_table(Q.table_small(L), L, (n, N_CONSTRAINTS_CHACHA, 777)) == {"small"}
    tb = Q.table_mixed(L, N_CONSTRAINTS_CHACHA)
    assert _check_table(tb, L, (n, N_CONSTRAINTS_CHACHA, 777)) == {"small", "mixed"}
    # the special columns are what their names say
    assert len(tb["a"][0].wide) == 1 and min(tb["a"][0].wide) < 777 and not tb["b"][0].wide
    assert len(tb["b"][4].wide) == 336 and not tb["a"][4].wide and all(set(tb["b"][c].wide) == set(tb["b"][4].wide) for c in (5, 6, 7))
    assert tb["a"][8].all_wide == tb["b"][8].all_wide == R - 1
    assert set(tb["a"][12].wide.values()) == {0, 1, 2, R - 2} == set(tb["b"][12].wide.values())
    assert len(tb["a"][13].wide) == n and set(tb["a"][13].wide.values()) == {0, 1, R - 1}
    sm = Q.table_small(L)
    q = n // 4
    quads = lambda col: {tuple(int(col.tern[i + k * q]) for k in range(4)) for i in (0, 1, q - 1)}
    assert [quads(sm["a"][c]) for c in (4, 5, 6, 7)] == [{(1, -1, 1, -1)}, {(-1, 1, -1, 1)}, {(1, 1, -1, -1)}, {(-1, -1, 1, 1)}]
    assert (sm["a"][1].tern == 1).all() and (sm["a"][2].tern == -1).all() and not sm["a"][3].tern.any() and not sm["b"][3].tern.any()
    # the integers a thread's first two stages see: a0 +- a1 reaches +-4, t0 - t2 reaches +-2
    seen = set()
    for c in range(8):
        t = sm["a"][c].tern.astype(int)
        t0, t1, t2, t3 = t[:q], t[q:2 * q], t[2 * q:3 * q], t[3 * q:]
        seen |= {("sum", int(v)) for v in np.unique(t0 + t2 + t1 + t3)} | {("dif", int(v)) for v in np.unique(t0 + t2 - t1 - t3)} | {("t02", int(v)) for v in np.unique(t0 - t2)}
    assert {("sum", 4), ("sum", -4), ("dif", 4), ("dif", -4), ("t02", 2), ("t02", -2)} <= seen


def test_aes_table_meets_the_tile_condition():
    L = 17
    assert _check_table(Q.table_aes(L), L, (1 << L,)) == {"small", "mixed"}


def test_digit_columns_mix_carries_within_a_thread():
    L = 15; n = 1 << L; q = n // 4
    cols = Q.digit_columns(L)
    assert len(cols) == 8 and all(len(T) == n and all(0 <= v < R for v in T) for T in cols)
    for k, c in enumerate(Q.DIGIT_WIDTHS):
        hi, lo = Q.always_carries(c), Q.never_carries(c)
        masks = {sum((cols[k][i + j * q] == hi) << j for j in range(4)) for i in range(q)}
        assert masks == set(range(16)) and set(cols[k]) == {hi, lo}
    assert set(Q.special_scalars()) <= set(cols[5]) | set(cols[6])


def test_symbol_is_exported_declared_wrapped_and_refused_without_the_opt_in():
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    assert " T gsc_debug_quotient\n" in syms and "extern long long gsc_debug_quotient(" in header and "struct gsc_debug_quotient_args {" in header
    import gsc_loader
    g = gsc_loader.load()
    assert "gsc_debug_quotient" in g.EXPORTS and callable(g.debug_quotient)
    fields = [f[0] for f in g.DebugQuotientArgs._fields_]
    body = header[header.index("struct gsc_debug_quotient_args {"):]
    body = body[:body.index("};")]
    assert re.findall(r"(\w+)\s*[,;]", body) == fields
    for txt in ("INTEGRATION.md", "DESIGN.md"):
        assert "gsc_debug_quotient" in open(os.path.join(ROOT, txt)).read(), txt
    code = ("import os, sys, ctypes as C; os.environ.pop('GSC_ENABLE_TEST_HOOKS', None)\n"
            "sys.path.insert(0, %r); import gsc_loader; g = gsc_loader.load(); L = g.lib()\n"
            "assert L.gsc_debug_quotient(C.byref(g.DebugQuotientArgs())) == -1 and L.gsc_debug_quotient(None) == -1\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.count("gsc_debug_quotient refused: test hooks are disabled") == 2, out.stdout + out.stderr
