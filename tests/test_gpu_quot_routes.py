"""GPU tests of the quotient kernels' production routes (csrc/k_ntt.hip) through gsc_debug_quotient (include/libprove.h): the first kernel on
byte planes — the narrow9 route, the plain-integer small and mixed branches — the digits recoded inside the last kernel at c = 17, 16 and 8,
a few columns (ncols) and live tiles.  tests/test_gpu_ntt.py drives the same kernels with every optional argument at its default; a batch call
takes none of those defaults, and real witnesses (bits, pseudo-random d) never reach the integer scalings +-4, a wide row equal to r-1, d = 0 or
r-1, or a digit carry through every window.

The reference (tests/quot_routes_model.py, proven on a CPU by tests/test_quot_routes_model_host.py) is Python integers and costs about a second
and a half per column at 2^15, so a launch holds at most eight columns — every special one — against it; every other column must equal,
exactly, the generic route of the same hook (no planes, c = 0) on the expanded 32-byte values, which tests/test_gpu_ntt.py pins to the oracle.
Every comparison is equality of bytes."""
import functools
import re

import numpy as np
import pytest

from conftest import AES
import quot_routes_model as Q

pytestmark = pytest.mark.gpu

R = Q.R
L_CHACHA = 15


def _n_constraints(g, algo):
    nc = int(re.search(r"constraints=(\d+)", g.describe(algo)).group(1))
    assert algo != g.CHACHA20 or nc == Q.N_CONSTRAINTS_CHACHA      # the tables whose tile condition tests/test_quot_routes_model_host.py proves
    return nc


def _d(raw, n):
    return np.frombuffer(raw, dtype=np.uint8).reshape(n, 64, 32)


@functools.lru_cache(maxsize=None)
def _small():
    return Q.table_small(L_CHACHA)


@functools.lru_cache(maxsize=None)
def _mixed(n_constraints):
    return Q.table_mixed(L_CHACHA, n_constraints)


def _reference(tb, col, m, L):
    return Q.le_bytes(Q.coset_product(tb["a"][col].values(m), tb["b"][col].values(m), L))


def _rows(which, n, n_constraints):
    return {"n": n, "constraints": n_constraints, "777": 777}[which]


def _check_planes(g, algo, tb, L, m):
    """planes with plain = 1 and plain = 0 against the reference (special columns) and the generic route (every column)"""
    n = 1 << L
    mats, planes = Q.matrices(tb["a"], tb["b"], m)
    generic = _d(g.debug_quotient(algo, mats, m), n)
    want = {col: _reference(tb, col, m, L) for col in tb["special"]}
    for col, w in want.items():
        assert np.array_equal(generic[:, col], w), "generic route, column %d" % col
    # with planes a ternary row's 32-byte value is nobody's: r-2 there shows that the planes are what the kernel reads
    poisoned = mats.copy()
    poisoned[(planes[:, :m] != Q.WIDE)] = np.frombuffer((R - 2).to_bytes(32, "big"), dtype=np.uint8)
    for plain in (1, 0):
        got = _d(g.debug_quotient(algo, poisoned, m, planes=planes, plain=plain), n)
        for col, w in want.items():
            assert np.array_equal(got[:, col], w), "plain=%d column %d" % (plain, col)
        bad = np.flatnonzero((got != generic).any(axis=(0, 2)))
        assert bad.size == 0, "plain=%d: columns %s differ from the generic route" % (plain, bad.tolist())


@pytest.mark.parametrize("rows", ["n", "777", "constraints"])
def test_ternary_tiles_take_the_small_branch(gsc_chacha, rows):
    """random ternary, all +1, all -1, zero, the +-4 / +-2 quads: narrow9 (plain = 0) and the plain-integer small branch (plain = 1)"""
    g = gsc_chacha; n = 1 << L_CHACHA
    assert g.lib().gsc_debug_quotient(g.C.byref(g.DebugQuotientArgs(algorithm=g.CHACHA20))) == n
    _check_planes(g, g.CHACHA20, _small(), L_CHACHA, _rows(rows, n, _n_constraints(g, g.CHACHA20)))


@pytest.mark.parametrize("rows", ["n", "777", "constraints"])
def test_tiles_with_wide_rows_take_the_mixed_branch(gsc_chacha, rows):
    """one wide row, ChaCha20's wide rows of b, every row r-1 (dif_run entered with d0 = 2 at its largest magnitudes), 0 / 1 / 2 / r-2 and ternary
    values behind wide markers; short vectors: rows >= m are wide markers over 0xFF bytes that nothing may read"""
    g = gsc_chacha; n = 1 << L_CHACHA; nc = _n_constraints(g, g.CHACHA20)
    _check_planes(g, g.CHACHA20, _mixed(nc), L_CHACHA, _rows(rows, n, nc))


def test_plain_without_planes_is_downgraded_to_the_generic_route(gsc_chacha):
    """the hook hands plain = 1 with null plane pointers to launch_quotient, whose own rule must clear it: with scale_mid_plain on 32-byte rows d is wrong"""
    g = gsc_chacha; n = 1 << L_CHACHA; nc = _n_constraints(g, g.CHACHA20)
    tb = _mixed(nc)
    mats, _ = Q.matrices(tb["a"], tb["b"], nc)
    generic = g.debug_quotient(g.CHACHA20, mats, nc)
    assert g.debug_quotient(g.CHACHA20, mats, nc, plain=1) == generic
    assert np.array_equal(_d(generic, n)[:, 8], _reference(tb, 8, nc, L_CHACHA))


def test_few_columns(gsc_chacha):
    """ncols = 5 (the latency path's shape) with planes: the tiles of columns 0 .. 7 run, the other columns keep what the hook's input kernel left"""
    g = gsc_chacha; n = 1 << L_CHACHA; m = _n_constraints(g, g.CHACHA20)
    tb = _mixed(m)
    mats, planes = Q.matrices(tb["a"], tb["b"], m)
    got = _d(g.debug_quotient(g.CHACHA20, mats, m, planes=planes, plain=1, ncols=5), n)
    for col in range(8):
        assert np.array_equal(got[:, col], _reference(tb, col, m, L_CHACHA)), "column %d" % col
    mont = {}
    for col in range(8, 64):
        vals = tb["a"][col].values(m)
        image = np.frombuffer(b"".join(mont.setdefault(v, (v * Q.R256 % R).to_bytes(32, "little")) for v in vals), dtype=np.uint8).reshape(m, 32)
        assert np.array_equal(got[:m, col], image), "column %d was touched" % col
    assert (got[m:, 8:] == 0xFF).all()


def test_live_tiles_with_planes_and_fused_digits(gsc_chacha):
    """live = 93 * 256 - 192 (ChaCha20's own count of tiles; the last one partly live) with planes, plain = 1 and c = 17: every position below live"""
    g = gsc_chacha; L = L_CHACHA; n = 1 << L; m = _n_constraints(g, g.CHACHA20)
    tb = _mixed(m)
    mats, planes = Q.matrices(tb["a"], tb["b"], m)
    live = 93 * 256 - 192
    generic = _d(g.debug_quotient(g.CHACHA20, mats, m), n)
    for col in tb["special"]:
        assert np.array_equal(generic[:, col], _reference(tb, col, m, L)), "generic route, column %d" % col
    buf = g.debug_quotient(g.CHACHA20, mats, m, planes=planes, plain=1, live=live, c=17)
    index = Q.quot_digit_index(L, np.arange(live))
    for col in range(64):
        got = Q.digits_by_position(buf, L, 17, col)[:, :live]
        assert np.array_equal(got, Q.recode_columns(generic[index, col], 17)), "column %d" % col
    for t in (0, live - 1):      # the integer recoder on the first and the last live position of the all-(r-1) column
        v = int.from_bytes(generic[index[t], 8].tobytes(), "little")
        assert [int(x) for x in Q.digits_by_position(buf, L, 17, 8)[:, t]] == Q.recode(v, 17)


# ---- the digits recoded inside the last kernel: d chosen through values_for -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _digit_inputs(n_constraints):
    """(T columns, mats): columns 0 .. 7 hold a = values_for(T), b = 1, m = n; the others random a and b on n_constraints rows, zero behind (one
    launch has m = n for the chosen columns' sake; test_fused_digits runs the others again with m = n_constraints at c = 17)"""
    L = L_CHACHA; n = 1 << L
    T = Q.digit_columns(L)
    rng = np.random.Generator(np.random.PCG64(5))
    mats = rng.integers(0, 256, size=(2, n, 64, 32), dtype=np.uint8)
    mats[..., 0] &= 0x1F                                   # < 2^253 < r
    mats[:, n_constraints:] = 0
    one = np.zeros(32, np.uint8); one[31] = 1
    for k, t in enumerate(T):
        a = Q.values_for(t, L)
        mats[0, :, k] = np.frombuffer(b"".join(v.to_bytes(32, "big") for v in a), dtype=np.uint8).reshape(n, 32)
        mats[1, :, k] = one
    return T, mats


def test_chosen_d_comes_back_exactly(gsc_chacha):
    g = gsc_chacha; n = 1 << L_CHACHA
    T, mats = _digit_inputs(_n_constraints(g, g.CHACHA20))
    d = _d(g.debug_quotient(g.CHACHA20, mats, n), n)
    for k, t in enumerate(T):
        assert np.array_equal(d[:, k], Q.le_bytes(t)), "column %d" % k


@pytest.mark.parametrize("c", Q.DIGIT_WIDTHS)
def test_fused_digits(gsc_chacha, c):
    """c = 17: the specialised recoder (funnel shifts at compile-time offsets); 16 and 8: signed_digit_step with packed int16 words, the digit -2^(c-1)
    included.  Chosen d: 0, 1, r-1, 2^(c-1), 2^(c-1) - 1, 2^c - 1, carry-free and always-carrying windows, 2^253 - 1, alternating bits — the four of a
    thread mixing carrying and carry-free scalars in all sixteen ways."""
    g = gsc_chacha; L = L_CHACHA; n = 1 << L
    T, mats = _digit_inputs(_n_constraints(g, g.CHACHA20))
    d = _d(g.debug_quotient(g.CHACHA20, mats, n), n)
    buf = g.debug_quotient(g.CHACHA20, mats, n, c=c)
    memo = {}
    for k, t in enumerate(T):
        assert np.array_equal(d[:, k], Q.le_bytes(t)), "column %d" % k
        got = Q.digits_of(buf, L, c, k)
        rows = list(range(n) if k < 7 else range(0, n, 61))      # the integer recoder on every chosen value; on the random column at a stride
        for i in rows:
            if t[i] not in memo:
                memo[t[i]] = Q.recode(t[i], c)
        want = np.array([memo[t[i]] for i in rows], dtype=np.int32).T
        bad = np.flatnonzero((got[:, rows] != want).any(axis=0))
        if bad.size:
            i = rows[bad[0]]
            raise AssertionError("c=%d column %d index %d (%d indices differ): d = %x, digits %s, want %s" % (c, k, i, bad.size, t[i], got[:, i].tolist(), memo[t[i]]))
    assert any(-(1 << (c - 1)) in w for w in memo.values())
    for col in range(64):
        assert np.array_equal(Q.digits_of(buf, L, c, col), Q.recode_columns(d[:, col], c)), "c=%d column %d" % (c, col)
    if c == 17:      # the filler columns once more with m = n_constraints: rows behind m are 0xFF bytes now, not zeros, and must give the same digits
        nc = _n_constraints(g, g.CHACHA20)
        short = g.debug_quotient(g.CHACHA20, np.ascontiguousarray(mats[:, :nc]), nc, c=c)
        for col in range(8, 64):
            assert np.array_equal(Q.digits_by_position(short, L, c, col), Q.digits_by_position(buf, L, c, col)), "m = n_constraints, column %d" % col


# ---- the 2^17 domain --------------------------------------------------------------------------------------------------------------------
def test_aes_domain_planes(gsc, aes_keys):
    """Lhi = 9: after the two register stages dif_run has an odd stage count, so one more unreduced stage runs before the reducing round.  Every row wide
    with r-1 (column 0), random ternary, the +-4 quads (column 8)."""
    name = "aes128"; algo = AES[name][0]; L = 17; n = 1 << L
    r1cs, pkb, vkb = aes_keys[name]
    assert gsc.init_algorithm(algo, pkb, r1cs)
    assert gsc.lib().gsc_debug_quotient(gsc.C.byref(gsc.DebugQuotientArgs(algorithm=algo))) == n
    _check_planes(gsc, algo, Q.table_aes(L), L, n)
