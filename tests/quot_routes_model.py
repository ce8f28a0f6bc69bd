"""Reference of the evaluation-form quotient kernels' production routes (csrc/k_ntt.hip through gsc_debug_quotient, include/libprove.h) and the
case tables of tests/test_gpu_quot_routes.py.  Every value is a plain Python integer; numpy only moves bytes (planes, big-endian matrices, the digit
buffer) and carries the bulk recoder recode_columns, which tests/test_quot_routes_model_host.py holds against the integer one.

  coset_product(a, b, L)   d_i = A(zeta w^i) B(zeta w^i) 2^261 mod r from the values of A and B on the n-th roots of unity (rows >= len count as zero)
  values_for(T, L)         the a (n values) for which b = 1 everywhere gives d = T exactly
  recode(T, c)             the signed digits of signed_digit_step (csrc/msm_dev.hpp), msm_windows(c) of them
  digits_of(buf, L, c, column)   the hook's digit buffer of one column as [window][natural index]
  planes_of / Col          a column as a ternary plane with wide rows, the form the small-integer witness path leaves a and b in

The case tables (table_small, table_mixed, table_aes, digit_columns) say per tile of four columns which branch of the first kernel each wave is meant
to take; wave_branches computes what the kernel's index arithmetic really gives (the tile condition) and the host test holds one against the other."""
import hashlib
import random

import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
ROOT_2_28 = 0x2a3c09f0a58a7e8500e0a7eb8ef62abc402d111e41112ed49bd61b6e725b19f0      # gnark-crypto's 2^28-th root of unity of Fr (tests/test_gpu_ntt.py)
WIDE = -128                       # WS_PLANE_WIDE (csrc/kernels.hpp)
MSM_MAX_WINDOW = 17               # csrc/kernels.hpp
P = 4                             # columns per workgroup tile (csrc/k_ntt.hip)
R261 = pow(2, 261, R)
R256 = pow(2, 256, R)
N_CONSTRAINTS_CHACHA = 23617      # ChaCha20-V3: the table the host test proves is built with it, the GPU test holds the engine's count against it


# ---- transforms ------------------------------------------------------------------------------------------------------------
_roots = {}


def roots(L):
    """(zeta, w, [w^k for k < n/2], [w^-k for k < n/2]) of the domain of size n = 2^L"""
    if L not in _roots:
        n = 1 << L
        zeta = pow(ROOT_2_28, 1 << (27 - L), R); w = zeta * zeta % R
        assert pow(zeta, n, R) == R - 1
        w_inv = pow(w, R - 2, R)
        fw, iv = [1] * max(n // 2, 1), [1] * max(n // 2, 1)
        for k in range(1, n // 2):
            fw[k] = fw[k - 1] * w % R; iv[k] = iv[k - 1] * w_inv % R
        _roots[L] = (zeta, w, fw, iv)
    return _roots[L]


def _transform(vals, tw):
    """sum_k vals[k] x^(i k) at x = tw[1] for every i: decimation in time on a bit-reversed copy, natural order out (tw: the n/2 powers of x)"""
    n = len(vals); lg = n.bit_length() - 1
    a = [0] * n
    for i in range(n):
        a[int(format(i, "0%db" % lg)[::-1], 2) if lg else 0] = vals[i]
    half = 1
    while half < n:
        step = n // (2 * half)
        ts = tw[0:half * step:step]
        for k in range(0, n, 2 * half):
            lo = a[k:k + half]
            hi = [x * t % R for x, t in zip(a[k + half:k + 2 * half], ts)]
            a[k:k + half] = [(u + v) % R for u, v in zip(lo, hi)]
            a[k + half:k + 2 * half] = [(u - v) % R for u, v in zip(lo, hi)]
        half *= 2
    return a


_coset_cache = {}


def coset_values(vals, L):
    """A(zeta w^i), i < n, of the polynomial A of degree < n with A(w^i) = vals[i] (zero for i >= len(vals)).  Cached by content."""
    n = 1 << L
    key = (L, len(vals), hashlib.sha256(b"".join(int(v).to_bytes(32, "little") for v in vals)).digest())
    hit = _coset_cache.get(key)
    if hit is not None:
        return hit
    zeta, w, fw, iv = roots(L)
    full = list(vals) + [0] * (n - len(vals))
    n_inv = pow(n, R - 2, R)
    coef = _transform(full, iv)
    zk = n_inv
    for k in range(n):
        coef[k] = coef[k] * zk % R; zk = zk * zeta % R
    out = _transform(coef, fw)
    if len(_coset_cache) >= 64:
        _coset_cache.clear()
    _coset_cache[key] = out
    return out


def coset_product(a, b, L):
    return [x * y % R * R261 % R for x, y in zip(coset_values(a, L), coset_values(b, L))]


def values_for(T, L):
    """the inverse of coset_product in a with b = 1 (B = 1): A(zeta w^i) = T_i / 2^261"""
    n = 1 << L
    assert len(T) == n
    zeta, w, fw, iv = roots(L)
    k261 = pow(R261, R - 2, R) * pow(n, R - 2, R) % R
    coef = _transform([t * k261 % R for t in T], iv)      # n^-1 sum_i T_i / 2^261 w^(-ik) = zeta^k A_k
    zeta_inv = pow(zeta, R - 2, R); zk = 1
    for k in range(n):
        coef[k] = coef[k] * zk % R; zk = zk * zeta_inv % R
    return _transform(coef, fw)


# ---- digits ----------------------------------------------------------------------------------------------------------------
def msm_windows(c):
    """csrc/kernels.hpp msm_windows: the top window absorbs the last carry"""
    nwin = (254 + c - 1) // c
    if ((R - 1) >> (c * (nwin - 1))) + 1 > (1 << (c - 1)) - 1:
        nwin += 1
    return nwin


def recode(T, c):
    """signed_digit_step (negated = false), msm_windows(c) times: digit_j in [-2^(c-1), 2^(c-1)), sum digit_j 2^(c j) = T"""
    out, carry, D = [], 0, 1 << (c - 1)
    for _ in range(msm_windows(c)):
        raw = (T & ((1 << c) - 1)) + carry
        T >>= c
        if raw >= D:
            out.append(raw - (1 << c)); carry = 1
        else:
            out.append(raw); carry = 0
    assert T == 0 and carry == 0
    return out


def recode_columns(le, c):
    """The same for many scalars at once: le = (N, 32) uint8, little-endian canonical values -> (nwin, N) int32"""
    le = np.ascontiguousarray(le, dtype=np.uint8).reshape(-1, 32)
    nwin = msm_windows(c)
    bits = np.unpackbits(le, axis=1, bitorder="little")
    bits = np.concatenate([bits, np.zeros((bits.shape[0], max(0, nwin * c - 256)), dtype=np.uint8)], axis=1)
    weights = (1 << np.arange(c, dtype=np.int64))
    out = np.empty((nwin, le.shape[0]), dtype=np.int32)
    carry = np.zeros(le.shape[0], dtype=np.int64)
    for j in range(nwin):
        raw = bits[:, c * j:c * j + c].astype(np.int64) @ weights + carry
        carry = (raw >= (1 << (c - 1))).astype(np.int64)
        out[j] = raw - (carry << c)
    assert not carry.any()
    return out


def quot_digit_index(L, t):
    """csrc/kernels.hpp quot_digit_index: the natural index at table position t (Python integers or numpy arrays)"""
    Lhi = (L + 1) // 2; Llo = L - Lhi; quarter = (1 << Lhi) // 4
    kq, m = t & 3, t >> 2
    return (((m % quarter) + kq * quarter) << Llo) + m // quarter


def digits_by_position(buf, L, c, column):
    """(nwin, n) int32: the digits of one column in table order.  16-byte word (j * n/8 + octet) * 64 + column holds eight int16 (c <= 16); c = 17
    takes two words at twice that index, eight int32: the positions 8 octet .. 8 octet + 7."""
    n = 1 << L; nwin = msm_windows(c); noct = n // 8
    raw = np.frombuffer(buf, dtype=np.int32 if c > 16 else np.int16)
    assert raw.size == nwin * noct * 64 * 8
    return raw.reshape(nwin, noct, 64, 8)[:, :, column, :].reshape(nwin, n).astype(np.int32)


def digits_of(buf, L, c, column):
    """(nwin, n) int32: digit j of natural index i at [j][i] (table position t is index quot_digit_index(L, t))"""
    pos = digits_by_position(buf, L, c, column)
    out = np.empty_like(pos)
    out[:, quot_digit_index(L, np.arange(1 << L))] = pos
    return out


# ---- columns ---------------------------------------------------------------------------------------------------------------
class Col:
    """One column of a or b: tern (n int8 entries 0, 1, -1) and wide = {row: value}, the rows that travel as 32-byte values under a wide marker
    (their tern entry is not used).  all_wide: every row is wide with that one value."""
    def __init__(self, tern, wide=None, all_wide=None):
        self.tern = np.asarray(tern, dtype=np.int8); self.wide = dict(wide or {}); self.all_wide = all_wide

    def values(self, m):
        if self.all_wide is not None:
            return [self.all_wide] * m
        v = [int(t) % R for t in self.tern[:m]]
        for row, x in self.wide.items():
            if row < m:
                v[row] = x
        return v

    def plane(self, m):
        """n entries; rows >= m are marked wide: nothing may read them"""
        p = np.full(self.tern.size, WIDE, dtype=np.int8)
        if self.all_wide is None:
            p[:m] = self.tern[:m]
            rows = [r for r in self.wide if r < m]
            p[rows] = WIDE
        return p

    def be(self, m):
        """(m, 32) uint8: the values as canonical big-endian bytes"""
        if getattr(self, "_be_all", None) is None:
            out = np.zeros((self.tern.size, 32), dtype=np.uint8)
            if self.all_wide is not None:
                out[:] = _be(self.all_wide)
            else:
                out[self.tern == 1, 31] = 1
                out[self.tern == -1] = _be(R - 1)
                if self.wide:
                    rows = list(self.wide)
                    out[rows] = np.frombuffer(b"".join(self.wide[r].to_bytes(32, "big") for r in rows), dtype=np.uint8).reshape(-1, 32)
            self._be_all = out
        return self._be_all[:m]


def _be(v):
    return np.frombuffer(int(v).to_bytes(32, "big"), dtype=np.uint8)


def planes_of(values):
    """values (integers below r) -> (plane, wide): 0, 1 and r-1 become the entries 0, 1, -1, every other value a wide marker"""
    plane = np.array([0 if v == 0 else 1 if v == 1 else -1 if v == R - 1 else WIDE for v in values], dtype=np.int8)
    return plane, {i: v for i, v in enumerate(values) if plane[i] == WIDE}


def matrices(cols_a, cols_b, m):
    """(mats_be (2, m, 64, 32) uint8, planes (2, n, 64) int8) of 64 columns"""
    n = cols_a[0].tern.size
    mats = np.empty((2, m, 64, 32), dtype=np.uint8); planes = np.empty((2, n, 64), dtype=np.int8)
    for k, cols in enumerate((cols_a, cols_b)):
        for c, col in enumerate(cols):
            mats[k, :, c] = col.be(m); planes[k, :, c] = col.plane(m)
    return mats, planes


def wave_branches(cols, L, m):
    """The tile condition.  (16, 2^Llo, waves) bool: True where wave `w` of workgroup `g` of the first kernel takes the MIXED branch for the tile of
    columns 4 k .. 4 k + 3: thread (u4, q) of a workgroup holds the rows ((u4 + j G/4) << Llo) + g, j < 4, of column q; a wave is 16 values of u4 by
    the four columns, and __all(small) fails for it as soon as one of those rows below m is wide in one of the four columns."""
    Lhi = (L + 1) // 2; Llo = L - Lhi; G = 1 << Lhi; n = 1 << L
    rows = np.arange(n)
    g, e = rows & ((1 << Llo) - 1), rows >> Llo
    wave = (e % (G // 4)) // 16
    out = np.zeros((len(cols) // P, 1 << Llo, G // 64), dtype=bool)
    for c, col in enumerate(cols):
        wide = (col.plane(m) == WIDE) & (rows < m)
        out[c // P, g[wide], wave[wide]] = True
    return out


def meets(branches, want):
    """want: 'small' no wave mixed, 'mixed' every wave mixed, 'both' some of each, 'one' exactly one wave mixed"""
    k = int(branches.sum())
    return {"small": k == 0, "mixed": k == branches.size, "both": 0 < k < branches.size, "one": k == 1}[want]


# ---- case tables -----------------------------------------------------------------------------------------------------------
# A table: {"a": 64 Col, "b": 64 Col, "special": the columns held against the reference, "want": {m or None: [(want_a, want_b) per tile]}}.
# want is what each tile's waves are meant to do at m rows (None: at every m).
def _tern(rng, n, weights):
    return np.array(rng.choices((0, 1, -1), weights=weights, k=n), dtype=np.int8)


def _quads(n, pattern):
    return np.repeat(np.array(pattern, dtype=np.int8), n // 4)      # rows i, i + n/4, i + n/2, i + 3n/4: one thread's four elements


def table_small(L):
    """Every tile ternary: all waves take the small branch.  Columns 0 .. 7 are the special ones: 0 random, 1 all +1, 2 all -1, 3 zero, 4 .. 7 the
    quads (+1, -1, +1, -1), its negation, (+1, +1, -1, -1), its negation — a0 - a1 = +-4, t0 - t2 = +-2 in a thread's first two stages; all +1 and
    all -1 give a0 + a1 = +-4."""
    n = 1 << L; rng = random.Random(1000 + L)
    sp = [_tern(rng, n, (1, 1, 1)), np.ones(n, np.int8), -np.ones(n, np.int8), np.zeros(n, np.int8),
          _quads(n, (1, -1, 1, -1)), _quads(n, (-1, 1, -1, 1)), _quads(n, (1, 1, -1, -1)), _quads(n, (-1, -1, 1, 1))]
    ring = [0, 1, 2, 4, 5, 6, 7]      # b of a special column is the next special column (zero stays with zero: it would hide its partner)
    a = [Col(t) for t in sp]
    b = [Col(sp[3]) if c == 3 else Col(sp[ring[(ring.index(c) + 1) % 7]]) for c in range(8)]
    for c in range(8, 64):
        wts = [(1, 1, 1), (8, 1, 0), (1, 8, 0), (20, 1, 1), (0, 1, 1), (1, 0, 1)][c % 6]      # dense, bits, sparse, signs only, ...
        a.append(Col(_tern(rng, n, wts))); b.append(Col(_tern(rng, n, wts[::-1] if c % 2 else wts)))
    return {"a": a, "b": b, "special": list(range(8)), "want": {None: [("small", "small")] * 16}}


def table_mixed(L, n_constraints):
    """Tiles with wide rows.  Special columns: 0 one wide row of a in a ternary tile (1: its ternary neighbour, which that wave takes through the mixed
    branch too); 4 ChaCha20's shape, 336 wide rows of b, the same rows in the tile's four columns; 8 every row wide, r-1 in a and b; 12 wide rows
    0, 1, 2, r-2; 13 every row a wide marker over a ternary value; 16, 60 random fillers."""
    n = 1 << L; rng = random.Random(2000 + L)
    tern = lambda: _tern(rng, n, (1, 1, 1))
    a, b = [None] * 64, [None] * 64
    # tile 0: one wide row (below 777, so that short vectors keep it)
    a[0] = Col(tern(), {300: rng.randrange(3, R - 2)})
    for c in (1, 2, 3):
        a[c] = Col(tern())
    for c in range(4):
        b[c] = Col(tern())
    # tile 1: the add32 rows of b
    rows = sorted(rng.sample(range(700), 16) + rng.sample(range(700, n_constraints), 320))
    for c in range(4, 8):
        a[c] = Col(tern()); b[c] = Col(_tern(rng, n, (4, 4, 1)), {r: rng.randrange(R) for r in rows})
    # tile 2: everything r-1 (the largest magnitudes the plain mixed branch sees)
    for c in range(8, 12):
        a[c] = Col(np.zeros(n, np.int8), all_wide=R - 1); b[c] = Col(np.zeros(n, np.int8), all_wide=R - 1)
    # tile 3: small values behind wide markers
    edge = (0, 1, 2, R - 2)
    a[12] = Col(tern(), {r: edge[(r // 5) % 4] for r in range(0, n, 5)}); b[12] = Col(tern(), {r: edge[(r // 7 + 1) % 4] for r in range(3, n, 7)})
    ta, tb = tern(), tern()
    a[13] = Col(ta, {r: int(ta[r]) % R for r in range(n)}); b[13] = Col(tb, {r: int(tb[r]) % R for r in range(n)})
    a[14] = Col(tern()); b[14] = Col(tern(), {r: R - 1 - (r % 3) for r in range(1, n, 2)})
    a[15] = Col(tern(), {n - 1: R - 1, 0: R - 2}); b[15] = Col(tern())
    want = [("one", "small"), ("small", "both"), ("mixed", "mixed"), ("mixed", "mixed")]
    want_short = [("one", "small"), ("small", "both"), ("both", "both"), ("both", "both")]      # m = 777: only the first wave of a workgroup holds rows below m
    # tiles 4 .. 15: fillers, a density of wide rows per vector
    dens = [(1.0, 1.0), (0.01, 0.0), (1.0, 0.0), (0.0, 0.5), (0.001, 0.001), (0.5, 0.5), (0.0, 1.0), (0.1, 0.0), (0.0, 0.0), (0.02, 0.3), (1.0, 0.01), (0.3, 0.3)]
    for t in range(4, 16):
        da, db = dens[t - 4]
        for c in range(4 * t, 4 * t + 4):
            for dst, d in ((a, da), (b, db)):
                wide = {r: rng.randrange(R) for r in range(n) if rng.random() < d} if 0 < d < 1 else {}
                dst[c] = Col(np.zeros(n, np.int8), {r: rng.randrange(R) for r in range(n)}) if d == 1.0 else Col(tern(), wide)
        kind = lambda d: "mixed" if d == 1.0 else "small" if d == 0.0 else None
        want.append((kind(da), kind(db))); want_short.append((None if da == 1.0 else kind(da), None if db == 1.0 else kind(db)))
    return {"a": a, "b": b, "special": [0, 1, 4, 8, 12, 13, 16, 60], "want": {1 << L: want, n_constraints: want, 777: want_short}}


def table_aes(L):
    """The 2^17 domain (nine strided stages: an odd count after the two register stages).  Tile 0 every row wide with r-1, tile 1 random ternary,
    tile 2 the +-4 quads; fillers behind.  Special columns: 0 and 8."""
    n = 1 << L; rng = random.Random(3000 + L)
    tern = lambda: _tern(rng, n, (1, 1, 1))
    a = [Col(np.zeros(n, np.int8), all_wide=R - 1) for _ in range(4)] + [Col(tern()) for _ in range(4)]
    b = [Col(np.zeros(n, np.int8), all_wide=R - 1) for _ in range(4)] + [Col(tern()) for _ in range(4)]
    pats = [(1, -1, 1, -1), (-1, 1, -1, 1), (1, 1, -1, -1), (-1, -1, 1, 1)]
    a += [Col(_quads(n, p)) for p in pats]; b += [Col(_quads(n, p)) for p in (pats[0], pats[0], pats[1], pats[2])]
    want = [("mixed", "mixed"), ("small", "small"), ("small", "small")]
    for t in range(3, 16):
        for c in range(4 * t, 4 * t + 4):
            wa = {r: rng.randrange(R) for r in rng.sample(range(n), 50)} if t % 2 else {}
            a.append(Col(tern(), wa)); b.append(Col(tern(), {r: R - 1 for r in rng.sample(range(n), 3)} if t % 3 == 0 else {}))
        want.append(("both" if t % 2 else "small", "both" if t % 3 == 0 else "small"))
    return {"a": a, "b": b, "special": [0, 8], "want": {None: want}}


DIGIT_WIDTHS = (17, 16, 8)      # the c = 17 specialisation; the int16 packing at its widest and at a narrow width.  (MSM_MAX_WINDOW = 17 and
                                # msm_windows(17) = 15: the generic loop with 32-bit words cannot be reached through launch_compute_d_digits.)


def _windows(c, v):
    """every c-bit window equal to v, cut below r"""
    x = sum(v << (c * j) for j in range(254 // c + 1)) & ((1 << 253) - 1)
    assert x < R
    return x


def special_scalars():
    """the chosen values of d, for every width of DIGIT_WIDTHS at once"""
    s = [0, 1, R - 1, R - 2, (1 << 253) - 1, 1 << 253,
         int("aa" * 32, 16) & ((1 << 253) - 1), int("55" * 32, 16) & ((1 << 253) - 1), int("aaaaaaaa55555555" * 4, 16) & ((1 << 253) - 1), int("ffffffff00000000" * 4, 16) & ((1 << 253) - 1)]
    for c in DIGIT_WIDTHS:
        s += [1 << (c - 1), (1 << (c - 1)) - 1, (1 << c) - 1, 1 << c, _windows(c, (1 << (c - 1)) - 1), _windows(c, 1 << (c - 1)), _windows(c, (1 << c) - 1)]
    return s


def never_carries(c):
    return _windows(c, (1 << (c - 1)) - 1)


def always_carries(c):
    return _windows(c, 1 << (c - 1))


def digit_columns(L):
    """Eight columns of chosen d (n values each).  A thread of the last kernel holds the indices i, i + n/4, i + n/2, i + 3n/4 (i < n/4) and keeps one
    carry bit for each: column k < 3 puts always_carries(c) / never_carries(c) of DIGIT_WIDTHS[k] there in all sixteen combinations (i mod 16: every
    rotation of every mix); 3: 2^253 - 1 against 0 likewise; 4: r-1 against 1; 5: four special values drawn per thread; 6: one special value per
    thread, four times; 7: random."""
    n = 1 << L; q = n // 4; rng = random.Random(4000 + L)
    sp = special_scalars()
    cols = []
    pairs = [(always_carries(c), never_carries(c)) for c in DIGIT_WIDTHS] + [((1 << 253) - 1, 0), (R - 1, 1)]
    for hi, lo in pairs:
        T = [0] * n
        for i in range(q):
            for k in range(4):
                T[i + k * q] = hi if ((i % 16) >> k) & 1 else lo
        cols.append(T)
    cols.append([rng.choice(sp) for _ in range(n)])
    T = [0] * n
    for i in range(q):
        T[i] = T[i + q] = T[i + 2 * q] = T[i + 3 * q] = sp[i % len(sp)]
    cols.append(T)
    cols.append([rng.randrange(R) for _ in range(n)])
    return cols


def le_bytes(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32)
