"""The quotient fold on Python integers, shared by test_quot_fold_dft_host.py and test_gpu_quot_fold_dft.py (no test of its own).

Notation is k_quot_bases.hip's: n = 2^L, x_i = w^i, y_i = zeta w^i, zeta^2 = w, zeta^n = -1.  `perm` maps a table position to a coset index;
the dropped set J is the table positions m - 1 .. n - 1.  Bases are modelled by their exponents: u[i] stands for U_i = u[i] G (i < m),
v[pos] for the V at table position pos (pos < n).  The engine's conventions are in the weights: its d is d_i 2^261 with 2^-261 folded into V,
so the x nodes' weights carry 2^261.  fold_dense is the dense route's sums term by term, fold_dft the three transforms."""

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
ROOT_2_28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904      # gnark-crypto's 2^28-th root of unity
K261 = pow(2, 261, R)


def inv(x):
    return pow(x % R, R - 2, R)


def table_order(n):
    """quot_digit_index of kernels.hpp: the coset index at table position t"""
    L = n.bit_length() - 1
    Lhi = (L + 1) // 2
    Llo = L - Lhi
    quarter = (1 << Lhi) // 4
    return [(((t >> 2) % quarter + (t & 3) * quarter) << Llo) + (t >> 2) // quarter for t in range(n)]


class Domain:
    def __init__(self, n):
        self.n = n
        L = n.bit_length() - 1
        assert n == 1 << L and L >= 2
        self.zeta = pow(ROOT_2_28, 1 << (27 - L), R)
        self.w = self.zeta * self.zeta % R
        assert pow(self.zeta, n, R) == R - 1
        self.x = [pow(self.w, i, R) for i in range(n)]
        self.y = [self.zeta * xi % R for xi in self.x]


def weights(dom, m, perm):
    """lam[q] of the dropped position m - 1 + q; node[p], weight[p] of the fold's 2m - 1 columns (k_qf_weights)"""
    n, x, y = dom.n, dom.x, dom.y
    yj = [y[perm[pos]] for pos in range(m - 1, n)]

    def zs(e):
        p = 1
        for s in range(m, n):
            p = p * (e - x[s]) % R
        return p

    def zj(e, skip=None):
        p = 1
        for q, t in enumerate(yj):
            if q != skip:
                p = p * (e - t) % R
        return p
    lam = [2 * n * zs(e) % R * inv(e * zj(e, q)) % R for q, e in enumerate(yj)]
    node = x[:m] + [y[perm[pos]] for pos in range(m - 1)]
    weight = [e * zj(e) % R * inv(2 * n * zs(e)) % R * (K261 if p < m else 1) % R for p, e in enumerate(node)]
    return lam, node, weight, yj


def fold_dense(dom, m, perm, u, v):
    """(U', V') exponents: U'_i = U_i + sum_J lam_j weight_i / (y_j - x_i) V_j,  V'_pos = V_pos + sum_J lam_j weight / (y_j - y_i) V_j"""
    lam, node, weight, yj = weights(dom, m, perm)
    sums = [weight[p] * sum(lam[q] * inv(yj[q] - node[p]) % R * v[m - 1 + q] for q in range(len(yj))) % R for p in range(2 * m - 1)]
    return [(u[i] + sums[i]) % R for i in range(m)], [(v[pos] + sums[m + pos]) % R for pos in range(m - 1)]


def g_hat(n, k):
    """the transform of g(d) = 1 / (w^d - 1), g(0) = 0, in closed form: sum_d g(d) w^(dk)"""
    half = inv(2)
    return ((n + 1) * half - k) % R if k else (1 - n) * half % R


def fold_dft(dom, m, perm, u, v):
    """the same by three transforms of size n (k_quot_bases.hip, "the fold as three group transforms")"""
    n, w, zeta = dom.n, dom.w, dom.zeta
    lam, node, weight, _ = weights(dom, m, perm)
    W = [0] * n
    for q in range(n - m + 1):
        W[perm[m - 1 + q]] = lam[q] * v[m - 1 + q] % R
    dft = lambda a: [sum(pow(w, -i * k % n, R) * a[k] for k in range(n)) % R for i in range(n)]      # k_qb_stage's direction
    What = dft(W)
    Ax = dft([pow(zeta, n - 1 - k, R) * What[(k + 1) % n] % R for k in range(n)])
    Gy = dft([g_hat(n, k) * What[k] % R for k in range(n)])
    half = inv(2)
    U2 = [(u[i] - weight[i] * half % R * Ax[-i % n]) % R for i in range(m)]
    V2 = [(v[pos] + weight[m + pos] * inv(n * node[m + pos]) % R * Gy[-perm[pos] % n]) % R for pos in range(m - 1)]
    return U2, V2


# ---- BN254 G1 (y^2 = x^3 + 3, generator (1, 2)) for the device test: k G as 64 B big-endian X | Y --------------------------------------------
def _jac_dbl(p):
    x, y, z = p
    if not z:
        return p
    a, b = x * x % P, y * y % P
    c = b * b % P
    d = 2 * ((x + b) * (x + b) - a - c) % P
    e = 3 * a % P
    x3 = (e * e - 2 * d) % P
    return x3, (e * (d - x3) - 8 * c) % P, 2 * y * z % P


def _jac_add(p, q):
    if not p[2]:
        return q
    if not q[2]:
        return p
    x1, y1, z1 = p
    x2, y2, z2 = q
    z1z1, z2z2 = z1 * z1 % P, z2 * z2 % P
    u1, u2 = x1 * z2z2 % P, x2 * z1z1 % P
    s1, s2 = y1 * z2 * z2z2 % P, y2 * z1 * z1z1 % P
    if u1 == u2:
        return _jac_dbl(p) if s1 == s2 else (1, 1, 0)
    h, r = (u2 - u1) % P, (s2 - s1) % P
    hh = h * h % P
    hhh, vv = h * hh % P, u1 * hh % P
    x3 = (r * r - hhh - 2 * vv) % P
    return x3, (r * (vv - x3) - s1 * hhh) % P, z1 * z2 * h % P


_G_ROWS = None      # [window of 4 bits][digit]: digit * 16^window * G


def g1_mul(k):
    """k G -> (64 B big-endian X | Y, infinity flag): the hook's point format"""
    global _G_ROWS
    if _G_ROWS is None:
        _G_ROWS, base = [], (1, 2, 1)
        for _ in range(64):
            row = [(1, 1, 0)]
            for _ in range(15):
                row.append(_jac_add(row[-1], base))
            _G_ROWS.append(row)
            base = _jac_add(row[15], base)
    k %= R
    acc = (1, 1, 0)
    for j in range(64):
        acc = _jac_add(acc, _G_ROWS[j][(k >> (4 * j)) & 15])
    if not acc[2]:
        return bytes(64), 1
    zi = pow(acc[2], P - 2, P)
    x, y = acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P
    assert (y * y - x * x * x - 3) % P == 0
    return x.to_bytes(32, "big") + y.to_bytes(32, "big"), 0
