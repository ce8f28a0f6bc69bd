"""The quotient fold (k_quot_fold.hip) on Python integers: no device, no library.

Rows m .. n-1 of a and b are zero, so A and B vanish on S = {w^i : m <= i < n} and P = A B = Z_S^2 Q with deg Q <= 2m - 2: the n coset
values d_i = P(zeta w^i) are determined by the m values c_i and any m - 1 of them.  The dropped ones (J) are Lagrange combinations of the
rest over the nodes {x_i} + {y_i : i in I}; their bases are folded into the others:  U'_i = U_i + sum_J alpha_ji V_j,
V'_i = V_i + sum_J beta_ji V_j.  The group is modelled by exponents: Z_k = tau^k (tau^n - 1) / delta mod r.

The engine's conventions are modelled too: its d is d_i 2^261 (with 2^-261 folded into V), its c the plain value, so alpha carries 2^261.
"""
import random

import pytest

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ROOT_2_28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904      # gnark-crypto's 2^28-th root of unity
K261 = pow(2, 261, R)


def inv(x):
    return pow(x % R, R - 2, R)


def prod(xs):
    p = 1
    for x in xs:
        p = p * x % R
    return p


def interpolate(points, values):
    """coefficients of the polynomial of degree < len(points) through (points, values)"""
    k = len(points)
    full = [1]                                          # prod (X - p)
    for p in points:
        full = [((full[i - 1] if i else 0) - p * (full[i] if i < len(full) else 0)) % R for i in range(len(full) + 1)]
    out = [0] * k
    for p, v in zip(points, values):
        q = [0] * k                                     # full / (X - p) by synthetic division
        carry = 0
        for i in range(k, 0, -1):
            carry = (full[i] + carry * p) % R
            q[i - 1] = carry
        scale = v * inv(sum(q[i] * pow(p, i, R) for i in range(k))) % R
        for i in range(k):
            out[i] = (out[i] + scale * q[i]) % R
    return out


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


class Model:
    def __init__(self, n, m, rng):
        self.n, self.m = n, m
        L = n.bit_length() - 1
        self.zeta = pow(ROOT_2_28, 1 << (27 - L), R)    # primitive 2n-th root: zeta^n = -1
        self.w = self.zeta * self.zeta % R
        assert pow(self.zeta, n, R) == R - 1
        self.x = [pow(self.w, i, R) for i in range(n)]
        self.y = [self.zeta * xi % R for xi in self.x]
        tau, delta = rng.randrange(2, R), rng.randrange(2, R)
        self.Z = [pow(tau, k, R) * (pow(tau, n, R) - 1) % R * inv(delta) % R for k in range(n - 1)] + [0]      # n - 1 points; the n-th is infinity
        a = [rng.randrange(R) if i < m else 0 for i in range(n)]
        b = [rng.randrange(R) if i < m else 0 for i in range(n)]
        self.c = [a[i] * b[i] % R for i in range(n)]
        A, B, C = interpolate(self.x, a), interpolate(self.x, b), interpolate(self.x, self.c)
        P = [0] * (2 * n - 1)
        for i, ai in enumerate(A):
            for j, bj in enumerate(B):
                P[i + j] = (P[i + j] + ai * bj) % R
        self.d = [evaluate(P, yi) for yi in self.y]
        num = [(P[i] - (C[i] if i < n else 0)) % R for i in range(2 * n - 1)]      # (P - C) / (X^n - 1)
        H = [0] * (n - 1)
        for i in range(2 * n - 2, n - 1, -1):
            H[i - n] = num[i]
            num[i - n] = (num[i - n] + num[i]) % R
        assert all(v == 0 for v in num[:n])
        self.target = sum(h * z for h, z in zip(H, self.Z)) % R
        i2n = inv(2 * n)
        self.U = [i2n * sum(pow(self.w, -i * k % n, R) * self.Z[k] for k in range(n)) % R for i in range(n)]
        # the engine's V: 2^-261 folded in; its scalars are d_i 2^261
        self.V = [-i2n * inv(K261) * sum(pow(self.zeta, -k % (2 * n), R) * pow(self.w, -i * k % n, R) * self.Z[k] for k in range(n)) % R for i in range(n)]
        self.dE = [di * K261 % R for di in self.d]

    def unfolded(self):
        return (sum(self.c[i] * self.U[i] for i in range(self.m)) + sum(self.dE[i] * self.V[i] for i in range(self.n))) % R

    def fold(self, J):
        """(U', V') for the dropped coset indices J, by the formulas of the issue"""
        n, m, x, y = self.n, self.m, self.x, self.y
        assert len(J) == n - m + 1
        I = [i for i in range(n) if i not in set(J)]
        S = x[m:]
        ZS = lambda t: prod(t - s for s in S)
        ZJ = lambda t: prod(t - y[j] for j in J)
        dZJ = lambda j: prod(y[j] - y[k] for k in J if k != j)
        lam = {j: ZS(y[j]) ** 2 * (-2 * n * pow(y[j], n - 1, R) * inv(ZS(y[j]) * dZJ(j))) % R for j in J}
        mu = [inv(ZS(x[i]) ** 2 * (2 * n * pow(x[i], n - 1, R) * inv(ZS(x[i]) * ZJ(x[i])))) for i in range(m)]
        nu = {i: inv(ZS(y[i]) ** 2 * (-2 * n * pow(y[i], n - 1, R) * inv(ZS(y[i]) * ZJ(y[i])))) for i in I}
        # the forms the device kernel evaluates (x^n = 1, y^n = -1 used)
        i2n = inv(2 * n)
        assert all(lam[j] == 2 * n * ZS(y[j]) * inv(y[j] * dZJ(j)) % R for j in J)
        assert all(mu[i] == x[i] * ZJ(x[i]) % R * i2n * inv(ZS(x[i])) % R for i in range(m))
        assert all(nu[i] == y[i] * ZJ(y[i]) % R * i2n * inv(ZS(y[i])) % R for i in I)
        # alpha multiplies the plain c_i and lands on the engine's V_j, which expects d_j 2^261; beta is homogeneous in d
        U2 = [(self.U[i] + sum(lam[j] * mu[i] % R * inv(y[j] - x[i]) % R * K261 % R * self.V[j] for j in J)) % R for i in range(m)]
        V2 = {i: (self.V[i] + sum(lam[j] * nu[i] % R * inv(y[j] - y[i]) % R * self.V[j] for j in J)) % R for i in I}
        return I, U2, V2


def table_order(n):
    """quot_digit_index of kernels.hpp: the coset index at table position t"""
    L = n.bit_length() - 1
    Lhi = (L + 1) // 2
    Llo = L - Lhi
    quarter = (1 << Lhi) // 4
    return [(((t >> 2) % quarter + (t & 3) * quarter) << Llo) + (t >> 2) // quarter for t in range(n)]


CASES = [(n, m) for n in (16, 32) for m in (1, 2, n // 2 + 1, n - 5, n - 1, n)]


@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("scattered", [False, True], ids=["suffix", "scattered"])
def test_fold_identity(n, m, scattered):
    rng = random.Random(1000 * n + 10 * m + scattered)
    mod = Model(n, m, rng)
    assert mod.unfolded() == mod.target                 # the identity of k_quot_bases.hip
    order = table_order(n)
    assert sorted(order) == list(range(n))
    J = rng.sample(range(n), n - m + 1) if scattered else order[m - 1:]      # the suffix of the Z set's table order
    I, U2, V2 = mod.fold(J)
    assert len(I) == m - 1
    folded = (sum(mod.c[i] * U2[i] for i in range(m)) + sum(mod.dE[i] * V2[i] for i in I)) % R
    assert folded == mod.target
    # U' and V' are a pair: U' with the old V counts the dropped bases' share twice
    mixed = (sum(mod.c[i] * U2[i] for i in range(m)) + sum(mod.dE[i] * mod.V[i] for i in range(n))) % R
    assert mixed != mod.target
