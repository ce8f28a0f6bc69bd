"""The quotient fold as three group transforms (k_quot_bases.hip) on Python integers: no device, no library.

The dense route adds sum_J alpha_ji V_j to U_i and sum_J beta_ji V_j to V_i term by term; the transform route gets both families of sums from
W^_k = sum_J w^(-jk) lam_j V_j:  the x nodes through y^n - x^n = -2 = (y - x) sum_k y^(n-1-k) x^k, the coset nodes through the closed-form
transform of g(d) = 1 / (w^d - 1).  Here both run on exponents (quot_fold_model.py), with the engine's 2^261 conventions in the weights, and must
agree exactly; the dense sums themselves are tied to the fold's defining property by test_quot_fold_host.py's polynomial model."""
import random

import pytest

import quot_fold_model as qm
from quot_fold_model import R

SIZES = (16, 32, 64)


def _perm(kind, n, rng):
    if kind == "identity":
        return list(range(n))
    if kind == "table":
        return qm.table_order(n)                       # the engine's: J is the suffix of the Z set's table order
    p = list(range(n))
    rng.shuffle(p)                                     # J scattered over the coset
    return p


@pytest.mark.parametrize("n", SIZES)
def test_closed_form_of_g_hat_equals_its_defining_sum(n):
    dom = qm.Domain(n)
    g = [0] + [qm.inv(dom.x[d] - 1) for d in range(1, n)]
    for k in range(n):
        assert qm.g_hat(n, k) == sum(g[d] * pow(dom.w, d * k % n, R) for d in range(n)) % R, k


@pytest.mark.parametrize("kind", ["identity", "table", "scattered"])
@pytest.mark.parametrize("n,m", [(n, m) for n in SIZES for m in (2, n // 2, n // 2 + 1, n - 1, n)])
def test_three_transforms_equal_the_dense_sums(n, m, kind):
    rng = random.Random(100 * n + m + len(kind))
    dom, perm = qm.Domain(n), _perm(kind, n, rng)
    u, v = [rng.randrange(R) for _ in range(m)], [rng.randrange(R) for _ in range(n)]
    U2, V2 = qm.fold_dense(dom, m, perm, u, v)
    assert len(U2) == m and len(V2) == m - 1
    assert (U2, V2) == qm.fold_dft(dom, m, perm, u, v)
    assert U2 != u                                     # the dropped bases weigh on every U'


@pytest.mark.parametrize("n,m", [(16, 9), (32, 27)])
def test_engine_conventions_the_dense_model_is_the_fold_of_the_polynomial_model(n, m):
    # the weights (2^261 on the x nodes, 2^-261 inside V) against test_quot_fold_host.py's Model, whose fold is checked against sum_k H_k Z_k
    from test_quot_fold_host import Model
    rng = random.Random(n + m)
    mod, perm = Model(n, m, rng), qm.table_order(n)
    dom = qm.Domain(n)
    u, v = mod.U[:m], [mod.V[perm[pos]] for pos in range(n)]
    I, U2, V2 = mod.fold([perm[pos] for pos in range(m - 1, n)])
    mine_U, mine_V = qm.fold_dft(dom, m, perm, u, v)
    assert mine_U == U2 and mine_V == [V2[perm[pos]] for pos in range(m - 1)]
    folded = (sum(mod.c[i] * mine_U[i] for i in range(m)) + sum(mod.dE[perm[pos]] * mine_V[pos] for pos in range(m - 1))) % R
    assert folded == mod.target


def test_a_wrong_wrap_or_a_wrong_g_hat_0_would_show():
    # the model notices what the device test is there to catch: W^ read at k instead of (k + 1) mod n, or g^_0 taken from the k > 0 formula
    n, m = 16, 9
    rng = random.Random(5)
    dom, perm = qm.Domain(n), qm.table_order(n)
    u, v = [rng.randrange(R) for _ in range(m)], [rng.randrange(R) for _ in range(n)]
    want = qm.fold_dense(dom, m, perm, u, v)
    keep = qm.g_hat
    try:
        qm.g_hat = lambda n_, k: ((n_ + 1) * qm.inv(2) - k) % R
        assert qm.fold_dft(dom, m, perm, u, v)[0] == want[0] and qm.fold_dft(dom, m, perm, u, v)[1] != want[1]
    finally:
        qm.g_hat = keep
    assert qm.fold_dft(dom, m, perm, u, v) == want
