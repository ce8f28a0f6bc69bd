// InitAlgorithm-time: the quotient bases pk.G1.Z of the proving key, once more in EVALUATION form.
//
// groth16.Prove ends the quotient with sum_k H_k Z_k over the COEFFICIENTS of H (reference libraries/prover/impl/provers.go:148,216;
// gnark backend/groth16/bn254 computeH + the Z multi-exponentiation — SURVEY.md §8(a) a7, a9).  With the identities of k_ntt.hip
//   H = (S - D) / 2,   S = the interpolation of c on the n-th roots of unity,   D = the interpolation of d_i = A(zeta w^i) B(zeta w^i)
//   on the coset zeta * (roots of unity), zeta^n = -1,
// the sum is linear in the VALUES c_i and d_i:
//   sum_k H_k Z_k = sum_i c_i U_i + sum_i d_i V_i,     U_i =  (1 / 2n) sum_k w^(-ik) Z_k,     V_i = -(1 / 2n) sum_k zeta^(-k) w^(-ik) Z_k,
// so the prover needs neither the inverse transform of c nor the one of d (two of its six transforms): c is what the solver wrote
// (three quarters zero, nearly all of the rest +-1: a flat MSM set like the wire sets), d feeds the windowed kernel with the bases
// V_i instead of Z_k.  Same group element, hence the same proof bytes.  U and V are discrete Fourier transforms of the key's points —
// "in the exponent": n log n / 2 butterflies whose twiddle products are scalar multiplications — computed here once per key.
// The kernels' d comes out in the NTT kernels' 2^261 Montgomery domain (d_i * 2^261 mod r as a canonical integer): that constant
// is folded into V as well.
#include "kernels.hpp"
#include "bn254_fp29.hpp"
#include "verify_dev.hpp"
#include "group_idft.hpp"

namespace gsc {
using namespace bn254;

namespace {

__device__ __forceinline__ fe9 qb_to_fp29(const fe& old_mont) { return Fp29::to_mont(Fp29::unpack(Fp::from_mont(old_mont))); }
__device__ __forceinline__ fe qb_from_fp29(const fe9& m) { return Fp::to_mont(Fp29::pack(Fp29::from_mont(m))); }

__device__ __forceinline__ fe qb_fr_pow(const fe& a, uint32_t e) {
    fe acc = Fr::one(); bool started = false;
    for (int i = 31; i >= 0; i--) {
        if (started) acc = Fr::sqr(acc);
        if ((e >> i) & 1) { acc = started ? Fr::mul(acc, a) : a; started = true; }
    }
    return acc;
}

// the primitive 2n-th root of unity the quotient kernels use (k_init.hip k_ntt_constants): gnark-crypto's 2^28-th root (SURVEY.md
// App. I; canonical, 8 little-endian words) squared 27 - L times
__device__ __forceinline__ fe qb_zeta(int L) {
    fe c; const uint32_t w[8] = {0x725b19f0u, 0x9bd61b6eu, 0x41112ed4u, 0x402d111eu, 0x8ef62abcu, 0x00e0a7ebu, 0xa58a7e85u, 0x2a3c09f0u};
    for (int i = 0; i < 8; i++) c.l[i] = w[i];
    fe z = Fr::to_mont(c);
    for (int t = 0; t < 27 - L; t++) z = Fr::sqr(z);
    return z;
}

// k * P for a canonical scalar k (8 little-endian words); exact group law throughout (init-time: clarity over speed)
// F: the coordinate field (Fp29f: G1, Fp2x: G2)
template <class F>
__device__ __noinline__ Xyzz9<F> qb_scalar_mul(const Xyzz9<F>& P, const fe& k) {
    using C = Curve9<F>;
    Xyzz9<F> acc = C::infinity();
    int top = 255;
    while (top >= 0 && !((k.l[top >> 5] >> (top & 31)) & 1u)) top--;
    for (int i = top; i >= 0; i--) {
        acc = C::dbl(acc);
        if ((k.l[i >> 5] >> (i & 31)) & 1u) acc = C::add(acc, P);
    }
    return acc;
}

// tw[e] = w^-e as a canonical integer, e < n/2
__global__ __launch_bounds__(64) void k_qb_twiddles(const fe* omega_inv, uint32_t half_n, fe* tw) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= half_n) return;
    tw[e] = Fr::from_mont(qb_fr_pow(*omega_inv, e));
}

// Y[pos] = lambda_k * Zfile[pos], k = bitrev(pos): the key stores Z in bit-reversed order (Zfile[pos] = Z_bitrev(pos), n - 1 points;
// position n - 1 is the missing top coefficient: the point at infinity).  mode 0 (U): lambda = 1 / 2n;
// mode 1 (V): lambda = -zeta^-k / (2n * 2^261).  zeta: the primitive 2n-th root with zeta^2 = w (k_init.hip derives the same one).
__global__ __launch_bounds__(64) void k_qb_load(const Aff<Fp>* zfile, const uint8_t* status, uint32_t n, int L, int mode,
                                                 const fe* omega_inv, const fe* n_inv, fe* Y) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    fe* dst = Y + 4 * (size_t)pos;
    if (pos == n - 1 || status[pos] == 2) { G1x::store_xyzz(dst, G1x::infinity()); return; }
    const uint32_t k = __brev(pos) >> (32 - L);
    fe lam = Fr::mul(*n_inv, Fr::inv(Fr::from_u32(2)));
    if (mode == 1) {
        const fe zeta_inv = Fr::mul(qb_zeta(L), *omega_inv);                      // zeta^-1 = zeta * w^-1
        const fe r261_inv = Fr::inv(qb_fr_pow(Fr::from_u32(2), 261));
        lam = Fr::neg(Fr::mul(Fr::mul(lam, r261_inv), qb_fr_pow(zeta_inv, k)));
    }
    const Aff9<Fp29f> P{qb_to_fp29(zfile[pos].x), qb_to_fp29(zfile[pos].y)};
    G1x::store_xyzz(dst, qb_scalar_mul(G1x::from_aff(P), Fr::from_mont(lam)));
}

// One decimation-in-time stage s (bit-reversed input, natural output after stage L - 1): pairs (j, j + 2^s) inside blocks of
// 2^(s+1), twiddle w^-((j mod 2^s) << (L-1-s)).  Over either group (F: Fp29f for G1, Fp2x for G2; a point takes 4 F::WORDS elements of Y):
// the quotient bases and the fold transform G1, the Lagrange bases of a powers file (launch_group_idft) both.
template <class F>
__global__ __launch_bounds__(64) void k_qb_stage(fe* Y, uint32_t half_n, int L, int s, const fe* tw) {
    using C = Curve9<F>;
    constexpr size_t W = 4 * F::WORDS;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= half_n) return;
    const uint32_t half = 1u << s, lo = t & (half - 1), j = ((t >> s) << (s + 1)) + lo, e = lo << (L - 1 - s);
    fe* pu = Y + W * (size_t)j; fe* pv = Y + W * (size_t)(j + half);
    const Xyzz9<F> u = C::load_xyzz(pu);
    Xyzz9<F> v = C::load_xyzz(pv);
    if (e) v = qb_scalar_mul(v, tw[e]);
    C::store_xyzz(pu, C::add(u, v));
    v.y = F::norm(F::neg(v.y));
    C::store_xyzz(pv, C::add(u, v));
}

// The inputs of launch_group_idft: Y[bitrev(k)] = (1 / n) in[k] for decoded key points (verify_dev.hpp VP1 / VP2; infinity stays infinity)
template <class P, class F>
__global__ __launch_bounds__(64) void k_gt_load(const P* in, uint32_t n, int L, fe* Y) {
    using C = Curve9<F>;
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    fe* dst = Y + 4 * F::WORDS * (size_t)(L ? __brev(k) >> (32 - L) : 0u);
    const P p = in[k];
    if (p.inf) { C::store_xyzz(dst, C::infinity()); return; }
    const fe n_inv = Fr::from_mont(Fr::inv(Fr::from_u32(n)));
    C::store_xyzz(dst, qb_scalar_mul(C::from_aff(Aff9<F>{p.x, p.y}), n_inv));
}
// ... and its outputs: natural order, affine, as decoded key points again
__device__ __forceinline__ vfy::VP1 gt_affine(const Xyzz9<Fp29f>& p) { return vfy::g1_affine(p); }
__device__ __forceinline__ vfy::VP2 gt_affine(const Xyzz9<Fp2x>& p) { return vfy::g2_affine(p); }
template <class P, class F>
__global__ __launch_bounds__(64) void k_gt_finish(const fe* Y, uint32_t n, P* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gt_affine(Curve9<F>::load_xyzz(Y + 4 * F::WORDS * (size_t)i));
}

// XYZZ -> affine bases in the layout the table builders take (8 x 32-bit Montgomery images); status 2 = the point at infinity
// perm (optional): out[i] = point perm[i] — the order the windowed MSM wants its bases in (kernels.hpp quot_digit_index)
__global__ __launch_bounds__(64) void k_qb_finish(const fe* Y, uint32_t n, const uint32_t* perm, Aff<Fp>* out, uint8_t* status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Xyzz9<Fp29f> p = G1x::load_xyzz(Y + 4 * (size_t)(perm ? perm[i] : i));
    if (p.inf) { status[i] = 2; out[i] = Aff<Fp>{Fp::zero(), Fp::zero()}; return; }
    const Aff9<Fp29f> a = G1x::to_aff(p);
    out[i] = Aff<Fp>{qb_from_fp29(a.x), qb_from_fp29(a.y)};
    status[i] = 0;
}

// ---- the fold: bases of the coset values that the domain's zero padding makes redundant ---------------------------------------------------
// Rows m .. n-1 of a and b are zero, so A and B vanish on S = {w^i : m <= i < n}: P = A B = Z_S^2 Q with deg Q <= 2m - 2, and the n values
// d_i = P(y_i), y_i = zeta w^i, are determined by the m values c_i = P(x_i), x_i = w^i, and any m - 1 of them.  The others (J, n - m + 1
// indices; I: the rest) are Lagrange combinations over the nodes {x_i : i < m} + {y_i : i in I},
//   d_j = sum_{i<m} alpha_ji c_i + sum_{i in I} beta_ji d_i,   alpha_ji = lambda_j mu_i / (y_j - x_i),   beta_ji = lambda_j nu_i / (y_j - y_i),
//   lambda_j = 2n Z_S(y_j) / (y_j Z_J'(y_j)),   mu_i = x_i Z_J(x_i) / (2n Z_S(x_i)),   nu_i = y_i Z_J(y_i) / (2n Z_S(y_i))
// (Z_S, Z_J: the vanishing polynomials of S and of {y_j : j in J}; x^n = 1 and y^n = -1 used), so their bases move into the rest, once
// per key:  U'_i = U_i + sum_J alpha_ji V_j,  V'_i = V_i + sum_J beta_ji V_j.  The engine's d is d_i 2^261 with 2^-261 folded into V:
// beta is homogeneous in d, alpha carries the factor 2^261.  tests/test_quot_fold_host.py checks the algebra on integers.
//
// Columns p of the fold: p < m the node x_p (base U_p), p >= m the node y of table position p - m (base V at that position); J = the table
// positions m - 1 .. n - 1 (perm: position -> coset index).

// pw[k] = w^k, k < n; yj[q] = the coset point of the dropped table position m - 1 + q (Montgomery)
__global__ __launch_bounds__(64) void k_qf_powers(const fe* omega, const uint32_t* perm, uint32_t n, int L, uint32_t m, fe* pw, fe* yj) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    pw[k] = qb_fr_pow(*omega, k);
    if (k >= m - 1) yj[k - (m - 1)] = Fr::mul(qb_zeta(L), qb_fr_pow(*omega, perm[k]));
}

// One thread per point: t < m the node x_t, then the n coset points in table order.  node[p], weight[p] (mu 2^261 or nu) for the columns,
// lam[q] for the dropped position m - 1 + q.  All Montgomery.
__global__ __launch_bounds__(64) void k_qf_weights(const fe* pw, const uint32_t* perm, uint32_t n, int L, uint32_t m, fe* node, fe* weight, const fe* yj, fe* lam) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m + n) return;
    const fe zeta = qb_zeta(L);
    const bool on_coset = t >= m;
    const uint32_t pos = on_coset ? t - m : 0u, idx = on_coset ? perm[pos] : t;
    const bool dropped = on_coset && pos >= m - 1;
    const fe e = on_coset ? Fr::mul(zeta, pw[idx]) : pw[idx];
    fe zs = Fr::one(), zj = Fr::one();
    for (uint32_t s = m; s < n; s++) zs = Fr::mul(zs, Fr::sub(e, pw[s]));
    for (uint32_t q = m - 1; q < n; q++) if (!(dropped && q == pos)) zj = Fr::mul(zj, Fr::sub(e, yj[q - (m - 1)]));      // (dropped: Z_J'(e))
    const fe two_n = Fr::from_u32(2 * n);
    if (dropped) {
        lam[pos - (m - 1)] = Fr::mul(Fr::mul(two_n, zs), Fr::inv(Fr::mul(e, zj)));
    } else {
        fe w = Fr::mul(Fr::mul(e, zj), Fr::inv(Fr::mul(two_n, zs)));
        if (!on_coset) w = Fr::mul(w, qb_fr_pow(Fr::from_u32(2), 261));
        const uint32_t p = on_coset ? m + pos : t;
        node[p] = e; weight[p] = w;
    }
}

// TEST HOOK: out[i] = a[i] + b[i] as canonical big-endian X | Y (zeros and flag 1 for the point at infinity)
__global__ __launch_bounds__(64) void k_qf_sum_be(const fe* a, const fe* b, uint32_t n, uint8_t* out, uint8_t* flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Xyzz9<Fp29f> p = G1x::add(G1x::load_xyzz(a + 4 * (size_t)i), G1x::load_xyzz(b + 4 * (size_t)i));
    fe xy[2] = {fe{}, fe{}};
    if (!p.inf) { const Aff9<Fp29f> q = G1x::to_aff(p); xy[0] = Fp29::pack(Fp29::from_mont(q.x)); xy[1] = Fp29::pack(Fp29::from_mont(q.y)); }
    flags[i] = p.inf ? 1 : 0;
    for (int c = 0; c < 2; c++) for (int k = 0; k < 32; k++) out[64 * (size_t)i + 32 * c + k] = (uint8_t)(xy[c].l[7 - k / 4] >> (8 * (3 - k % 4)));
}

// ---- the sums as three group transforms ----------------------------------------------------------------------------------------------------
// The fold needs, for every column, a sum over the dropped bases: sum_J lambda_j V_j / (y_j - x_i) for U'_i (i < m) and sum_J lambda_j V_j / (y_j - y_i)
// for V'_i (i in I) — (2m - 1)(n - m + 1) terms taken one by one.  Both sums are structured in the node index:
// with W_j = lambda_j V_j (j in J; the point at infinity elsewhere) and W^_k = sum_j w^(-jk) W_j (one transform of size n),
//   x nodes (i < m):      y^n - x^n = -2 = (y - x) sum_k y^(n-1-k) x^k, hence
//     sum_J W_j / (y_j - x_i) = -1/2 sum_k w^(ik) zeta^(n-1-k) W^_((k+1) mod n);
//   coset nodes (i in I): 1 / (y_j - y_i) = g(j - i) / y_i with g(d) = 1 / (w^d - 1), g(0) = 0 — a cyclic correlation, and
//     g^_k = sum_d g(d) w^(dk) is closed-form, g^_0 = (1 - n) / 2, g^_k = (n + 1) / 2 - k (0 < k < n), hence
//     sum_J W_j / (y_j - y_i) = 1 / (n y_i) sum_k w^(ik) g^_k W^_k.
// The outer sums run in the other direction: k_qb_stage's transform, read at index (-i) mod n.  U'_i = U_i - (weight_i / 2) A^[-i],
// V'_i = V_i + (weight_i / (n y_i)) G^[-i] (weight: mu 2^261 or nu, k_qf_weights): the group elements defined above, whichever way they are summed.
// tests/test_quot_fold_dft_host.py checks the identities on integers.

// cst[0] = w = zeta^2, cst[1] = w^-1 = w^(n-1) (Montgomery): what k_qf_powers and k_qb_twiddles take from the key's domain record
__global__ void k_qfd_consts(int L, fe* cst) {
    if (blockIdx.x || threadIdx.x) return;
    const fe w = Fr::sqr(qb_zeta(L));
    cst[0] = w; cst[1] = qb_fr_pow(w, (1u << L) - 1u);
}

// Y[bitrev(j)] = lambda_q V(position m - 1 + q), j = perm[position]; the point at infinity for the coset indices that stay (and for a dropped V
// that is the point at infinity)
__global__ __launch_bounds__(64) void k_qfd_load(const Aff<Fp>* V, const uint8_t* status, const uint32_t* perm, uint32_t n, int L, uint32_t m, const fe* lam, fe* Y) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    fe* dst = Y + 4 * (size_t)(__brev(perm[pos]) >> (32 - L));
    if (pos < m - 1 || status[pos] == 2) { G1x::store_xyzz(dst, G1x::infinity()); return; }
    const Aff9<Fp29f> P{qb_to_fp29(V[pos].x), qb_to_fp29(V[pos].y)};
    G1x::store_xyzz(dst, qb_scalar_mul(G1x::from_aff(P), Fr::from_mont(lam[pos - (m - 1)])));
}

// The second pass's inputs from W^ (natural order), written in bit-reversed order.  mode 0: zeta^(n-1-k) W^_((k+1) mod n); mode 1: g^_k W^_k
__global__ __launch_bounds__(64) void k_qfd_pointwise(const fe* What, uint32_t n, int L, int mode, fe* Y) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    fe s; uint32_t src = k;
    if (mode == 0) { s = qb_fr_pow(qb_zeta(L), n - 1 - k); src = (k + 1) & (n - 1); }
    else {
        const fe half = Fr::inv(Fr::from_u32(2));
        s = k ? Fr::sub(Fr::mul(Fr::from_u32(n + 1), half), Fr::from_u32(k)) : Fr::neg(Fr::mul(Fr::from_u32(n - 1), half));
    }
    const Xyzz9<Fp29f> p = G1x::load_xyzz(What + 4 * (size_t)src);
    G1x::store_xyzz(Y + 4 * (size_t)(__brev(k) >> (32 - L)), qb_scalar_mul(p, Fr::from_mont(s)));
}

// Column p of the fold (k_qf_weights): p < m the node x_p, out U'_p = U_p - (weight_p / 2) Ax[-p]; p >= m the coset node of table position
// p - m, index i = perm[p - m], out V'_(p-m) = V_(p-m) + (weight_p / (n node_p)) Gy[-i].  Affine in the table builders' layout; status 2 = the point at infinity.
__global__ __launch_bounds__(64) void k_qfd_finish(const fe* Ax, const fe* Gy, const uint32_t* perm, uint32_t n, uint32_t m, const fe* node, const fe* weight,
                                                   const Aff<Fp>* U, const uint8_t* stU, const Aff<Fp>* V, const uint8_t* stV, Aff<Fp>* U2, uint8_t* stU2, Aff<Fp>* V2, uint8_t* stV2) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= 2 * m - 1) return;
    const bool on_coset = p >= m;
    const uint32_t o = on_coset ? p - m : p, i = on_coset ? perm[o] : p, at = (n - i) & (n - 1);
    const fe s = on_coset ? Fr::mul(weight[p], Fr::inv(Fr::mul(Fr::from_u32(n), node[p]))) : Fr::neg(Fr::mul(weight[p], Fr::inv(Fr::from_u32(2))));
    Xyzz9<Fp29f> q = qb_scalar_mul(G1x::load_xyzz((on_coset ? Gy : Ax) + 4 * (size_t)at), Fr::from_mont(s));
    const Aff<Fp>& b = on_coset ? V[o] : U[o];
    if ((on_coset ? stV[o] : stU[o]) != 2) q = G1x::add(q, G1x::from_aff(Aff9<Fp29f>{qb_to_fp29(b.x), qb_to_fp29(b.y)}));
    Aff<Fp>* out = on_coset ? V2 + o : U2 + o; uint8_t* st = on_coset ? stV2 + o : stU2 + o;
    if (q.inf) { *st = 2; *out = Aff<Fp>{Fp::zero(), Fp::zero()}; return; }
    const Aff9<Fp29f> a = G1x::to_aff(q);
    *out = Aff<Fp>{qb_from_fp29(a.x), qb_from_fp29(a.y)};
    *st = 0;
}

// TEST HOOK: affine points between 64 B canonical big-endian X | Y with a flag (1: the point at infinity) and the bases' layout with a status (2)
__global__ __launch_bounds__(64) void k_qfd_from_be(const uint8_t* be, const uint8_t* flags, uint32_t n, Aff<Fp>* out, uint8_t* status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe xy[2] = {fe{}, fe{}};
    for (int c = 0; c < 2; c++) for (int k = 0; k < 32; k++) xy[c].l[7 - k / 4] |= (uint32_t)be[64 * (size_t)i + 32 * c + k] << (8 * (3 - k % 4));
    const bool inf = flags[i] != 0;
    out[i] = inf ? Aff<Fp>{Fp::zero(), Fp::zero()} : Aff<Fp>{Fp::to_mont(xy[0]), Fp::to_mont(xy[1])};
    status[i] = inf ? 2 : 0;
}
__global__ __launch_bounds__(64) void k_qfd_to_be(const Aff<Fp>* in, const uint8_t* status, uint32_t n, uint8_t* be, uint8_t* flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool inf = status[i] == 2;
    fe xy[2] = {fe{}, fe{}};
    if (!inf) { xy[0] = Fp::from_mont(in[i].x); xy[1] = Fp::from_mont(in[i].y); }
    flags[i] = inf ? 1 : 0;
    for (int c = 0; c < 2; c++) for (int k = 0; k < 32; k++) be[64 * (size_t)i + 32 * c + k] = (uint8_t)(xy[c].l[7 - k / 4] >> (8 * (3 - k % 4)));
}

}  // namespace

size_t quot_fold_dft_scratch_bytes(int L, uint32_t m) {
    const size_t n = (size_t)1 << L, nj = n - m + 1;
    return (2 + n + n / 2 + 2 * (2 * (size_t)m - 1) + 2 * nj) * sizeof(fe) + 3 * n * sizeof(G1Xyzz);
}
// the fold's weights: pw (n elements, scratch), node and weight (2m - 1), yj and lam (n - m + 1), all Montgomery
static void launch_quot_fold_weights(const fe* omega, const uint32_t* perm, int L, uint32_t m, fe* pw, fe* node, fe* weight, fe* yj, fe* lam, hipStream_t s) {
    const uint32_t n = 1u << L;
    hipLaunchKernelGGL(k_qf_powers, dim3((n + 63) / 64), dim3(64), 0, s, omega, perm, n, L, m, pw, yj);
    hipLaunchKernelGGL(k_qf_weights, dim3((m + n + 63) / 64), dim3(64), 0, s, pw, perm, n, L, m, node, weight, yj, lam);
}
void launch_quot_fold_dft(int L, uint32_t m, const uint32_t* perm, const G1Aff* U, const uint8_t* stU, const G1Aff* V, const uint8_t* stV,
                          G1Aff* U2, uint8_t* stU2, G1Aff* V2, uint8_t* stV2, void* scratch, hipStream_t s, hipEvent_t weights_done) {
    const uint32_t n = 1u << L, hn = n / 2, nj = n - m + 1, ncols = 2 * m - 1, blocks = (n + 63) / 64;
    fe* cst = static_cast<fe*>(scratch); fe* pw = cst + 2; fe* tw = pw + n; fe* node = tw + hn; fe* weight = node + ncols; fe* yj = weight + ncols; fe* lam = yj + nj;
    fe* What = lam + nj; fe* Ax = What + 4 * (size_t)n; fe* Gy = Ax + 4 * (size_t)n;
    hipLaunchKernelGGL(k_qfd_consts, dim3(1), dim3(64), 0, s, L, cst);
    launch_quot_fold_weights(cst, perm, L, m, pw, node, weight, yj, lam, s);
    if (weights_done) (void)hipEventRecord(weights_done, s);
    hipLaunchKernelGGL(k_qb_twiddles, dim3((hn + 63) / 64), dim3(64), 0, s, cst + 1, hn, tw);
    auto transform = [&](fe* Y) { for (int st = 0; st < L; st++) hipLaunchKernelGGL(k_qb_stage<Fp29f>, dim3((hn + 63) / 64), dim3(64), 0, s, Y, hn, L, st, tw); };
    hipLaunchKernelGGL(k_qfd_load, dim3(blocks), dim3(64), 0, s, reinterpret_cast<const Aff<Fp>*>(V), stV, perm, n, L, m, lam, What);
    transform(What);
    hipLaunchKernelGGL(k_qfd_pointwise, dim3(blocks), dim3(64), 0, s, What, n, L, 0, Ax);
    hipLaunchKernelGGL(k_qfd_pointwise, dim3(blocks), dim3(64), 0, s, What, n, L, 1, Gy);
    transform(Ax);
    transform(Gy);
    hipLaunchKernelGGL(k_qfd_finish, dim3((ncols + 63) / 64), dim3(64), 0, s, Ax, Gy, perm, n, m, node, weight, reinterpret_cast<const Aff<Fp>*>(U), stU,
                       reinterpret_cast<const Aff<Fp>*>(V), stV, reinterpret_cast<Aff<Fp>*>(U2), stU2, reinterpret_cast<Aff<Fp>*>(V2), stV2);
}
void launch_g1_aff_from_be(const uint8_t* be, const uint8_t* flags, size_t n, G1Aff* out, uint8_t* status, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_qfd_from_be, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, be, flags, (uint32_t)n, reinterpret_cast<Aff<Fp>*>(out), status);
}
void launch_g1_aff_to_be(const G1Aff* in, const uint8_t* status, size_t n, uint8_t* be, uint8_t* flags, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_qfd_to_be, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const Aff<Fp>*>(in), status, (uint32_t)n, be, flags);
}

void launch_g1_sum_be(const G1Xyzz* a, const G1Xyzz* b, size_t n, uint8_t* out, uint8_t* flags, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_qf_sum_be, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const fe*>(a), reinterpret_cast<const fe*>(b), (uint32_t)n, out, flags);
}

size_t group_idft_scratch_bytes(int L, bool g2) { const size_t n = (size_t)1 << L; return (2 + n / 2) * sizeof(fe) + n * (g2 ? sizeof(G2Xyzz) : sizeof(G1Xyzz)); }
template <class P, class F> static void group_idft(const P* in, int L, void* scratch, P* out, hipStream_t s) {
    const uint32_t n = 1u << L, hn = n / 2;
    fe* cst = static_cast<fe*>(scratch); fe* tw = cst + 2; fe* Y = tw + hn;
    hipLaunchKernelGGL(k_qfd_consts, dim3(1), dim3(64), 0, s, L, cst);
    hipLaunchKernelGGL(k_qb_twiddles, dim3((hn + 63) / 64), dim3(64), 0, s, cst + 1, hn, tw);
    hipLaunchKernelGGL((k_gt_load<P, F>), dim3((n + 63) / 64), dim3(64), 0, s, in, n, L, Y);
    for (int st = 0; st < L; st++) hipLaunchKernelGGL(k_qb_stage<F>, dim3((hn + 63) / 64), dim3(64), 0, s, Y, hn, L, st, tw);
    hipLaunchKernelGGL((k_gt_finish<P, F>), dim3((n + 63) / 64), dim3(64), 0, s, (const fe*)Y, n, out);
}
void launch_group_idft(const vfy::VP1* in, int L, void* scratch, vfy::VP1* out, hipStream_t s) { group_idft<vfy::VP1, Fp29f>(in, L, scratch, out, s); }
void launch_group_idft(const vfy::VP2* in, int L, void* scratch, vfy::VP2* out, hipStream_t s) { group_idft<vfy::VP2, Fp2x>(in, L, scratch, out, s); }

void launch_quot_bases(const G1Aff* zfile, const uint8_t* zstatus, int L, int mode, const fe* omega_inv, const fe* n_inv,
                       fe* tw, G1Xyzz* scratch, const uint32_t* perm, G1Aff* out, uint8_t* status, hipStream_t s) {
    const uint32_t n = 1u << L, hn = n / 2;
    fe* Y = reinterpret_cast<fe*>(scratch);
    hipLaunchKernelGGL(k_qb_twiddles, dim3((hn + 63) / 64), dim3(64), 0, s, omega_inv, hn, tw);
    hipLaunchKernelGGL(k_qb_load, dim3((n + 63) / 64), dim3(64), 0, s, reinterpret_cast<const Aff<Fp>*>(zfile), zstatus, n, L, mode, omega_inv, n_inv, Y);
    for (int st = 0; st < L; st++) hipLaunchKernelGGL(k_qb_stage<Fp29f>, dim3((hn + 63) / 64), dim3(64), 0, s, Y, hn, L, st, tw);
    hipLaunchKernelGGL(k_qb_finish, dim3((n + 63) / 64), dim3(64), 0, s, Y, n, perm, reinterpret_cast<Aff<Fp>*>(out), status);
}

}  // namespace gsc
