// Key ceremony, second phase (gsc_setup_contribute / gsc_setup_verify_contribution): the device side.
//   k_scale_points<P, S>  one thread per point: out = k P.  S says where k comes from: UniformScalar, ONE scalar shared by every thread (x, 1/x
//                       or the Schnorr nonce of a contribution; uniform loads), or PerPointScalar, a scalar of its own for every point (a
//                       contribution to a powers file, DESIGN.md §3.12: the rows k_fr_powers wrote, word-major, so a wave's loads coalesce).
//                       k is toxic waste, so the ladder takes the same steps whatever its bits are: every step is one doubling and
//                       one exact addition of P that is always computed (madd<true>: it handles acc = infinity and acc = +-P), and the bit
//                       only selects, limb by limb, which of the two values goes on.  The current word of k sits in a register and the next
//                       is loaded when the (uniform) step counter crosses a word; there is no private array indexed by a runtime value.
//                       One inversion per thread makes the result affine.
//   k_fr_powers         row i = m x^(first + i) mod r, canonical, word-major: the scalars of one section of a powers file.  The index is
//                       public, so the square-and-multiply over its bits branches; x, m and the rows are toxic waste (secret buffers).
//   k_points_be<P>      decoded points -> raw big-endian bytes
//   k_phase2_rlc<P>, _sum<P>  a verifier's two random combinations sum rho_i a_i, sum rho_i b_i (a contribution's check: Z and K before and
//                       after; a powers file's check, srs_gpu.cpp: a vector and itself shifted by one, in G1 and in G2): the batched
//                       verifier's 128-bit scalar multiplication (verify_batch_dev.hpp g1_mul; the same walk over G2) and block sum
//                       (block_sum.hpp), then one block per sum.
// Points are the verifier's decoded images (verify_dev.hpp VP1 / VP2), as k_verify_key_points leaves them.
#include "phase2_kernels.hpp"
#include "block_sum.hpp"

namespace gsc {
using namespace vfy;

namespace {

constexpr int kThreads = 64;

template <class P> struct GroupOfPoint;
template <> struct GroupOfPoint<VP1> { using F = bn254::Fp29f; using C = bn254::G1x; };
template <> struct GroupOfPoint<VP2> { using F = bn254::Fp2x; using C = bn254::G2x; };
template <class P> using XyzzOf = bn254::Xyzz9<typename GroupOfPoint<P>::F>;      // VP1: G1X, VP2: G2X

// m all ones: a, m zero: b
DEVFN fe9 pick(uint32_t m, const fe9& a, const fe9& b) {
    fe9 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = (int32_t)(((uint32_t)a.l[i] & m) | ((uint32_t)b.l[i] & ~m));
    return r;
}
DEVFN fe9x2 pick(uint32_t m, const fe9x2& a, const fe9x2& b) { return fe9x2{pick(m, a.a0, b.a0), pick(m, a.a1, b.a1)}; }
template <class F> DEVFN bn254::Xyzz9<F> pick(uint32_t m, const bn254::Xyzz9<F>& a, const bn254::Xyzz9<F>& b) {
    bn254::Xyzz9<F> r;
    r.x = pick(m, a.x, b.x); r.y = pick(m, a.y, b.y); r.zz = pick(m, a.zz, b.zz); r.zzz = pick(m, a.zzz, b.zzz);
    r.inf = (((uint32_t)a.inf & m) | ((uint32_t)b.inf & ~m)) != 0;
    return r;
}

DEVFN VP1 affine_of(const bn254::Xyzz9<bn254::Fp29f>& p) { return g1_affine(p); }
DEVFN VP2 affine_of(const bn254::Xyzz9<bn254::Fp2x>& p) { return g2_affine(p); }

// where a ladder's scalar comes from: word w (of eight, little-endian) of point i's scalar
struct UniformScalar {
    const uint32_t* k;
    DEVFN uint32_t word(int w, size_t) const { return k[w]; }
};
struct PerPointScalar {
    const uint32_t* k; size_t n;      // word-major over the n points: k[w * n + i]
    DEVFN uint32_t word(int w, size_t i) const { return k[(size_t)w * n + i]; }
};

template <class P, class S>
__global__ __launch_bounds__(kThreads) void k_scale_points(const P* in, size_t n, const S k, P* out) {
    using G = GroupOfPoint<P>;
    using C = typename G::C;
    const size_t i = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (i >= n) return;
    const P p = in[i];
    if (p.inf) { out[i] = p; return; }      // which points of a key are infinity is public
    const bn254::Aff9<typename G::F> a{p.x, p.y};
    bn254::Xyzz9<typename G::F> acc = C::infinity();
    uint32_t w = k.word(7, i);
    for (int b = 253; b >= 0; b--) {        // k < r < 2^254
        if ((b & 31) == 31) w = k.word(b >> 5, i);      // b is uniform: no branch on the scalar
        acc = C::dbl(acc);
        const bn254::Xyzz9<typename G::F> sum = C::template madd<true>(acc, a);
        const uint32_t m = 0u - ((w >> (b & 31)) & 1u);
        acc = pick(m, sum, acc);
    }
    out[i] = affine_of(acc);
}

// rows[w * n + i] = word w of m x^(first + i) mod r (canonical); x, m: eight little-endian words each, canonical, below r
__global__ __launch_bounds__(kThreads) void k_fr_powers(const uint32_t* x, const uint32_t* m, uint64_t first, size_t n, uint32_t* rows) {
    using Fr = bn254::Fr;
    const size_t i = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (i >= n) return;
    bn254::fe xc, mc;
    for (int j = 0; j < 8; j++) { xc.l[j] = x[j]; mc.l[j] = m[j]; }
    const bn254::fe xm = Fr::to_mont(xc);
    const uint64_t e = first + i;           // public: the position in the file
    bn254::fe acc = Fr::one();
    for (int b = 63 - __clzll(e | 1); b >= 0; b--) {
        acc = Fr::sqr(acc);
        if ((e >> b) & 1) acc = Fr::mul(acc, xm);
    }
    const bn254::fe v = Fr::mul(acc, mc);   // Montgomery x^e times canonical m: canonical m x^e
    for (int j = 0; j < 8; j++) rows[(size_t)j * n + i] = v.l[j];
}

DEVFN void be32_of(const e1& v, uint8_t* o) {
    const fe w = F::pack(F::from_mont(v));
    for (int j = 0; j < 8; j++) for (int b = 0; b < 4; b++) o[4 * j + b] = (uint8_t)(w.l[7 - j] >> (24 - 8 * b));
}
DEVFN void point_be(const VP1& p, uint8_t* o) { be32_of(p.x, o); be32_of(p.y, o + 32); }
DEVFN void point_be(const VP2& p, uint8_t* o) { be32_of(p.x.a1, o); be32_of(p.x.a0, o + 32); be32_of(p.y.a1, o + 64); be32_of(p.y.a0, o + 96); }

template <class P>
__global__ __launch_bounds__(kThreads) void k_points_be(const P* p, size_t n, uint8_t* out, uint8_t* inf) {
    constexpr size_t W = sizeof(P) == sizeof(VP1) ? 64 : 128;
    const size_t i = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (i >= n) return;
    const P v = p[i];
    inf[i] = v.inf ? 1 : 0;
    if (v.inf) { for (size_t j = 0; j < W; j++) out[W * i + j] = 0; return; }
    point_be(v, out + W * i);
}

// rho P over 128 bits, exact double-and-add: the batched verifier's g1_mul, and the same walk over G2
DEVFN G1X rlc_mul(const VP1& p, const uint32_t* k) { return g1_mul(p, k, 128); }
DEVFN G2X rlc_mul(const VP2& p, const uint32_t* k) {
    G2X acc = bn254::G2x::infinity();
    if (p.inf) return acc;
    const bn254::Aff9<bn254::Fp2x> a{p.x, p.y};
    for (int i = 127; i >= 0; i--) {
        acc = bn254::G2x::dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1) acc = bn254::G2x::madd<true>(acc, a);
    }
    return acc;
}

template <class P>
__global__ __launch_bounds__(kThreads) void k_phase2_rlc(const P* a, const P* b, const uint32_t* rho, size_t n, XyzzOf<P>* part) {
    using C = typename GroupOfPoint<P>::C;
    __shared__ XyzzOf<P> red[kThreads];
    const size_t i = blockIdx.x * (size_t)kThreads + threadIdx.x;
    const bool ok = i < n;
    uint32_t r[4];
    for (int w = 0; w < 4; w++) r[w] = ok ? rho[4 * i + w] : 0;
    const XyzzOf<P> sa = block_sum<kThreads>(ok ? rlc_mul(a[i], r) : C::infinity(), red);
    const XyzzOf<P> sb = block_sum<kThreads>(ok ? rlc_mul(b[i], r) : C::infinity(), red);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = sa; part[2 * blockIdx.x + 1] = sb; }
}
// block j: sums[j] = the sum of part[2 b + j] over the nblk blocks of k_phase2_rlc
template <class P>
__global__ __launch_bounds__(kThreads) void k_phase2_rlc_sum(const XyzzOf<P>* part, size_t nblk, P* sums) {
    using C = typename GroupOfPoint<P>::C;
    __shared__ XyzzOf<P> red[kThreads];
    XyzzOf<P> acc = C::infinity();
    for (size_t b = threadIdx.x; b < nblk; b += kThreads) acc = C::add(acc, part[2 * b + blockIdx.x]);
    const XyzzOf<P> total = block_sum<kThreads>(acc, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = affine_of(total);
}

unsigned blocks(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

void launch_scale_points(const VP1* in, size_t n, const uint32_t* k, VP1* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL((k_scale_points<VP1, UniformScalar>), dim3(blocks(n)), dim3(kThreads), 0, s, in, n, UniformScalar{k}, out);
}
void launch_scale_points(const VP2* in, size_t n, const uint32_t* k, VP2* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL((k_scale_points<VP2, UniformScalar>), dim3(blocks(n)), dim3(kThreads), 0, s, in, n, UniformScalar{k}, out);
}
void launch_scale_points_each(const VP1* in, size_t n, const uint32_t* rows, VP1* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL((k_scale_points<VP1, PerPointScalar>), dim3(blocks(n)), dim3(kThreads), 0, s, in, n, PerPointScalar{rows, n}, out);
}
void launch_scale_points_each(const VP2* in, size_t n, const uint32_t* rows, VP2* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL((k_scale_points<VP2, PerPointScalar>), dim3(blocks(n)), dim3(kThreads), 0, s, in, n, PerPointScalar{rows, n}, out);
}
void launch_fr_powers(const uint32_t* x, const uint32_t* m, uint64_t first, size_t n, uint32_t* rows, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_fr_powers, dim3(blocks(n)), dim3(kThreads), 0, s, x, m, first, n, rows);
}
void launch_points_be(const VP1* p, size_t n, uint8_t* out, uint8_t* inf, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_points_be<VP1>, dim3(blocks(n)), dim3(kThreads), 0, s, p, n, out, inf);
}
void launch_points_be(const VP2* p, size_t n, uint8_t* out, uint8_t* inf, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_points_be<VP2>, dim3(blocks(n)), dim3(kThreads), 0, s, p, n, out, inf);
}
size_t phase2_rlc_blocks(size_t n) { return blocks(n); }
template <class P> static void launch_rlc_of(const P* a, const P* b, const uint32_t* rho, size_t n, XyzzOf<P>* part, P* sums, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_phase2_rlc<P>, dim3(blocks(n)), dim3(kThreads), 0, s, a, b, rho, n, part);
    hipLaunchKernelGGL(k_phase2_rlc_sum<P>, dim3(2), dim3(kThreads), 0, s, (const XyzzOf<P>*)part, (size_t)blocks(n), sums);
}
void launch_phase2_rlc(const VP1* a, const VP1* b, const uint32_t* rho, size_t n, G1X* part, VP1* sums, hipStream_t s) { launch_rlc_of<VP1>(a, b, rho, n, part, sums, s); }
void launch_phase2_rlc(const VP2* a, const VP2* b, const uint32_t* rho, size_t n, G2X* part, VP2* sums, hipStream_t s) { launch_rlc_of<VP2>(a, b, rho, n, part, sums, s); }

}  // namespace gsc
