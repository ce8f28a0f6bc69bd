// Slice reductions of the MSMs, wire classification (calibration) and proof assembly.
//
// The gather-accumulate kernels themselves are in k_msm_win.hip; this file holds what follows them in groth16.Prove
// (reference libraries/prover/impl/provers.go:148,216; SURVEY.md §8(a) a9 msmReduceChunk, a12 assembly, App. D).
#include "msm_dev.hpp"
#include "sha256_dev.hpp"

namespace gsc {
using namespace bn254;

namespace {

// one wave sums up to 64 slices of one proof: lanes = slices, butterfly over __shfl_xor
template <class F>
__global__ __launch_bounds__(64) void k_msm_reduce(const fe* partial, size_t nslices, size_t batch, fe* out) {
    using C = Curve9<F>;
    const size_t p = blockIdx.x, grp = blockIdx.y;
    const size_t slice = grp * 64 + threadIdx.x;
    Xyzz9<F> v = slice < nslices ? C::load_xyzz(partial + (slice * batch + p) * (4 * F::WORDS)) : C::infinity();
    v = wave_sum(v);
    if (threadIdx.x == 0) C::store_xyzz(out + (grp * batch + p) * (4 * F::WORDS), v);
}

// the butterfly for calls with a handful of statements: only the columns of the first `npr` proofs of every row of `stride` columns
// (a row = a window; one row for a flat set) — the other columns of the 64-wide batch hold nothing anybody reads
template <class F>
__global__ __launch_bounds__(64) void k_msm_reduce_few(const fe* partial, size_t nslices, size_t cols, fe* out, uint32_t npr, uint32_t stride) {
    using C = Curve9<F>;
    const size_t p = (size_t)(blockIdx.x / npr) * stride + blockIdx.x % npr, grp = blockIdx.y;
    const size_t slice = grp * 64 + threadIdx.x;
    Xyzz9<F> v = slice < nslices ? C::load_xyzz(partial + (slice * cols + p) * (4 * F::WORDS)) : C::infinity();
    v = wave_sum(v);
    if (threadIdx.x == 0) C::store_xyzz(out + (grp * cols + p) * (4 * F::WORDS), v);
}

// the same sum with lanes = proofs: every lane adds up to MSM_REDUCE_FANIN slice partials of ITS proof one after the other.  No lane
// idles (the butterfly above keeps 64 lanes busy for 63 useful additions out of 384), loads are coalesced; used whenever the
// batch is large enough to fill the chip this way (launch_msm_reduce picks).
template <class F>
__global__ __launch_bounds__(64) void k_msm_reduce_seq(const fe* partial, size_t nslices, size_t batch, fe* out) {
    using C = Curve9<F>;
    const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x, grp = blockIdx.y;
    const size_t s0 = grp * MSM_REDUCE_FANIN, s1 = s0 + MSM_REDUCE_FANIN < nslices ? s0 + MSM_REDUCE_FANIN : nslices;
    Xyzz9<F> v = C::load_xyzz(partial + (s0 * batch + p) * (4 * F::WORDS));
    for (size_t sl = s0 + 1; sl < s1; sl++) v = C::add(v, C::load_xyzz(partial + (sl * batch + p) * (4 * F::WORDS)));
    C::store_xyzz(out + (grp * batch + p) * (4 * F::WORDS), v);
}

// ---- calibration: what do the wires of this circuit look like? (engine.hip calibrate) ----
__global__ __launch_bounds__(64) void k_classify_wires(const fe* W, size_t n_wires, size_t batch, const uint32_t* status, uint8_t* cls) {
    const size_t w = blockIdx.x;                 // one wave per wire, lanes = proofs (strided over the batch)
    if (w >= n_wires) return;
    int worst = 0;
    for (size_t p = threadIdx.x; p < batch; p += 64) {
        if (status[p] != 0xFFFFFFFFu) continue;  // a statement the solver rejected says nothing
        fe s = load_fe(W + w * batch + p);
        uint32_t z = 0, o = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) { z |= s.l[i]; o |= s.l[i] ^ FrParams::one(i); }
        if (z == 0 || o == 0) continue;          // 0 or 1
        s = Fr::from_mont(s);
        (void)sign_normalise(s);
        int top = 0;
#pragma unroll
        for (int i = 7; i >= 0; i--) if (!top && s.l[i]) top = 32 * i + 32 - __clz(s.l[i]);
                                                 // (a value that is not 0/1 but has magnitude 1 is -1: class 1)
        worst = top > worst ? top : worst;
    }
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(worst, m); worst = o > worst ? o : worst; }
    if (threadIdx.x == 0) cls[w] = (uint8_t)worst;
}

// ---- proof assembly ----
__device__ __forceinline__ void store_canon(uint8_t* dst, const fe9& mont) {      // canonical integer, 8 little-endian words
    const fe c = Fp29::pack(Fp29::from_mont(mont));
    uint32_t* q = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = c.l[i];
}

// role 0: Ar = sumA, t0 = s * Ar.  role 1: Bs1 = sumB1, t1 = r * Bs1.   tmp[role][proof]
__global__ __launch_bounds__(64) void k_fin_scalarmul(const G1Xyzz* sumA, const G1Xyzz* sumB1, const uint8_t* rs, size_t batch,
                                                       G1Xyzz* tmp, uint8_t* out, uint8_t* flags) {
    const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
    const int role = blockIdx.y;
    if (p >= batch) return;
    const fe* src = reinterpret_cast<const fe*>(role == 0 ? sumA : sumB1) + 4 * p;
    Xyzz9<Fp29f> P = G1x::load_xyzz(src);
    const uint32_t* sc = reinterpret_cast<const uint32_t*>(rs + 64 * p) + (role == 0 ? 8 : 0);   // role 0 uses s, role 1 uses r
    Xyzz9<Fp29f> acc = G1x::infinity();
    if (!P.inf) {
        Aff9<Fp29f> A = G1x::to_aff(P);
        if (role == 0) { store_canon(out + 256 * p, A.x); store_canon(out + 256 * p + 32, A.y); }
        for (int i = 253; i >= 0; i--) {
            acc = G1x::dbl(acc);
            if ((sc[i >> 5] >> (i & 31)) & 1u) acc = G1x::madd<true>(acc, A);
        }
    } else if (role == 0) {
        atomicOr(reinterpret_cast<unsigned int*>(flags) + (p >> 2), 1u << (8 * (p & 3)));
    }
    G1x::store_xyzz(reinterpret_cast<fe*>(tmp) + ((size_t)role * batch + p) * 4, acc);
}
// The same for calls with a handful of statements: one WAVE per (statement, role), and the scalar split in two halves by the curve's
// endomorphism (glv.hpp: k = k1 + k2 lambda, k A = k1 A + k2 phi(A), phi(x, y) = (beta x, y)).  Each half is cut into 26 five-bit
// chunks; lanes 0..25 own the chunks of k1, lanes 32..57 those of k2: all lanes walk the ONE doubling chain 2^i A together (125
// doublings, nothing else on it), a lane keeps 2^(5q) A when the chain passes it (the k2 lanes apply phi: one product), multiplies it
// by its chunk (5 doublings, <= 5 additions) and a butterfly adds the pieces up.  125 doublings + 16 additions on the critical
// path instead of 254 + ~127 (and no field inversion: the chain starts from the XYZZ sum, a third wave turns Ar into the affine
// form the proof carries): the longest serial chain of a single Prove, 2.3 -> 0.68 ms.
__global__ __launch_bounds__(64) void k_fin_scalarmul_few(const G1Xyzz* sumA, const G1Xyzz* sumB1, const GlvSplit* glv, size_t batch,
                                                           G1Xyzz* tmp, uint8_t* out, uint8_t* flags) {
    using F = Fp29f;
    const size_t p = blockIdx.x;
    const int role = blockIdx.y;
    const uint32_t lane = threadIdx.x;
    const fe* src = reinterpret_cast<const fe*>(role == 1 ? sumB1 : sumA) + 4 * p;
    const Xyzz9<F> P = G1x::load_xyzz(src);
    if (role == 2) {                                         // the proof's Ar in affine form: a field inversion (0.28 ms) that the chains need not wait for
        if (lane == 0) {
            if (!P.inf) { const Aff9<F> A = G1x::to_aff(P); store_canon(out + 256 * p, A.x); store_canon(out + 256 * p + 32, A.y); }
            else atomicOr(reinterpret_cast<unsigned int*>(flags) + (p >> 2), 1u << (8 * (p & 3)));
        }
        return;
    }
    const GlvSplit* g = glv + 2 * p + role;                  // role 0: s, role 1: r
    Xyzz9<F> acc = G1x::infinity();
    if (!P.inf) {                                            // (wave-uniform)
        const bool second = lane >= 32;
        const uint32_t q = lane & 31;
        Xyzz9<F> R = P, mine = R;
#pragma unroll 1
        for (uint32_t i = 0; i < 125; i++) {
            R = G1x::dbl(R);
            const bool take = 5 * q == i + 1;
            mine.x = take ? R.x : mine.x; mine.y = take ? R.y : mine.y; mine.zz = take ? R.zz : mine.zz; mine.zzz = take ? R.zzz : mine.zzz;
        }
        {
            fe bw = {};                                      // beta, canonical
            bw.l[0] = 0x77fffffeu; bw.l[1] = 0x57634731u; bw.l[2] = 0xacdb5c4fu; bw.l[3] = 0xd4f263f1u; bw.l[4] = 0xa0d48bacu; bw.l[5] = 0x59e26bceu;
            const fe9 bx = F::mul(mine.x, Fp29::to_mont(Fp29::unpack(bw)));
            mine.x = second ? bx : mine.x;
        }
        const uint32_t* kw = second ? g->k2 : g->k1;
        if ((g->neg >> (second ? 1 : 0)) & 1u) mine.y = F::norm(F::neg(mine.y));
        uint32_t chunk = 0;
        if (q < 26) {
            const uint32_t o = 5 * q, w = o >> 5, sh = o & 31;
            chunk = kw[w] >> sh;
            if (sh > 27) chunk |= kw[w + 1] << (32 - sh);    // (w + 1 <= 4)
            chunk &= 31u;
        }
#pragma unroll 1
        for (int b = 4; b >= 0; b--) {
            acc = G1x::dbl(acc);
            const Xyzz9<F> t = G1x::add(acc, mine);
            if ((chunk >> b) & 1u) acc = t;
        }
        acc = wave_sum(acc);
    }
    if (lane == 0) G1x::store_xyzz(reinterpret_cast<fe*>(tmp) + ((size_t)role * batch + p) * 4, acc);
}
__global__ __launch_bounds__(64) void k_fin_combine(const G2Xyzz* sumB2, const G1Xyzz* sumK, const G1Xyzz* sumZ, const G1Xyzz* sumC, const G1Xyzz* tmp,
                                                     size_t batch, uint8_t* out, uint8_t* flags) {
    const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= batch) return;
    const int role = blockIdx.y;
    uint32_t fl = 0;
    if (role == 0) {
        const fe* K = reinterpret_cast<const fe*>(sumK); const fe* Z = reinterpret_cast<const fe*>(sumZ); const fe* T = reinterpret_cast<const fe*>(tmp);
        Xyzz9<Fp29f> v = G1x::add(G1x::add(G1x::load_xyzz(K + 4 * p), G1x::load_xyzz(Z + 4 * p)), G1x::add(G1x::load_xyzz(T + 4 * p), G1x::load_xyzz(T + 4 * (batch + p))));
        if (sumC) v = G1x::add(v, G1x::load_xyzz(reinterpret_cast<const fe*>(sumC) + 4 * p));
        if (v.inf) fl |= 4;
        else { Aff9<Fp29f> A = G1x::to_aff(v); store_canon(out + 256 * p + 192, A.x); store_canon(out + 256 * p + 224, A.y); }
    } else {
        Xyzz9<Fp2x> v = G2x::load_xyzz(reinterpret_cast<const fe*>(sumB2) + 8 * p);
        if (v.inf) fl |= 2;
        else {
            Aff9<Fp2x> A = G2x::to_aff(v);
            store_canon(out + 256 * p + 64, A.x.a0); store_canon(out + 256 * p + 96, A.x.a1);
            store_canon(out + 256 * p + 128, A.y.a0); store_canon(out + 256 * p + 160, A.y.a1);
        }
    }
    if (fl) atomicOr(reinterpret_cast<unsigned int*>(flags) + (p >> 2), fl << (8 * (p & 3)));
}

__global__ void k_points_to_affine_be(const G1Xyzz* points, size_t batch, uint8_t* out, uint8_t* flags, uint32_t bit) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= batch) return;
    Xyzz9<Fp29f> v = G1x::load_xyzz(reinterpret_cast<const fe*>(points) + 4 * p);
    uint8_t* o = out + 64 * p;
    if (v.inf) { for (int i = 0; i < 64; i++) o[i] = 0; atomicOr(reinterpret_cast<unsigned int*>(flags) + (p >> 2), bit << (8 * (p & 3))); return; }
    Aff9<Fp29f> A = G1x::to_aff(v);
    const fe x = Fp29::pack(Fp29::from_mont(A.x)), y = Fp29::pack(Fp29::from_mont(A.y));
    for (int i = 0; i < 8; i++) {
        const uint32_t xw = x.l[7 - i], yw = y.l[7 - i];
        o[4 * i] = (uint8_t)(xw >> 24); o[4 * i + 1] = (uint8_t)(xw >> 16); o[4 * i + 2] = (uint8_t)(xw >> 8); o[4 * i + 3] = (uint8_t)xw;
        o[32 + 4 * i] = (uint8_t)(yw >> 24); o[32 + 4 * i + 1] = (uint8_t)(yw >> 16); o[32 + 4 * i + 2] = (uint8_t)(yw >> 8); o[32 + 4 * i + 3] = (uint8_t)yw;
    }
}
// ---- commitment challenge on the device (AES-V2): hash_to_field(D) with RFC 9380 expand_message_xmd(SHA-256) ----
// cpts: batch x 64 bytes (uncompressed big-endian X | Y of the commitment, as gnark's Marshal() writes it) -> commit[proof] =
// hash_to_field(cpts[proof], DST "bsb22-commitment") in Montgomery form: 48 xmd bytes as a big-endian integer mod r
// (gnark-crypto fr.Hash).  Replaces a device -> host -> device round trip per batch.
__global__ void k_challenge_from_point(const uint8_t* cpts, fe* commit, size_t batch) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= batch) return;
    const uint32_t* m = reinterpret_cast<const uint32_t*>(cpts + 64 * p);
    uint32_t msg[16], h[12];
    for (int i = 0; i < 16; i++) msg[i] = __builtin_bswap32(m[i]);
    xmd::commitment_xmd(msg, h);
    // 48 bytes = b_1 | first 16 bytes of b_2, big-endian integer mod r by Horner over 32-bit words
    fe acc = Fr::zero();
    const fe w32 = Fr::mul(Fr::from_u32(65536), Fr::from_u32(65536));
    for (int i = 0; i < 12; i++) acc = Fr::add(Fr::mul(acc, w32), Fr::from_u32(h[i]));
    store_fe(commit + p, acc);
}

}  // namespace

// returns the number of partial sums left per proof (1 = done)
template <class XyzzT, class F = typename GroupOf<XyzzT>::F>
static size_t msm_reduce(const XyzzT* partial, size_t nslices, size_t batch, XyzzT* out, hipStream_t s) {
    const size_t groups = msm_reduce_groups(nslices, batch);
    const fe* in = reinterpret_cast<const fe*>(partial); fe* o = reinterpret_cast<fe*>(out);
    if (msm_reduce_by_proof(nslices, batch)) hipLaunchKernelGGL(k_msm_reduce_seq<F>, dim3((unsigned)(batch / 64), (unsigned)groups), dim3(64), 0, s, in, nslices, batch, o);
    else hipLaunchKernelGGL(k_msm_reduce<F>, dim3((unsigned)batch, (unsigned)groups), dim3(64), 0, s, in, nslices, batch, o);
    return groups;
}
template <class XyzzT, class F = typename GroupOf<XyzzT>::F>
static size_t msm_reduce_few(const XyzzT* partial, size_t nslices, size_t cols, size_t stride, size_t npr, XyzzT* out, hipStream_t s) {
    const size_t groups = (nslices + 63) / 64;
    hipLaunchKernelGGL(k_msm_reduce_few<F>, dim3((unsigned)(cols / stride * npr), (unsigned)groups), dim3(64), 0, s, reinterpret_cast<const fe*>(partial), nslices, cols, reinterpret_cast<fe*>(out), (uint32_t)npr, (uint32_t)stride);
    return groups;
}
size_t launch_msm_reduce(const G1Xyzz* partial, size_t nslices, size_t batch, G1Xyzz* out, hipStream_t s) { return msm_reduce(partial, nslices, batch, out, s); }
size_t launch_msm_reduce(const G2Xyzz* partial, size_t nslices, size_t batch, G2Xyzz* out, hipStream_t s) { return msm_reduce(partial, nslices, batch, out, s); }
size_t launch_msm_reduce_few(const G1Xyzz* partial, size_t nslices, size_t cols, size_t stride, size_t npr, G1Xyzz* out, hipStream_t s) { return msm_reduce_few(partial, nslices, cols, stride, npr, out, s); }
size_t launch_msm_reduce_few(const G2Xyzz* partial, size_t nslices, size_t cols, size_t stride, size_t npr, G2Xyzz* out, hipStream_t s) { return msm_reduce_few(partial, nslices, cols, stride, npr, out, s); }
void launch_classify_wires(const fe* W, size_t n_wires, size_t batch, const uint32_t* status, uint8_t* cls, hipStream_t s) {
    if (n_wires) hipLaunchKernelGGL(k_classify_wires, dim3((unsigned)n_wires), dim3(64), 0, s, W, n_wires, batch, status, cls);
}
void launch_points_to_affine_be(const G1Xyzz* points, size_t batch, uint8_t* out, uint8_t* flags, uint32_t bit, hipStream_t s) {
    hipLaunchKernelGGL(k_points_to_affine_be, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, points, batch, out, flags, bit);
}
void launch_challenge_from_point(const uint8_t* cpts, fe* commit, size_t batch, hipStream_t s) {
    hipLaunchKernelGGL(k_challenge_from_point, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, cpts, commit, batch);
}
void launch_fin_scalarmul(const G1Xyzz* sumA, const G1Xyzz* sumB1, const uint8_t* rs, size_t batch, uint8_t* out, uint8_t* flags, G1Xyzz* tmp, hipStream_t s) {
    hipLaunchKernelGGL(k_fin_scalarmul, dim3((unsigned)((batch + 63) / 64), 2), dim3(64), 0, s, sumA, sumB1, rs, batch, tmp, out, flags);
}
void launch_fin_scalarmul_few(const G1Xyzz* sumA, const G1Xyzz* sumB1, const GlvSplit* glv, size_t batch, size_t nproofs, uint8_t* out, uint8_t* flags, G1Xyzz* tmp, hipStream_t s) {
    hipLaunchKernelGGL(k_fin_scalarmul_few, dim3((unsigned)nproofs, 3), dim3(64), 0, s, sumA, sumB1, glv, batch, tmp, out, flags);      // roles: s * Ar, r * Bs1, Ar -> affine
}
void launch_fin_combine(const G2Xyzz* sumB2, const G1Xyzz* sumK, const G1Xyzz* sumZ, const G1Xyzz* sumC, const G1Xyzz* tmp, size_t batch, uint8_t* out, uint8_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_fin_combine, dim3((unsigned)((batch + 63) / 64), 2), dim3(64), 0, s, sumB2, sumK, sumZ, sumC, tmp, batch, out, flags);
}

}  // namespace gsc
