// TEST HOOK gsc_debug_assemble (include/libprove.h): the proof assembly kernels on a caller's MSM sums and scalars, without a key, a circuit or an
// algorithm.  The sums are built from affine points and a scale each, and the production launchers run in the order and with the argument
// conventions of engine_prove.hip (stage_upload, stage_witness, stage_early_sums / stage_msms, stage_assembly): flags zeroed over their padded
// words; launch_prep_rs; launch_points_to_affine_be (bit 8) and launch_challenge_from_point for a commitment; launch_fin_scalarmul, or
// launch_fin_scalarmul_few on glv_split's halves (or on the caller's, to reach the rest of the kernel's contract); launch_points_to_affine_be (bit 16); launch_fin_combine.  No production kernel is changed or
// copied for it: the two kernels here build an XYZZ sum from its affine form and turn tmp back into affine coordinates (debug_ops.hpp's sum_out).
// tests/test_gpu_assemble.py is the caller.
#include "assemble_debug.hpp"
#include "engine_impl.hpp"
#include "msm_dev.hpp"
#include "debug_ops.hpp"
#include "glv.hpp"

namespace gsc {
using namespace bn254;

namespace {

// sums[i] = (x l^2, y l^3, l^2, l^3) for the canonical affine point pts[i] and the scale lam[i] != 0; four zeros for inf[i] != 0
template <class F>
__global__ __launch_bounds__(64) void k_debug_assemble_in(const fe* pts, const uint8_t* inf, const fe* lam, size_t n, fe* sums) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Curve9<F>::store_xyzz(sums + i * (4 * F::WORDS), dbg::curve_xyzz<F>(pts + i * (2 * F::WORDS), inf[i] != 0, lam + i * F::WORDS));
}

// out[i] = sums[i] as canonical little-endian x, y; inf[i] = 1 and zeros for the point at infinity
__global__ __launch_bounds__(64) void k_debug_assemble_out(const fe* sums, size_t n, fe* out, uint8_t* inf) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) dbg::sum_out<Fp29f>(sums, i, out, inf);
}

[[noreturn]] void refuse(const std::string& why) { throw std::runtime_error("gsc_debug_assemble: " + why); }

struct PointSet { const char* name; const uint8_t *pts, *inf, *lam; int words; bool given() const { return pts && inf && lam; } };

bool below_le(const uint8_t* le, const uint8_t* mod_be) {      // 32 little-endian bytes < the big-endian modulus
    for (int i = 0; i < 32; i++) { const uint8_t v = le[31 - i]; if (v != mod_be[i]) return v < mod_be[i]; }
    return false;
}

// what the host can decide: everything but "the point is on the curve / in the subgroup"
void check(const gsc_debug_assemble_args& a, const PointSet* sets) {
    if (a.batch < 1 || a.batch > 256) refuse("the batch is 1 .. 256 columns");
    if (a.nproofs > 32 || a.nproofs > a.batch) refuse("nproofs beyond the latency kernel's 32 / the batch");
    if (a.n_wires > 4096) refuse("more than 4096 wires");
    if (a.fill > 255) refuse("fill is one byte");
    if (!a.rs || !a.out || !a.flags || !a.tmp || !a.tmp_inf || !a.W) refuse("a buffer is missing: rs, out, flags, tmp, tmp_inf, W");
    if (a.nproofs && !a.glv) refuse("a buffer is missing: glv");
    if (a.mask && !a.mask_out) refuse("a buffer is missing: mask_out");
    if (a.glv_in && !a.nproofs) refuse("glv_in without nproofs: only the latency kernel reads halves");
    for (size_t i = 0; a.glv_in && i < 2 * (size_t)a.nproofs; i++) {
        uint32_t w[11]; memcpy(w, a.glv_in + 44 * i, 44);
        if (w[4] >> 2 || w[9] >> 2 || w[10] > 3) refuse("glv_in with a magnitude of 2^130 or more, or neg above 3");
    }
    for (int i = 0; i < 5; i++) if (!sets[i].given()) refuse(std::string("a buffer is missing: ") + sets[i].name);
    for (int i = 5; i < 8; i++) if ((sets[i].pts || sets[i].inf || sets[i].lam) && !sets[i].given()) refuse(std::string("a buffer is missing: ") + sets[i].name);
    if (sets[6].given() != sets[7].given()) refuse("a buffer is missing: D and Pok come together");
    if (sets[6].given() && (!a.cpts || !a.commit)) refuse("a buffer is missing: cpts, commit");
    for (size_t i = 0; i < 2 * (size_t)a.batch; i++) if (!below_le(a.rs + 32 * i, kFrModBE)) refuse("a scalar that is not below r");
    if (a.mask) for (size_t i = 0; i < a.batch; i++) if (!below_le(a.mask + 32 * i, kFrModBE)) refuse("a mask that is not below r");
    for (int k = 0; k < 8; k++) {
        const PointSet& ps = sets[k];
        if (!ps.given()) continue;
        const size_t lw = 32 * (size_t)ps.words;
        for (size_t i = 0; i < a.batch; i++) {
            bool zero = true;
            for (size_t q = 0; q < lw; q++) zero = zero && !ps.lam[lw * i + q];
            if (zero) refuse(std::string("a scale that is zero: ") + ps.name);
            for (int w = 0; w < ps.words; w++) if (memcmp(ps.lam + lw * i + 32 * w, kFpModBE, 32) >= 0) refuse(std::string("a scale that is not below p: ") + ps.name);
            if (ps.inf[i]) continue;
            const uint8_t* pt = ps.pts + 2 * lw * i;
            zero = true; for (size_t q = 0; q < 2 * lw; q++) zero = zero && !pt[q];
            if ((pt[0] & 0xC0) || zero) refuse(std::string("a point that is not raw and finite: ") + ps.name);
        }
    }
}

// big-endian values of 32 bytes, in G2 the imaginary part first -> canonical little-endian fe, real part first
void be_to_fe(const uint8_t* be, int words, fe* out) {
    for (int w = 0; w < words; w++) {
        const uint8_t* src = be + 32 * (words - 1 - w);
        for (int l = 0; l < 8; l++) out[w].l[l] = ((uint32_t)src[28 - 4 * l] << 24) | ((uint32_t)src[29 - 4 * l] << 16) | ((uint32_t)src[30 - 4 * l] << 8) | src[31 - 4 * l];
    }
}

// the set's finite points through the production decode (on the curve, in G2 in the subgroup), then one XYZZ sum per column
template <class AffT, class XyzzT>
void build_sums(const PointSet& ps, size_t B, XyzzT* sums, hipStream_t s) {
    using F = typename GroupOf<AffT>::F;
    constexpr int W = F::WORDS;
    const size_t cb = 32 * W;
    KeyPoints raw; size_t nfin = 0;
    std::vector<fe> pts(2 * W * B), lam(W * B);
    for (size_t i = 0; i < B; i++) {
        be_to_fe(ps.lam + cb * i, W, &lam[W * i]);
        if (ps.inf[i]) continue;
        const uint8_t* pt = ps.pts + 2 * cb * i;
        raw.x.insert(raw.x.end(), pt, pt + cb); raw.y.insert(raw.y.end(), pt + cb, pt + 2 * cb);
        be_to_fe(pt, W, &pts[2 * W * i]); be_to_fe(pt + cb, W, &pts[2 * W * i + W]);
        nfin++;
    }
    if (nfin) {
        DevBuf<AffT> dec(nfin);
        std::vector<uint8_t> st;
        if constexpr (W == 1) st = decode_g1_points(raw, dec.p, s); else st = decode_g2_points(raw, dec.p, s);
        for (size_t k = 0; k < nfin; k++) if (st[k] != 0) refuse(std::string("a point that is not on the curve / in the group: ") + ps.name);
    }
    DevBuf<fe> d_pts(pts.size()), d_lam(lam.size()); DevBuf<uint8_t> d_inf(B);
    d_pts.upload(pts.data(), pts.size(), s); d_lam.upload(lam.data(), lam.size(), s); d_inf.upload(ps.inf, B, s);
    hipLaunchKernelGGL(k_debug_assemble_in<F>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, d_pts.p, d_inf.p, d_lam.p, B, reinterpret_cast<fe*>(sums));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));      // (the staging buffers go out of scope)
}

void run(const gsc_debug_assemble_args& a, const PointSet* sets) {
    const size_t B = a.batch, npr = a.nproofs, nw = a.n_wires, flag_bytes = (B + 3) / 4 * 4;
    const bool has_c = sets[5].given(), has_commitment = sets[6].given();
    hipStream_t s = nullptr;
    DevBuf<G1Xyzz> sumA(B), sumB1(B), sumK(B), sumZ(B), sumC(has_c ? B : 0), sumD(has_commitment ? B : 0), sumPok(has_commitment ? B : 0), tmp(2 * B);
    DevBuf<G2Xyzz> sumB2(B);
    build_sums<G1Aff, G1Xyzz>(sets[0], B, sumA.p, s); build_sums<G1Aff, G1Xyzz>(sets[1], B, sumB1.p, s);
    build_sums<G1Aff, G1Xyzz>(sets[2], B, sumK.p, s); build_sums<G1Aff, G1Xyzz>(sets[3], B, sumZ.p, s);
    build_sums<G2Aff, G2Xyzz>(sets[4], B, sumB2.p, s);
    if (has_c) build_sums<G1Aff, G1Xyzz>(sets[5], B, sumC.p, s);
    if (has_commitment) { build_sums<G1Aff, G1Xyzz>(sets[6], B, sumD.p, s); build_sums<G1Aff, G1Xyzz>(sets[7], B, sumPok.p, s); }

    DevBuf<uint8_t> d_rs(64 * B), d_out(256 * B), d_flags(flag_bytes), d_mask_in(a.mask ? 32 * B : 0), d_cpts(has_commitment ? 128 * B : 0);
    DevBuf<fe> d_W((nw + 4) * B), d_mask(B), d_commit(B);
    DevBuf<GlvSplit> d_glv(npr ? 2 * npr : 0);
    std::vector<GlvSplit> h_glv(2 * npr);
    // stage_upload
    d_rs.upload(a.rs, 64 * B, s);
    for (size_t i = 0; i < npr; i++) for (int role = 0; role < 2; role++) {
        GlvSplit& g = h_glv[2 * i + role];
        if (a.glv_in) { const uint8_t* src = a.glv_in + 44 * (2 * i + role); memcpy(g.k1, src, 20); memcpy(g.k2, src + 20, 20); memcpy(&g.neg, src + 40, 4); continue; }
        uint32_t w[8]; memcpy(w, a.rs + 64 * i + (role == 0 ? 32 : 0), 32);
        if (!glv_split(w, g)) throw std::runtime_error("internal: scalar split out of range");
    }
    if (npr) d_glv.upload(h_glv.data(), 2 * npr, s);
    HIP_CHECK(hipMemsetAsync(d_flags.p, 0, d_flags.bytes(), s));
    // what the engine's buffers hold from earlier calls is the caller's fill here; tmp's unwritten columns (latency kernel) are the point at infinity
    HIP_CHECK(hipMemsetAsync(d_out.p, (int)a.fill, d_out.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_W.p, (int)a.fill, d_W.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_mask.p, (int)a.fill, d_mask.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_commit.p, (int)a.fill, d_commit.bytes(), s));
    HIP_CHECK(hipMemsetAsync(tmp.p, 0, tmp.bytes(), s));
    if (has_commitment) HIP_CHECK(hipMemsetAsync(d_cpts.p, (int)a.fill, d_cpts.bytes(), s));
    // stage_witness
    if (a.mask) d_mask_in.upload(a.mask, 32 * B, s);
    launch_prep_rs(d_rs.p, d_W.p, nw, B, a.mask ? d_mask_in.p : nullptr, d_mask.p, s);
    if (has_commitment) {
        launch_points_to_affine_be(sumD.p, B, d_cpts.p, d_flags.p, 8, s);
        launch_challenge_from_point(d_cpts.p, d_commit.p, B, s);
    }
    // stage_early_sums / stage_msms
    if (npr) launch_fin_scalarmul_few(sumA.p, sumB1.p, d_glv.p, B, npr, d_out.p, d_flags.p, tmp.p, s);
    else launch_fin_scalarmul(sumA.p, sumB1.p, d_rs.p, B, d_out.p, d_flags.p, tmp.p, s);
    if (has_commitment) launch_points_to_affine_be(sumPok.p, B, d_cpts.p + 64 * B, d_flags.p, 16, s);
    // stage_assembly
    launch_fin_combine(sumB2.p, sumK.p, sumZ.p, has_c ? sumC.p : nullptr, tmp.p, B, d_out.p, d_flags.p, s);
    HIP_CHECK(hipGetLastError());
    // ---- results ----
    DevBuf<fe> d_taff(4 * B); DevBuf<uint8_t> d_tinf(2 * B);
    hipLaunchKernelGGL(k_debug_assemble_out, dim3((unsigned)((2 * B + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const fe*>(tmp.p), 2 * B, d_taff.p, d_tinf.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(a.out, d_out.p, 256 * B, hipMemcpyDeviceToHost, s));
    std::vector<uint8_t> h_flags(flag_bytes);
    HIP_CHECK(hipMemcpyAsync(h_flags.data(), d_flags.p, flag_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(a.tmp, d_taff.p, d_taff.bytes(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(a.tmp_inf, d_tinf.p, 2 * B, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(a.W, d_W.p + nw * B, 4 * B * sizeof(fe), hipMemcpyDeviceToHost, s));
    if (a.mask) HIP_CHECK(hipMemcpyAsync(a.mask_out, d_mask.p, B * sizeof(fe), hipMemcpyDeviceToHost, s));
    if (has_commitment) {
        HIP_CHECK(hipMemcpyAsync(a.cpts, d_cpts.p, 128 * B, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(a.commit, d_commit.p, B * sizeof(fe), hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    memcpy(a.flags, h_flags.data(), B);
    for (size_t i = 0; i < 2 * npr; i++) { memcpy(a.glv + 44 * i, h_glv[i].k1, 20); memcpy(a.glv + 44 * i + 20, h_glv[i].k2, 20); memcpy(a.glv + 44 * i + 40, &h_glv[i].neg, 4); }
}

}  // namespace

void debug_assemble(int device, const gsc_debug_assemble_args& a) {
    const PointSet sets[8] = {{"A", a.a_pts, a.a_inf, a.a_lam, 1}, {"B1", a.b1_pts, a.b1_inf, a.b1_lam, 1}, {"K", a.k_pts, a.k_inf, a.k_lam, 1}, {"Z", a.z_pts, a.z_inf, a.z_lam, 1},
                              {"B2", a.b2_pts, a.b2_inf, a.b2_lam, 2}, {"C", a.c_pts, a.c_inf, a.c_lam, 1}, {"D", a.d_pts, a.d_inf, a.d_lam, 1}, {"Pok", a.pok_pts, a.pok_inf, a.pok_lam, 1}};
    check(a, sets);      // every refusal the host can decide comes before a device is asked for
    use_device(device);
    run(a, sets);
}

}  // namespace gsc
