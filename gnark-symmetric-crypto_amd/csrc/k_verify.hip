// GPU Groth16 verifier kernels (gsc_verify_init / gsc_verify_raw / VerifyBatch): one thread per proof or per table entry.  The
// arithmetic is the per-thread code of verify_dev.hpp; this file only maps it onto threads.
//
// Replaces, on the GPU, groth16.Verify of the reference's verifier library (libraries/verifier/impl/verifiers.go:50-152), which
// libverify.so (verifier.cpp) implements on the CPU with identical verdicts.
#include "verify_kernels.hpp"
#include "verify_dev.hpp"

namespace gsc {
using namespace vfy;

namespace {

// key points: n1 compressed G1 (32 bytes) then n2 compressed G2 (64 bytes, with the subgroup test); st: 0 finite, 1 infinity, -1 bad
__global__ __launch_bounds__(64) void k_verify_key_points(const uint8_t* g1, size_t n1, const uint8_t* g2, size_t n2, VP1* o1, VP2* o2, int8_t* st) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    // slots of 64 / 128 bytes: a raw point fills its slot, a compressed one the first half (verify_dev.hpp decode_g1_key / decode_g2_key)
    if (i < n1) st[i] = (int8_t)decode_g1_key(g1 + 64 * i, o1[i]);
    else if (i < n1 + n2) st[i] = (int8_t)decode_g2_key(g2 + 128 * (i - n1), o2[i - n1]);
}
// window tables: entry (w, v) for w < nwin; desc[w] = (first K index, shift | subset << 16)
__global__ __launch_bounds__(64) void k_verify_tables(const VP1* K, const uint32_t* desc, size_t nwin, VP1* table) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= nwin * 256) return;
    const size_t w = i / 256;
    const uint32_t first = desc[2 * w], sh = desc[2 * w + 1];
    table[i] = table_entry((sh >> 16) != 0, K, first, sh & 0xFFFF, (uint32_t)(i % 256));
}
__global__ __launch_bounds__(64) void k_verify_lines(const VP2* q, size_t n, Line* out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n && !q[i].inf) lines_of(q[i], out + kLineSteps * i);
}
__global__ __launch_bounds__(64) void k_verify_prep(KeyDev k, const uint8_t* proofs, const uint8_t* win, const uint8_t* pre, ProofDev* pd, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    ProofDev p;
    p.ok = 0;
    if (pre[i]) prep_one(k, proofs + kProofSlot * i, win + kWindows * i, p);
    pd[i] = p;
}
__global__ __launch_bounds__(64) void k_verify_pairing(KeyDev k, const ProofDev* pd, uint8_t* verdict, F12* fout, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    verdict[i] = pair_one(k, pd[i], fout ? fout + i : nullptr) ? 1 : 0;
}
// test hook: uncompressed big-endian points (G1 x|y, G2 x.a1|x.a0|y.a1|y.a0; all-zero = infinity) -> ProofDev with A = P, B = Q
__global__ __launch_bounds__(64) void k_verify_debug_points(const uint8_t* g1, const uint8_t* g2, ProofDev* pd, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    ProofDev p;
    const uint8_t *a = g1 + 64 * i, *b = g2 + 128 * i;
    uint32_t oa = 0, ob = 0;
    for (int j = 0; j < 64; j++) oa |= a[j];
    for (int j = 0; j < 128; j++) ob |= b[j];
    bool ok = true;
    p.A.inf = oa == 0; p.B.inf = ob == 0;
    p.A.x = p.A.y = F::zero(); p.B.x = p.B.y = F2::zero();
    if (oa) ok = fp_from_be(a, false, p.A.x) && fp_from_be(a + 32, false, p.A.y) && ok;
    if (ob) ok = fp_from_be(b, false, p.B.x.a1) && fp_from_be(b + 32, false, p.B.x.a0) && fp_from_be(b + 64, false, p.B.y.a1) && fp_from_be(b + 96, false, p.B.y.a0) && ok;
    p.ok = ok;
    pd[i] = p;
}
// F12 -> 12 x 32-byte big-endian canonical coefficients, coefficient 2 i + j = component j (of 1, u) of the w^i coefficient
__global__ __launch_bounds__(64) void k_verify_f12_bytes(const F12* f, uint8_t* out, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < 12; c++) {
        const e2& v = f[i].c[c / 2];
        const fe w = F::pack(F::from_mont(c & 1 ? v.a1 : v.a0));
        uint8_t* o = out + 384 * i + 32 * c;
        for (int j = 0; j < 8; j++) for (int b = 0; b < 4; b++) o[4 * j + b] = (uint8_t)(w.l[7 - j] >> (24 - 8 * b));
    }
}
// test hook: n affine points `stride` bytes apart from src on (VP1, or VP2 when g2) -> canonical big-endian X | Y (G2: X.A1 | X.A0 | Y.A1 | Y.A0)
// and an infinity byte behind them (zero coordinates for the point at infinity), `ostride` bytes apart; live (optional, int32 words
// `lstride` bytes apart): point i is converted only where its word is not zero, its bytes stay as they were otherwise
__global__ __launch_bounds__(64) void k_verify_point_bytes(const uint8_t* src, size_t stride, int g2, const uint8_t* live, size_t lstride, uint8_t* out, size_t ostride, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (live && !*(const int32_t*)(live + lstride * i)) return;
    uint8_t* o = out + ostride * i;
    e1 c[4]; int nc; bool inf;
    if (g2) { const VP2& p = *(const VP2*)(src + stride * i); c[0] = p.x.a1; c[1] = p.x.a0; c[2] = p.y.a1; c[3] = p.y.a0; nc = 4; inf = p.inf != 0; }
    else { const VP1& p = *(const VP1*)(src + stride * i); c[0] = p.x; c[1] = p.y; c[2] = c[3] = F::zero(); nc = 2; inf = p.inf != 0; }
    for (int k = 0; k < nc; k++) {
        const fe w = F::pack(F::from_mont(c[k]));
        for (int j = 0; j < 8; j++) for (int b = 0; b < 4; b++) o[32 * k + 4 * j + b] = inf ? 0 : (uint8_t)(w.l[7 - j] >> (24 - 8 * b));
    }
    o[32 * nc] = inf ? 1 : 0;
}

unsigned blocks(size_t n) { return (unsigned)((n + 63) / 64); }

}  // namespace

void launch_verify_key_points(const uint8_t* g1, size_t n1, const uint8_t* g2, size_t n2, VP1* o1, VP2* o2, int8_t* st, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_key_points, dim3(blocks(n1 + n2)), dim3(64), 0, s, g1, n1, g2, n2, o1, o2, st);
}
void launch_verify_tables(const VP1* K, const uint32_t* desc, size_t nwin, VP1* table, hipStream_t s) {
    if (nwin) hipLaunchKernelGGL(k_verify_tables, dim3(blocks(nwin * 256)), dim3(64), 0, s, K, desc, nwin, table);
}
void launch_verify_lines(const VP2* q, size_t n, Line* out, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_lines, dim3(blocks(n)), dim3(64), 0, s, q, n, out);
}
void launch_verify_prep(const KeyDev& k, const uint8_t* proofs, const uint8_t* win, const uint8_t* pre, ProofDev* pd, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_verify_prep, dim3(blocks(n)), dim3(64), 0, s, k, proofs, win, pre, pd, n);
}
void launch_verify_pairing(const KeyDev& k, const ProofDev* pd, uint8_t* verdict, F12* fout, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_verify_pairing, dim3(blocks(n)), dim3(64), 0, s, k, pd, verdict, fout, n);
}
void launch_verify_debug_points(const uint8_t* g1, const uint8_t* g2, ProofDev* pd, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_verify_debug_points, dim3(blocks(n)), dim3(64), 0, s, g1, g2, pd, n);
}
void launch_verify_f12_bytes(const F12* f, uint8_t* out, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_verify_f12_bytes, dim3(blocks(n)), dim3(64), 0, s, f, out, n);
}
void launch_verify_point_bytes(const void* src, size_t stride, bool g2, const void* live, size_t lstride, uint8_t* out, size_t ostride, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_verify_point_bytes, dim3(blocks(n)), dim3(64), 0, s, (const uint8_t*)src, stride, g2 ? 1 : 0, (const uint8_t*)live, lstride, out, ostride, n);
}

}  // namespace gsc
