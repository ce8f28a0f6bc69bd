// GPU verifier in libprove.so: gsc_verify_init, gsc_verify_raw, VerifyBatch, gsc_verify_json, gsc_debug_pairing, and the batched check
// gsc_verify_raw_batched, gsc_verify_all, VerifyAll, and the claim-wise batched check gsc_verify_claims, VerifyClaims (include/libprove.h).
// Verdicts are those of libverify.so's Verify (verifier.cpp); the host only checks sizes and packs bytes (verify_common),
// decoding and every curve operation run in k_verify.hip (k_verify_batch.hip for the batched check, k_verify_claims.hip for the claim-wise one).  Each key owns a non-blocking stream and chunk buffers on one device
// (GSC_DEVICE, or the first of GSC_DEVICES); calls on the same key are serialised, and nothing here synchronises the device.
// Routing: a call of at most GSC_VERIFY_FEW_MAX items takes the few-proof kernels (k_verify_few.hip: 8 lanes per proof), larger
// calls the per-thread ones; gsc_verify_last_path reports which.
// The last section is the prover's self-check (prove_check.hpp): the same key object on an engine replica's device, fed by k_check_prep from a
// lane's output buffers on the lane's stream.
#include "../../include/libprove.h"
#include "json.hpp"
#include "verify_common.hpp"
#include "host_ciphers.hpp"
#include "verify_batch_kernels.hpp"
#include "verify_claims_kernels.hpp"
#include "verify_kernels.hpp"
#include "verify_few_kernels.hpp"
#include "prove_check.hpp"
#include "prove_check_kernels.hpp"
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>
#include <sys/random.h>

namespace {

using namespace gsc;
using namespace gsc::vfy;
namespace V = gsc::verify;

constexpr size_t kChunk = 65536;      // proofs per device pass: buffers are allocated once per key, so memory does not grow with n

// Largest call (items of one algorithm) that takes the few-proof kernels unless GSC_VERIFY_FEW_MAX says otherwise: the largest
// measured size at which they beat the per-thread kernels by at least 10 %.
constexpr size_t kFewMaxDefault = 8192;
enum { kPathThread = 1, kPathFew = 2 };
std::atomic<int> g_path_mode{0};      // gsc_debug_verify_path: 0 automatic, else the forced path

// GSC_VERIFY_FEW_MAX: decimal digits only; anything else (a sign, letters, nothing, a value past 64 bits) is refused with a line on
// stderr and the default stands
size_t few_max_setting() {
    const char* v = getenv("GSC_VERIFY_FEW_MAX");
    if (!v) return kFewMaxDefault;
    const size_t len = strlen(v);
    bool digits = len > 0 && len <= 19;
    for (size_t i = 0; digits && i < len; i++) digits = v[i] >= '0' && v[i] <= '9';
    if (!digits) { fprintf(stderr, "GSC_VERIFY_FEW_MAX=%s is not a number of proofs: using %zu\n", v, kFewMaxDefault); return kFewMaxDefault; }
    return (size_t)strtoull(v, nullptr, 10);
}

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
void ck(hipError_t e, const char* what) { if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e)); }

int verify_device() {
    if (const char* dv = getenv("GSC_DEVICES")) { const char* q = dv; while (*q == ',' || *q == ' ') q++; if (*q) return atoi(q); }
    if (const char* d = getenv("GSC_DEVICE")) return atoi(d);
    return 0;
}

thread_local size_t* devbuf_tally = nullptr;      // build_key points this at the key's byte count: what its buffers take of device memory
thread_local int devbuf_device = 0;               // ... and this at the key's device: the same bytes, summed per device (gsc_memory_info)
std::atomic<size_t> g_device_bytes[64];           // what the live keys (the verifier's and the self-check contexts') hold on each device
std::atomic<size_t>& device_bytes(int device) { return g_device_bytes[device >= 0 && device < 64 ? device : 63]; }
struct Tallying { Tallying(size_t* t, int device) { devbuf_tally = t; devbuf_device = device; } ~Tallying() { devbuf_tally = nullptr; } };
template <class T> struct DevBuf {
    T* p = nullptr;
    size_t* tally = nullptr; size_t held = 0; int device = 0;      // the counts this buffer is part of while it lives
    void alloc(size_t n) { ck(hipMalloc(&p, n * sizeof(T) + 1), "hipMalloc"); tally = devbuf_tally; device = devbuf_device; held = n * sizeof(T) + 1; if (tally) { *tally += held; device_bytes(device) += held; } }
    ~DevBuf() { if (p) { (void)hipFree(p); if (tally) { *tally -= held; device_bytes(device) -= held; } } }
};

struct GpuKey {
    int device = 0, algo = 0;
    size_t cap = 0;                      // proofs per device pass: what the chunk buffers below hold (kChunk for a verifier's key)
    size_t bytes = 0;                    // device memory of the key's own buffers (those allocated later included)
    hipStream_t stream = nullptr;
    bool has_commitment = false, fits = false;
    size_t few_max = 0;                  // GSC_VERIFY_FEW_MAX as it stood when the key loaded
    std::atomic<int> last_path{0};
    DevBuf<Line> few_lines;              // kFewChunk x kLineSteps lines of the proofs' own B (180 MB): allocated with the key unless
                                         // GSC_VERIFY_FEW_MAX=0, else by the first call forced onto the path (route_few)
    DevBuf<VP1> K, table, ctable;
    DevBuf<Line> lines;
    KeyDev kd{};
    std::mutex mu;                       // one call at a time on the chunk buffers below
    DevBuf<uint8_t> proofs, win, pre, verdict;
    DevBuf<ProofDev> pd;
    DevBuf<uint32_t> rnd;                // batched check (k_verify_batch.hip): randomizers and the buffers of BatchBufs
    DevBuf<VP1> ra, fixed;
    DevBuf<uint8_t> bok, bflag;
    DevBuf<G1X> part;
    DevBuf<uint64_t> rpart;
    DevBuf<F12> f;
    BatchBufs bufs() const { return BatchBufs{ra.p, bok.p, part.p, rpart.p, fixed.p, f.p, bflag.p}; }
    DevBuf<claims::Part> cparts;         // claim-wise check (k_verify_claims.hip): the buffers of ClaimBufs for one chunk, allocated by
    DevBuf<G1X> cterms;                  // the key's first gsc_verify_claims call (claim_bufs)
    DevBuf<uint32_t> crho;
    DevBuf<VP1> cfixed;
    DevBuf<F12> cpf;
    DevBuf<uint8_t> cflag;
    ClaimBufs claim_bufs() {
        if (!cparts.p) {
            Tallying tallying(&bytes, device);
            cparts.alloc(cap); cterms.alloc(cap * kBatchSums); crho.alloc(cap * 5); cfixed.alloc(cap * kBatchFixed);
            cpf.alloc(cap * kBatchFixed); cflag.alloc(cap);
        }
        return ClaimBufs{cparts.p, cterms.p, crho.p, cfixed.p, cpf.p, cflag.p};
    }
    size_t few_cap() const { return std::min(cap, kFewChunk); }      // proofs the few-proof lines buffer holds
    ~GpuKey() { if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } }
};

std::mutex g_mu;
// never destroyed: a key released at process exit would call into a HIP runtime that may already be gone
std::shared_ptr<GpuKey>* const g_keys = new std::shared_ptr<GpuKey>[3];
bool g_dir_tried = false;
const char* kFiles[3] = {"vk.chacha20", "vk.aes128", "vk.aes256"};

// the key on `device` with chunk buffers for `cap` proofs per pass (a verifier's key: verify_device(), kChunk; a prover replica's check context:
// the replica's device and its largest lane).  point_status (optional, gsc_debug_verify_g1): k_verify_key_points' answer per key point, G1 then G2
std::shared_ptr<GpuKey> build_key(int algo, const uint8_t* b, size_t n, int device, size_t cap, std::vector<int8_t>* point_status = nullptr) {
    V::VkLayout lay; std::string err;
    if (!V::parse_vk_layout(b, n, lay, &err)) { printf("%s\n", err.c_str()); return nullptr; }
    auto k = std::make_shared<GpuKey>();
    Tallying tallying(&k->bytes, device);
    k->device = device; k->cap = cap;
    k->few_max = few_max_setting();
    k->algo = algo;
    ck(hipSetDevice(k->device), "hipSetDevice");
    ck(hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking), "hipStreamCreate");
    hipStream_t s = k->stream;
    // the key's points: G1 alpha, beta1, delta1, K...; G2 beta, gamma, delta (, ped_g, ped_gsn) — each compressed or raw, in slots of
    // 64 / 128 bytes (a compressed point fills the first half of its slot, the rest stays zero)
    std::vector<uint8_t> g1, g2;
    auto add = [&](std::vector<uint8_t>& v, size_t at, size_t cb) {
        const size_t len = V::point_is_raw(b + at) ? 2 * cb : cb, o = v.size();
        v.resize(o + 2 * cb, 0); memcpy(v.data() + o, b + at, len);
    };
    add(g1, lay.alpha, 32); add(g1, lay.g1_beta, 32); add(g1, lay.g1_delta, 32);
    for (size_t at : lay.K) add(g1, at, 32);
    add(g2, lay.beta, 64); add(g2, lay.gamma, 64); add(g2, lay.delta, 64);
    if (lay.has_commitment) { add(g2, lay.ped_g, 64); add(g2, lay.ped_gsn, 64); }
    const size_t n1 = g1.size() / 64, n2 = g2.size() / 128;
    DevBuf<uint8_t> d1, d2; DevBuf<VP1> p1; DevBuf<VP2> p2; DevBuf<int8_t> st;
    d1.alloc(g1.size()); d2.alloc(g2.size()); p1.alloc(n1); p2.alloc(5); st.alloc(n1 + n2);
    ck(hipMemcpyAsync(d1.p, g1.data(), g1.size(), hipMemcpyHostToDevice, s), "copy");
    ck(hipMemcpyAsync(d2.p, g2.data(), g2.size(), hipMemcpyHostToDevice, s), "copy");
    launch_verify_key_points(d1.p, n1, d2.p, n2, p1.p, p2.p, st.p, s);
    std::vector<int8_t> hs(n1 + n2);
    std::vector<VP1> h1(n1); VP2 h2[5];
    ck(hipMemcpyAsync(hs.data(), st.p, hs.size(), hipMemcpyDeviceToHost, s), "copy");
    ck(hipMemcpyAsync(h1.data(), p1.p, n1 * sizeof(VP1), hipMemcpyDeviceToHost, s), "copy");
    ck(hipMemcpyAsync(h2, p2.p, n2 * sizeof(VP2), hipMemcpyDeviceToHost, s), "copy");
    ck(hipStreamSynchronize(s), "key points");
    for (int8_t v : hs) if (v < 0) { printf("vk: bad point\n"); return nullptr; }
    if (point_status) *point_status = hs;
    k->has_commitment = lay.has_commitment;
    k->fits = V::key_fits(algo, lay.K.size(), lay.has_commitment);
    KeyDev& kd = k->kd;
    kd.has_commitment = lay.has_commitment; kd.fits = k->fits;
    kd.alpha = h1[0];
    for (int i = 0; i < 5; i++) kd.qinf[i] = (i < (int)n2) ? h2[i].inf : 1;
    k->lines.alloc(5 * kLineSteps);
    launch_verify_lines(p2.p, n2, k->lines.p, s);
    for (int i = 0; i < 5; i++) kd.lines[i] = k->lines.p + i * kLineSteps;
    k->table.alloc(V::kWindows * 256); k->ctable.alloc(kCommitWindows * 256);
    kd.table = k->table.p; kd.ctable = k->ctable.p;
    if (k->fits) {
        kd.k0 = h1[3];
        std::vector<uint32_t> desc(2 * V::kWindows), cdesc(2 * kCommitWindows);
        for (size_t j = 0; j < V::kWindows; j++) { uint32_t f, sh; V::window_base(algo, j, f, sh); desc[2 * j] = f; desc[2 * j + 1] = sh | (algo == 0 ? 1u << 16 : 0u); }
        for (int j = 0; j < kCommitWindows; j++) { cdesc[2 * j] = (uint32_t)(1 + V::num_public(algo)); cdesc[2 * j + 1] = 8 * j; }
        DevBuf<uint32_t> dd, dc; dd.alloc(desc.size()); dc.alloc(cdesc.size());
        ck(hipMemcpyAsync(dd.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, s), "copy");
        ck(hipMemcpyAsync(dc.p, cdesc.data(), cdesc.size() * 4, hipMemcpyHostToDevice, s), "copy");
        const VP1* Kd = p1.p + 3;     // K[0] is the fourth G1 point of the upload
        launch_verify_tables(Kd, dd.p, V::kWindows, k->table.p, s);
        if (lay.has_commitment) launch_verify_tables(Kd, dc.p, kCommitWindows, k->ctable.p, s);
        ck(hipStreamSynchronize(s), "key tables");
    }
    ck(hipStreamSynchronize(s), "key lines");
    k->proofs.alloc(cap * kProofSlot); k->win.alloc(cap * V::kWindows); k->pre.alloc(cap); k->verdict.alloc(cap); k->pd.alloc(cap);
    const size_t nblk = batch_blocks(cap);
    k->rnd.alloc(cap * kRandWords); k->ra.alloc(cap); k->fixed.alloc(kBatchFixed); k->bok.alloc(cap); k->bflag.alloc(1);
    k->part.alloc(nblk * kBatchSums); k->rpart.alloc(nblk * 4); k->f.alloc(cap + kBatchFixed);
    if (k->few_max) k->few_lines.alloc(k->few_cap() * kLineSteps);
    return k;
}

void load_dir_once() {      // like libverify: keys from GSC_VK_DIR on first use (g_mu held)
    if (g_dir_tried) return;
    g_dir_tried = true;
    const char* dir = getenv("GSC_VK_DIR"); if (!dir) return;
    for (int a = 0; a < 3; a++) if (!g_keys[a]) {
        std::ifstream f(std::string(dir) + "/" + kFiles[a], std::ios::binary); if (!f) continue;
        std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        try { g_keys[a] = build_key(a, buf.data(), buf.size(), verify_device(), kChunk); } catch (const std::exception& e) { printf("%s\n", e.what()); }
    }
}
std::shared_ptr<GpuKey> key_for(int algo) { std::lock_guard<std::mutex> l(g_mu); load_dir_once(); return g_keys[algo]; }

// items [off, off + m): the host pre-check and the public-input windows, uploaded, then k_verify_prep into k.pd (k.mu held).
// Returns how many items passed the host pre-check.
size_t prep_chunk(GpuKey& k, const uint8_t* proofs, const uint32_t* lens, const uint8_t* signals, size_t off, size_t m,
                  std::vector<uint8_t>& win, std::vector<uint8_t>& pre) {
    size_t passed = 0;
    for (size_t i = 0; i < m; i++) {
        const size_t j = off + i;
        pre[i] = lens[j] <= (uint32_t)kProofSlot && V::proof_shape_ok(proofs + kProofSlot * j, lens[j], k.has_commitment);
        passed += pre[i];
        V::public_windows(k.algo, signals + V::kSignalBytes * j, win.data() + V::kWindows * i);
    }
    hipStream_t s = k.stream;
    ck(hipMemcpyAsync(k.proofs.p, proofs + kProofSlot * off, m * kProofSlot, hipMemcpyHostToDevice, s), "copy");
    ck(hipMemcpyAsync(k.win.p, win.data(), m * V::kWindows, hipMemcpyHostToDevice, s), "copy");
    ck(hipMemcpyAsync(k.pre.p, pre.data(), m, hipMemcpyHostToDevice, s), "copy");
    launch_verify_prep(k.kd, k.proofs.p, k.win.p, k.pre.p, k.pd.p, m, s);
    ck(hipGetLastError(), "k_verify_prep");
    return passed;
}

// the path of a call of n items, recorded for gsc_verify_last_path (k.mu held)
bool route_few(GpuKey& k, size_t n) {
    const int mode = g_path_mode.load();
    const bool few = mode ? mode == kPathFew : n <= k.few_max;
    k.last_path = few ? kPathFew : kPathThread;
    if (few && !k.few_lines.p) {
        Tallying tallying(&k.bytes, k.device);
        k.few_lines.alloc(k.few_cap() * kLineSteps);
    }
    return few;
}
// verdicts of the m proofs in k.pd into k.verdict, one pairing check per proof on the call's path, on stream s
void launch_pairings(GpuKey& k, bool few, size_t m, hipStream_t s) {
    if (few) {
        launch_verify_few_lines(k.pd.p, m, k.few_lines.p, s);
        launch_verify_few_pairing(k.kd, k.pd.p, k.few_lines.p, k.verdict.p, nullptr, m, s);
    } else launch_verify_pairing(k.kd, k.pd.p, k.verdict.p, nullptr, m, s);
    ck(hipGetLastError(), "k_verify_pairing");
}

// verdicts for n items; proofs in 196-byte slots.  Returns the number accepted; throws HipError on a device error.
long long run_verify(GpuKey& k, const uint8_t* proofs, const uint32_t* lens, const uint8_t* signals, size_t n, uint8_t* verdicts) {
    std::lock_guard<std::mutex> l(k.mu);
    ck(hipSetDevice(k.device), "hipSetDevice");
    long long accepted = 0;
    const bool few = route_few(k, n);
    const size_t chunk = std::min(n, few ? kFewChunk : kChunk);
    std::vector<uint8_t> win(chunk * V::kWindows), pre(chunk);
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        if (!k.fits) { memset(verdicts + off, 0, m); continue; }
        prep_chunk(k, proofs, lens, signals, off, m, win, pre);
        hipStream_t s = k.stream;
        launch_pairings(k, few, m, k.stream);
        ck(hipMemcpyAsync(verdicts + off, k.verdict.p, m, hipMemcpyDeviceToHost, s), "copy");
        ck(hipStreamSynchronize(s), "verify");
        for (size_t i = 0; i < m; i++) accepted += verdicts[off + i];
    }
    return accepted;
}

// ---- batched check ----
// Randomizers: OS CSPRNG bytes, drawn afresh for every chunk of every call.  gsc_debug_verify_randomizers (a test hook) can make
// them a fixed function of a seed, or all 1 (the naive sum the randomizers exist to defeat).
enum class RandMode { Csprng, Seeded, Ones };
std::mutex g_rand_mu;
RandMode g_rand_mode = RandMode::Csprng;
uint8_t g_rand_seed[32];

void os_random(uint8_t* out, size_t n) {
    for (size_t got = 0; got < n;) {
        const ssize_t r = getrandom(out + got, n - got, 0);
        if (r > 0) got += (size_t)r;
        else if (r < 0 && errno != EINTR) throw std::runtime_error(std::string("getrandom failed: ") + strerror(errno));
    }
}
// m x kRandWords words: rho_i, then t_i when `with_t` (else 0); uniform, nonzero 128-bit values
void draw_randomizers(uint32_t* out, size_t m, bool with_t, uint64_t chunk) {
    RandMode mode; uint8_t seed[32];
    { std::lock_guard<std::mutex> l(g_rand_mu); mode = g_rand_mode; memcpy(seed, g_rand_seed, 32); }
    const int nw = with_t ? 8 : 4;
    std::vector<uint8_t> bytes(16 * (with_t ? 2 : 1) * m, 0);
    if (mode == RandMode::Csprng) os_random(bytes.data(), bytes.size());
    else if (mode == RandMode::Seeded) {
        uint8_t nonce[12] = {0};
        for (int b = 0; b < 8; b++) nonce[b] = (uint8_t)(chunk >> (8 * b));
        chacha20_xor_stream(seed, nonce, 0, bytes.data(), bytes.data(), bytes.size());
    }
    for (size_t i = 0; i < m; i++) {
        uint32_t* r = out + (size_t)kRandWords * i;
        for (int w = 0; w < kRandWords; w++) r[w] = 0;
        for (int h = 0; h < nw / 4; h++) {
            uint32_t* v = r + 4 * h;
            if (mode == RandMode::Ones) { v[0] = 1; continue; }
            uint8_t* b = bytes.data() + 16 * ((nw / 4) * i + h);
            for (;;) {
                uint32_t any = 0;
                for (int w = 0; w < 4; w++) { memcpy(&v[w], b + 4 * w, 4); any |= v[w]; }
                if (any) break;
                if (mode == RandMode::Seeded) { v[0] = 1; break; }
                os_random(b, 16);
            }
        }
    }
}

// the batched check over n items.  all == false: verdicts as run_verify's, returns the number accepted.  all == true (verdicts
// unused): returns 1 iff every item is accepted, else 0, stopping at the first failing chunk.  Throws HipError on a device error.
long long run_verify_batched(GpuKey& k, const uint8_t* proofs, const uint32_t* lens, const uint8_t* signals, size_t n, uint8_t* verdicts, bool all) {
    std::lock_guard<std::mutex> l(k.mu);
    ck(hipSetDevice(k.device), "hipSetDevice");
    long long accepted = 0;
    const bool few = route_few(k, n);
    const size_t chunk = std::max<size_t>(1, std::min(n, few ? kFewChunk : kChunk));
    std::vector<uint8_t> win(chunk * V::kWindows), pre(chunk), okh(all ? chunk : 0);
    std::vector<uint32_t> rnd(chunk * kRandWords);
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        if (!k.fits) { if (all) return 0; memset(verdicts + off, 0, m); continue; }
        const size_t passed = prep_chunk(k, proofs, lens, signals, off, m, win, pre);
        if (all && passed < m) { ck(hipStreamSynchronize(k.stream), "verify"); return 0; }
        draw_randomizers(rnd.data(), m, k.has_commitment, off / chunk);      // on the host while k_verify_prep runs
        hipStream_t s = k.stream;
        ck(hipMemcpyAsync(k.rnd.p, rnd.data(), m * kRandWords * sizeof(uint32_t), hipMemcpyHostToDevice, s), "copy");
        launch_verify_batch(k.kd, k.pd.p, k.rnd.p, m, k.bufs(), few ? k.few_lines.p : nullptr, s);
        ck(hipGetLastError(), "k_verify_batch");
        uint8_t* okv = all ? okh.data() : verdicts + off;
        uint8_t flag = 0;
        ck(hipMemcpyAsync(okv, k.bok.p, m, hipMemcpyDeviceToHost, s), "copy");
        ck(hipMemcpyAsync(&flag, k.bflag.p, 1, hipMemcpyDeviceToHost, s), "copy");
        ck(hipStreamSynchronize(s), "verify batch");
        size_t nok = 0;
        for (size_t i = 0; i < m; i++) nok += okv[i];
        if (all) { if (!flag || nok < m) return 0; continue; }
        if (!flag) {      // some proof with ok fails: the per-proof pairings of the same ProofDev decide, as in run_verify
            launch_pairings(k, few, m, k.stream);
            ck(hipMemcpyAsync(verdicts + off, k.verdict.p, m, hipMemcpyDeviceToHost, s), "copy");
            ck(hipStreamSynchronize(s), "verify");
            nok = 0;
            for (size_t i = 0; i < m; i++) nok += verdicts[off + i];
        }
        accepted += (long long)nok;
    }
    return all ? 1 : accepted;
}

// ---- claim-wise batched check ----
// Claim j is the items [ends[j-1], ends[j]) (the caller has checked ends).  A chunk's items are cut into parts at the claim and chunk
// boundaries; every part is one equation on the device with its own randomizers' sums, and a claim is accepted iff every one of its
// parts holds and every one of its items decodes.  Returns the number of claims accepted; throws HipError on a device error.
long long run_verify_claims(GpuKey& k, const uint8_t* proofs, const uint32_t* lens, const uint8_t* signals, size_t n, const uint64_t* ends, size_t m,
                            uint8_t* verdicts) {
    std::lock_guard<std::mutex> l(k.mu);
    ck(hipSetDevice(k.device), "hipSetDevice");
    for (size_t j = 0; j < m; j++) verdicts[j] = (k.fits || ends[j] == (j ? ends[j - 1] : 0)) ? 1 : 0;      // empty claims hold
    if (n && k.fits) {
        const bool few = route_few(k, n);
        const size_t chunk = std::min(n, few ? kFewChunk : kChunk);
        const ClaimBufs cb = k.claim_bufs();
        std::vector<uint8_t> win(chunk * V::kWindows), pre(chunk), okh(chunk), flag(chunk);
        std::vector<uint32_t> rnd(chunk * kRandWords);
        std::vector<claims::Part> parts;
        std::vector<size_t> owner;      // the claim of each part
        size_t first = 0;               // the first claim that may own items from `off` on
        for (size_t off = 0; off < n; off += chunk) {
            const size_t cm = std::min(chunk, n - off);
            parts.clear(); owner.clear();
            while (ends[first] <= off) first++;
            for (size_t j = first; j < m; j++) {
                const size_t lo = std::max<size_t>(j ? ends[j - 1] : 0, off), hi = std::min<size_t>(ends[j], off + cm);
                if (lo >= off + cm) break;
                if (lo < hi) { parts.push_back(claims::Part{(uint32_t)(lo - off), (uint32_t)(hi - off)}); owner.push_back(j); }
            }
            prep_chunk(k, proofs, lens, signals, off, cm, win, pre);
            draw_randomizers(rnd.data(), cm, k.has_commitment, off / chunk);      // on the host while k_verify_prep runs
            hipStream_t s = k.stream;
            ck(hipMemcpyAsync(k.rnd.p, rnd.data(), cm * kRandWords * sizeof(uint32_t), hipMemcpyHostToDevice, s), "copy");
            ck(hipMemcpyAsync(cb.parts, parts.data(), parts.size() * sizeof(claims::Part), hipMemcpyHostToDevice, s), "copy");
            launch_verify_claims(k.kd, k.pd.p, k.rnd.p, cm, parts.size(), k.bufs(), cb, few ? k.few_lines.p : nullptr, s);
            ck(hipGetLastError(), "k_verify_claims");
            ck(hipMemcpyAsync(okh.data(), k.bok.p, cm, hipMemcpyDeviceToHost, s), "copy");
            ck(hipMemcpyAsync(flag.data(), cb.flag, parts.size(), hipMemcpyDeviceToHost, s), "copy");
            ck(hipStreamSynchronize(s), "verify claims");
            for (size_t p = 0; p < parts.size(); p++) {
                bool good = flag[p] == 1;
                for (uint32_t i = parts[p].begin; good && i < parts[p].end; i++) good = okh[i] == 1;
                if (!good) verdicts[owner[p]] = 0;
            }
        }
    }
    long long accepted = 0;
    for (size_t j = 0; j < m; j++) accepted += verdicts[j];
    return accepted;
}

// VerifyBatch / VerifyAll: the well-formed items of a JSON array grouped by algorithm, as gsc_verify_raw's arguments
struct Grouped {
    std::vector<size_t> where[3];
    std::vector<uint8_t> slots[3], sigs[3];
    std::vector<uint32_t> lens[3];
    size_t bad = 0;           // items that do not parse as a Verify request
};
Grouped group_requests(const JsonValue& root) {
    Grouped g;
    for (size_t i = 0; i < root.items.size(); i++) {
        int algo; std::vector<uint8_t> proof, sig;
        if (!V::parse_request(root.items[i], algo, proof, sig) || algo < 0 || sig.size() != V::kSignalBytes) { g.bad++; continue; }
        g.where[algo].push_back(i);
        std::vector<uint8_t> slot(kProofSlot, 0);
        memcpy(slot.data(), proof.data(), std::min(proof.size(), (size_t)kProofSlot));
        g.slots[algo].insert(g.slots[algo].end(), slot.begin(), slot.end());
        g.sigs[algo].insert(g.sigs[algo].end(), sig.begin(), sig.end());
        g.lens[algo].push_back(proof.size() > kProofSlot ? UINT32_MAX : (uint32_t)proof.size());
    }
    return g;
}

struct Prove_return to_c(const std::string& s) {
    char* p = (char*)malloc(s.size() + 1);
    memcpy(p, s.data(), s.size()); p[s.size()] = 0;
    return Prove_return{p, (GoInt)s.size()};
}

}  // namespace

extern "C" {

int gsc_verify_init(GoUint8 algorithmID, GoSlice verifyingKey) {
    if (algorithmID > 2 || !verifyingKey.data || verifyingKey.len <= 0) return 0;
    try {
        auto k = build_key(algorithmID, (const uint8_t*)verifyingKey.data, (size_t)verifyingKey.len, verify_device(), kChunk);
        if (!k) return 0;
        std::lock_guard<std::mutex> l(g_mu);
        g_keys[algorithmID] = std::move(k);
        return 1;
    } catch (const std::exception& e) { printf("gsc_verify_init: %s\n", e.what()); return 0; }
}

long long gsc_verify_raw(GoUint8 algorithmID, const uint8_t* proofs, const uint32_t* proof_lens, const uint8_t* signals, size_t n, uint8_t* verdicts) {
    if (n) memset(verdicts, 0, n);
    if (algorithmID > 2) return -1;
    auto k = key_for(algorithmID);
    if (!k) return -1;
    if (!n) return 0;
    try { return run_verify(*k, proofs, proof_lens, signals, n, verdicts); }
    catch (const std::exception& e) { printf("gsc_verify_raw: %s\n", e.what()); memset(verdicts, 0, n); return -2; }
}

struct Prove_return VerifyBatch(GoSlice params) {
    std::string out;
    try {
        JsonValue root;
        try { root = json_parse((const char*)params.data, params.len > 0 ? (size_t)params.len : 0); }
        catch (const JsonSyntaxError& e) { return to_c("{\"Offset\":" + std::to_string(e.offset) + "}"); }
        if (root.kind != JsonValue::Array) return to_c(json_quote("VerifyBatch expects a JSON array"));
        const size_t n = root.items.size();
        std::vector<uint8_t> verdict(n, 0);
        // the well-formed items grouped by algorithm: one gsc_verify_raw pass each, verdicts put back in place
        Grouped g = group_requests(root);
        for (int a = 0; a < 3; a++) {
            const size_t m = g.where[a].size();
            if (!m) continue;
            std::vector<uint8_t> v(m);
            if (gsc_verify_raw((GoUint8)a, g.slots[a].data(), g.lens[a].data(), g.sigs[a].data(), m, v.data()) < 0) continue;   // no key: false
            for (size_t i = 0; i < m; i++) verdict[g.where[a][i]] = v[i];
        }
        out = "[";
        for (size_t i = 0; i < n; i++) { if (i) out += ","; out += verdict[i] ? "true" : "false"; }
        out += "]";
    } catch (const std::exception& e) { out = json_quote(e.what()); }
    return to_c(out);
}

GoUint8 gsc_verify_json(GoSlice params) {
    try {
        JsonValue arr;
        arr.kind = JsonValue::Array;
        arr.items.push_back(json_parse((const char*)params.data, params.len > 0 ? (size_t)params.len : 0));
        Grouped g = group_requests(arr);      // VerifyBatch's parser on an array of this one item
        for (int a = 0; a < 3; a++) if (g.where[a].size()) {
            uint8_t v = 0;
            return gsc_verify_raw((GoUint8)a, g.slots[a].data(), g.lens[a].data(), g.sigs[a].data(), 1, &v) == 1 && v;
        }
        return 0;
    } catch (const std::exception&) { return 0; }
}

int gsc_verify_last_path(GoUint8 algorithmID) {
    if (algorithmID > 2) return -1;
    auto k = key_for(algorithmID);
    return k ? k->last_path.load() : -1;
}

long long gsc_verify_raw_batched(GoUint8 algorithmID, const uint8_t* proofs, const uint32_t* proof_lens, const uint8_t* signals, size_t n,
                                 uint8_t* verdicts) {
    if (n) memset(verdicts, 0, n);
    if (algorithmID > 2) return -1;
    auto k = key_for(algorithmID);
    if (!k) return -1;
    if (!n) return 0;
    try { return run_verify_batched(*k, proofs, proof_lens, signals, n, verdicts, false); }
    catch (const std::exception& e) { printf("gsc_verify_raw_batched: %s\n", e.what()); memset(verdicts, 0, n); return -2; }
}

int gsc_verify_all(GoUint8 algorithmID, const uint8_t* proofs, const uint32_t* proof_lens, const uint8_t* signals, size_t n) {
    if (algorithmID > 2) return -1;
    auto k = key_for(algorithmID);
    if (!k) return -1;
    try { return (int)run_verify_batched(*k, proofs, proof_lens, signals, n, nullptr, true); }
    catch (const std::exception& e) { printf("gsc_verify_all: %s\n", e.what()); return -2; }
}

long long gsc_verify_claims(GoUint8 algorithmID, const uint8_t* proofs, const uint32_t* proof_lens, const uint8_t* signals, size_t n,
                            const uint64_t* claim_ends, size_t m, uint8_t* verdicts) {
    if (algorithmID > 2) return -1;
    auto k = key_for(algorithmID);
    if (!k) return -1;
    for (size_t j = 0; j < m; j++) if (claim_ends[j] < (j ? claim_ends[j - 1] : 0)) return -3;
    if ((m ? claim_ends[m - 1] : 0) != n) return -3;
    if (!m) return 0;
    try { return run_verify_claims(*k, proofs, proof_lens, signals, n, claim_ends, m, verdicts); }
    catch (const std::exception& e) { printf("gsc_verify_claims: %s\n", e.what()); memset(verdicts, 0, m); return -2; }
}

struct Prove_return VerifyClaims(GoSlice params) {
    std::string out;
    try {
        JsonValue root;
        try { root = json_parse((const char*)params.data, params.len > 0 ? (size_t)params.len : 0); }
        catch (const JsonSyntaxError& e) { return to_c("{\"Offset\":" + std::to_string(e.offset) + "}"); }
        if (root.kind != JsonValue::Array) return to_c(json_quote("VerifyClaims expects a JSON array"));
        const size_t nc = root.items.size();
        std::vector<uint8_t> verdict(nc, 0);
        // every well-formed claim split by cipher: per cipher the items of all claims in one gsc_verify_claims call, a claim's share
        // of them as one claim of that call
        std::vector<uint8_t> slots[3], sigs[3];
        std::vector<uint32_t> lens[3];
        std::vector<uint64_t> ends[3];
        std::vector<size_t> claim_of[3];
        for (size_t c = 0; c < nc; c++) {
            const JsonValue& claim = root.items[c];
            if (claim.kind != JsonValue::Array || claim.items.empty()) continue;
            Grouped g = group_requests(claim);
            if (g.bad) continue;
            verdict[c] = 1;
            for (int a = 0; a < 3; a++) if (!g.where[a].empty()) {
                slots[a].insert(slots[a].end(), g.slots[a].begin(), g.slots[a].end());
                sigs[a].insert(sigs[a].end(), g.sigs[a].begin(), g.sigs[a].end());
                lens[a].insert(lens[a].end(), g.lens[a].begin(), g.lens[a].end());
                ends[a].push_back(lens[a].size());
                claim_of[a].push_back(c);
            }
        }
        for (int a = 0; a < 3; a++) {
            const size_t mc = ends[a].size();
            if (!mc) continue;
            std::vector<uint8_t> v(mc, 0);
            const bool ran = gsc_verify_claims((GoUint8)a, slots[a].data(), lens[a].data(), sigs[a].data(), lens[a].size(), ends[a].data(), mc, v.data()) >= 0;   // no key: false
            for (size_t i = 0; i < mc; i++) if (!ran || !v[i]) verdict[claim_of[a][i]] = 0;
        }
        out = "[";
        for (size_t c = 0; c < nc; c++) { if (c) out += ","; out += verdict[c] ? "true" : "false"; }
        out += "]";
    } catch (const std::exception& e) { out = json_quote(e.what()); }
    return to_c(out);
}

GoUint8 VerifyAll(GoSlice params) {
    try {
        const JsonValue root = json_parse((const char*)params.data, params.len > 0 ? (size_t)params.len : 0);
        if (root.kind != JsonValue::Array || root.items.empty()) return 0;
        Grouped g = group_requests(root);
        if (g.bad) return 0;
        for (int a = 0; a < 3; a++) {
            const size_t m = g.where[a].size();
            if (m && gsc_verify_all((GoUint8)a, g.slots[a].data(), g.lens[a].data(), g.sigs[a].data(), m) != 1) return 0;
        }
        return 1;
    } catch (const std::exception&) { return 0; }
}

}  // extern "C"

// gsc_debug_verify_randomizers' body (capi.cpp gates the hook): NULL seed and !all_ones: the OS CSPRNG again
int gsc_verify_debug_randomizers_impl(const uint8_t* seed32, int all_ones) {
    std::lock_guard<std::mutex> l(g_rand_mu);
    if (all_ones) g_rand_mode = RandMode::Ones;
    else if (seed32) { g_rand_mode = RandMode::Seeded; memcpy(g_rand_seed, seed32, 32); }
    else g_rand_mode = RandMode::Csprng;
    return 0;
}

// n randomizers of four words each for the key ceremony's random combinations (sigma_gpu.cpp), drawn as the verifier draws its own
void gsc_verify_draw_rho_impl(uint32_t* out, size_t n) {
    std::vector<uint32_t> rnd((size_t)kRandWords * n);
    draw_randomizers(rnd.data(), n, false, 0);
    for (size_t i = 0; i < n; i++) memcpy(out + 4 * i, rnd.data() + (size_t)kRandWords * i, 16);
}

// the verifier's device, for the key ceremony (phase2_gpu.cpp): GSC_DEVICE, or the first of GSC_DEVICES
int gsc_verify_device_impl() { return verify_device(); }

// gsc_debug_verify_path's body
int gsc_verify_debug_path_impl(int mode) {
    if (mode < 0 || mode > 2) return -1;
    g_path_mode = mode;
    return 0;
}

// gsc_debug_pairing's and gsc_debug_pairing_few's body: capi.cpp exports the hooks behind its GSC_ENABLE_TEST_HOOKS gate and calls this
long long gsc_verify_debug_pairing_impl(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out, bool few) {
    if (!n) return 0;
    try {
        ck(hipSetDevice(verify_device()), "hipSetDevice");
        hipStream_t s; ck(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
        std::unique_ptr<void, void (*)(void*)> guard((void*)s, [](void* p) { (void)hipStreamSynchronize((hipStream_t)p); (void)hipStreamDestroy((hipStream_t)p); });
        DevBuf<uint8_t> d1, d2, dout, verdict; DevBuf<ProofDev> pd; DevBuf<F12> f;
        d1.alloc(64 * n); d2.alloc(128 * n); dout.alloc(384 * n); verdict.alloc(n); pd.alloc(n); f.alloc(n);
        ck(hipMemcpyAsync(d1.p, g1, 64 * n, hipMemcpyHostToDevice, s), "copy");
        ck(hipMemcpyAsync(d2.p, g2, 128 * n, hipMemcpyHostToDevice, s), "copy");
        KeyDev kd{};
        kd.fits = 1; kd.has_commitment = 0;
        for (int i = 0; i < 5; i++) kd.qinf[i] = 1;
        kd.alpha.inf = 1;
        launch_verify_debug_points(d1.p, d2.p, pd.p, n, s);
        DevBuf<Line> lines;
        if (few) {
            lines.alloc(n * kLineSteps);
            launch_verify_few_lines(pd.p, n, lines.p, s);
            launch_verify_few_pairing(kd, pd.p, lines.p, verdict.p, f.p, n, s);
        } else launch_verify_pairing(kd, pd.p, verdict.p, f.p, n, s);
        launch_verify_f12_bytes(f.p, dout.p, n, s);
        ck(hipMemcpyAsync(out, dout.p, 384 * n, hipMemcpyDeviceToHost, s), "copy");
        ck(hipStreamSynchronize(s), "debug pairing");
        return (long long)n;
    } catch (const std::exception& e) { printf("gsc_debug_pairing: %s\n", e.what()); return -1; }
}

// gsc_debug_verify_g1's body (include/libprove.h): a key of its own from build_key, prep_chunk, then the production launchers on the caller's
// randomizers; every output is collected on the host first, so a call that fails has written nothing
int gsc_verify_debug_g1_impl(const gsc_debug_verify_g1_args& a) {
    constexpr size_t kG1 = 65, kG2 = 129;
    auto refuse = [](const char* why) { printf("gsc_debug_verify_g1: %s\n", why); return -1; };
    if (a.algorithm > 2 || !a.vk || !a.vk_len) return refuse("algorithm is 0 .. 2 with a key");
    if (a.n < 1 || a.n > kFewChunk || !a.proofs || !a.lens || !a.signals || !a.rnd) return refuse("n is 1 .. 8192 with proofs, lens, signals and rnd");
    if (a.path != kPathThread && a.path != kPathFew) return refuse("path is 1 or 2");
    if (a.fill > 255) return refuse("fill is a byte");
    if (a.np && !a.ends) return refuse("parts without ends");
    for (size_t j = 0; j < a.np; j++) if (a.ends[j] <= (j ? a.ends[j - 1] : 0) || a.ends[j] > a.n) return refuse("part ends are strictly increasing up to n");
    if (a.np && a.ends[a.np - 1] != a.n) return refuse("the last part ends at n");
    try {
        const size_t n = a.n, np = a.np;
        std::vector<int8_t> status;
        auto key = build_key((int)a.algorithm, a.vk, a.vk_len, verify_device(), n, &status);
        if (!key) return -2;
        GpuKey& k = *key;
        if (!k.fits) { printf("gsc_debug_verify_g1: the key is not one of the algorithm's circuit\n"); return -3; }
        std::lock_guard<std::mutex> l(k.mu);
        ck(hipSetDevice(k.device), "hipSetDevice");
        hipStream_t s = k.stream;
        const bool few = a.path == kPathFew, com = k.has_commitment;
        if (few && !k.few_lines.p) { Tallying tallying(&k.bytes, k.device); k.few_lines.alloc(k.few_cap() * kLineSteps); }
        // one device image per output, filled first; the host copies below are what the caller gets
        struct Out { DevBuf<uint8_t> d; std::vector<uint8_t> h; };
        auto make = [&](Out& o, size_t bytes) { o.d.alloc(bytes); o.h.resize(bytes); ck(hipMemsetAsync(o.d.p, (int)a.fill, bytes, s), "fill"); };
        auto fetch = [&](Out& o) { if (!o.h.empty()) ck(hipMemcpyAsync(o.h.data(), o.d.p, o.h.size(), hipMemcpyDeviceToHost, s), "copy"); };
        Out table, ctable, g1, g2, fixed, pfixed;
        make(table, V::kWindows * 256 * kG1); make(ctable, kCommitWindows * 256 * kG1); make(g1, n * 6 * kG1); make(g2, n * kG2);
        make(fixed, kBatchFixed * kG1); make(pfixed, std::max<size_t>(np, 1) * kBatchFixed * kG1);
        launch_verify_point_bytes(k.table.p, sizeof(VP1), false, nullptr, 0, table.d.p, kG1, V::kWindows * 256, s);
        if (com) launch_verify_point_bytes(k.ctable.p, sizeof(VP1), false, nullptr, 0, ctable.d.p, kG1, kCommitWindows * 256, s);

        std::vector<uint8_t> win(n * V::kWindows), pre(n);
        prep_chunk(k, a.proofs, a.lens, a.signals, 0, n, win, pre);
        ck(hipMemcpyAsync(k.rnd.p, a.rnd, n * kRandWords * sizeof(uint32_t), hipMemcpyHostToDevice, s), "copy");
        launch_verify_batch(k.kd, k.pd.p, k.rnd.p, n, k.bufs(), few ? k.few_lines.p : nullptr, s);
        ck(hipGetLastError(), "k_verify_batch");
        std::vector<ProofDev> pd(n);
        std::vector<uint8_t> okv(n), ok(n), pflag(np, (uint8_t)a.fill);
        std::vector<uint32_t> prho(5 * np);
        uint8_t flag = 0;
        ck(hipMemcpyAsync(pd.data(), k.pd.p, n * sizeof(ProofDev), hipMemcpyDeviceToHost, s), "copy");
        ck(hipMemcpyAsync(okv.data(), k.bok.p, n, hipMemcpyDeviceToHost, s), "copy");
        ck(hipMemcpyAsync(&flag, k.bflag.p, 1, hipMemcpyDeviceToHost, s), "copy");
        const uint8_t* pdb = (const uint8_t*)k.pd.p;
        const size_t live = offsetof(ProofDev, ok);
        const size_t at[5] = {offsetof(ProofDev, A), offsetof(ProofDev, C), offsetof(ProofDev, L), offsetof(ProofDev, D), offsetof(ProofDev, pok)};
        for (int j = 0; j < 5; j++) if (j != 3 || com) launch_verify_point_bytes(pdb + at[j], sizeof(ProofDev), false, pdb + live, sizeof(ProofDev), g1.d.p + kG1 * j, 6 * kG1, n, s);
        launch_verify_point_bytes(k.ra.p, sizeof(VP1), false, nullptr, 0, g1.d.p + kG1 * 5, 6 * kG1, n, s);
        launch_verify_point_bytes(pdb + offsetof(ProofDev, B), sizeof(ProofDev), true, pdb + live, sizeof(ProofDev), g2.d.p, kG2, n, s);
        launch_verify_point_bytes(k.fixed.p, sizeof(VP1), false, nullptr, 0, fixed.d.p, kG1, kBatchFixed, s);
        if (np) {
            const ClaimBufs cb = k.claim_bufs();
            std::vector<claims::Part> parts(np);
            for (size_t j = 0; j < np; j++) parts[j] = claims::Part{(uint32_t)(j ? a.ends[j - 1] : 0), (uint32_t)a.ends[j]};
            ck(hipMemcpyAsync(cb.parts, parts.data(), np * sizeof(claims::Part), hipMemcpyHostToDevice, s), "copy");
            launch_verify_claims(k.kd, k.pd.p, k.rnd.p, n, np, k.bufs(), cb, few ? k.few_lines.p : nullptr, s);
            ck(hipGetLastError(), "k_verify_claims");
            for (int j = 0; j < (com ? kBatchFixed : 3); j++) launch_verify_point_bytes(cb.fixed + j, kBatchFixed * sizeof(VP1), false, nullptr, 0, pfixed.d.p + kG1 * j, kBatchFixed * kG1, np, s);
            ck(hipMemcpyAsync(prho.data(), cb.rho, 5 * np * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "copy");
            ck(hipMemcpyAsync(pflag.data(), cb.flag, np, hipMemcpyDeviceToHost, s), "copy");
            ck(hipStreamSynchronize(s), "verify claims");      // parts is read by the copy above
        }
        ck(hipGetLastError(), "k_verify_point_bytes");
        fetch(table); fetch(ctable); fetch(g1); fetch(g2); fetch(fixed); fetch(pfixed);
        ck(hipStreamSynchronize(s), "debug verify g1");
        for (size_t i = 0; i < n; i++) ok[i] = pd[i].ok ? 1 : 0;
        auto give = [](void* dst, const void* src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
        give(a.key_status, status.data(), std::min(a.key_status_cap, status.size()));
        give(a.table, table.h.data(), table.h.size()); give(a.ctable, ctable.h.data(), ctable.h.size());
        give(a.ok, ok.data(), n); give(a.g1, g1.h.data(), g1.h.size()); give(a.g2, g2.h.data(), g2.h.size()); give(a.okv, okv.data(), n);
        give(a.fixed, fixed.h.data(), fixed.h.size()); give(a.flag, &flag, 1);
        give(a.pfixed, pfixed.h.data(), np * kBatchFixed * kG1); give(a.prho, prho.data(), 5 * np * sizeof(uint32_t)); give(a.pflag, pflag.data(), np);
        return 0;
    } catch (const std::exception& e) { printf("gsc_debug_verify_g1: %s\n", e.what()); return -1; }
}

// ---- the prover's self-check (prove_check.hpp): a key as above on an engine replica's device, fed from a lane's output buffers ----
namespace gsc {

struct ProveCheckCtx {
    std::shared_ptr<GpuKey> key;
    std::atomic<uint64_t> chunks{0}, proofs{0}, refused{0}, fallbacks{0};
};

std::shared_ptr<ProveCheckCtx> prove_check_create(int algo, const uint8_t* vk, size_t len, int device, size_t cap) {
    auto c = std::make_shared<ProveCheckCtx>();
    c->key = build_key(algo, vk, len, device, cap);
    if (!c->key) return nullptr;
    return c;
}
size_t prove_check_device_bytes(const ProveCheckCtx& c) { return c.key->bytes; }
size_t verifier_device_bytes(int device) { return device_bytes(device).load(); }
void prove_check_add_stats(const ProveCheckCtx& c, uint64_t out[4]) {
    out[0] += c.chunks.load(); out[1] += c.proofs.load(); out[2] += c.refused.load(); out[3] += c.fallbacks.load();
}

// Everything goes on the LANE's stream s (the key's own stream is idle in a check context); the caller has made the key's device current.
ProveCheckPass::ProveCheckPass(std::shared_ptr<ProveCheckCtx> ctx, const ProveCheckInput& in, hipStream_t s)
    : ctx_(std::move(ctx)), lock_(ctx_->key->mu), s_(s), n_(in.n), win_(in.n * V::kWindows), verdict_(in.n, 0), rnd_(in.n * kRandWords) {
    GpuKey& k = *ctx_->key;
    if (!n_) return;
    if (n_ > k.cap) throw std::runtime_error("internal: a chunk larger than the self-check's buffers");
    if (!k.fits) return;      // the key is not one of this circuit: Verify accepts nothing under it, every verdict stays 0
    for (size_t i = 0; i < n_; i++) V::public_windows(k.algo, in.signals + V::kSignalBytes * i, win_.data() + V::kWindows * i);
    // the route of a verifier call of n items; the lines buffer bounds the few-proof pass
    few_ = route_few(k, n_) && n_ <= k.few_cap();
    draw_randomizers(rnd_.data(), n_, k.has_commitment, ctx_->chunks.load());
    ck(hipMemcpyAsync(k.win.p, win_.data(), n_ * V::kWindows, hipMemcpyHostToDevice, s), "copy");
    ck(hipMemcpyAsync(k.rnd.p, rnd_.data(), n_ * kRandWords * sizeof(uint32_t), hipMemcpyHostToDevice, s), "copy");
    launch_check_prep(k.kd, ProverOut{in.d_out, in.d_cpts, in.d_status, in.d_flags, in.B, n_}, k.win.p, k.pd.p, s);
    ck(hipGetLastError(), "k_check_prep");
    launch_verify_batch(k.kd, k.pd.p, k.rnd.p, n_, k.bufs(), few_ ? k.few_lines.p : nullptr, s);
    ck(hipGetLastError(), "k_verify_batch");
    ck(hipMemcpyAsync(verdict_.data(), k.bok.p, n_, hipMemcpyDeviceToHost, s), "copy");
    ck(hipMemcpyAsync(&flag_, k.bflag.p, 1, hipMemcpyDeviceToHost, s), "copy");
}
// a pass that is dropped before finish() (an exception on the way) has kernels on the context's buffers: they are through before the next pass may start
ProveCheckPass::~ProveCheckPass() { if (!finished_) (void)hipStreamSynchronize(s_); }

const std::vector<uint8_t>& ProveCheckPass::finish(const uint32_t* status, const uint8_t* flags) {
    GpuKey& k = *ctx_->key;
    finished_ = true;
    if (!n_ || !k.fits) return verdict_;
    // the batch equation holds over the proofs that took part (ok): nothing more to do when those are all the prover would release
    bool all = flag_ != 0;
    for (size_t i = 0; all && i < n_; i++) if (status[i] == 0xFFFFFFFFu && !flags[i] && !verdict_[i]) all = false;
    if (all) return verdict_;
    // otherwise the per-proof pairings over the same ProofDev entries decide, as in run_verify_batched
    fell_back_ = true;
    launch_pairings(k, few_, n_, s_);
    ck(hipMemcpyAsync(verdict_.data(), k.verdict.p, n_, hipMemcpyDeviceToHost, s_), "copy");
    ck(hipStreamSynchronize(s_), "prove check");
    return verdict_;
}
void ProveCheckPass::count(size_t checked, size_t refused) {
    ctx_->chunks++; ctx_->proofs += checked; ctx_->refused += refused; if (fell_back_) ctx_->fallbacks++;
}

}  // namespace gsc
