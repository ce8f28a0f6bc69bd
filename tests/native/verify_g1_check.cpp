// Host build of the verifier's G1 stage (csrc/verify_dev.hpp, verify_batch_dev.hpp, verify_claims_dev.hpp compiled by g++ with the HIP headers):
// what gsc_debug_verify_g1 (include/libprove.h) runs on the device, walked one item at a time with the threads, the lanes of a block and the
// reduction trees of k_verify.hip, k_verify_batch.hip and k_verify_claims.hip in loops, printing the fields the hook returns in the hook's bytes.
// tests/test_verify_g1_model_host.py holds the output against tests/verifymodel.py, so that a failure on the GPU lies in the device mapping.
//   stdin : algorithm (0/1/2) | mode (bit 0: no pairings, the flags are printed as 2; bit 1: the window tables are built in full and printed;
//           without it only the entries the proofs read are built, each by the same table_entry) | fill byte |
//           vk length (u32 LE) | vk | n (u32 LE) | n x (proof length u32 LE | 196-byte slot | 144 signal bytes | 8 randomizer words) |
//           np (u32 LE) | np x part end (u32 LE)
//   stdout: "key <rc>" (0, -2 refused, -3 not the algorithm's), then one "<field> <hex>" line per field: key_status, [table, ctable,] ok, g1, g2, okv,
//           fixed, flag, pfixed, prho, pflag.  okv is printed as a copy of ok: the byte k_verify_batch_scale and k_verify_claims_scale store is not
//           modelled on its own here, the GPU tests compare the device's.
#include "verify_claims_dev.hpp"
#include "verify_common.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace gsc::vfy;
namespace V = gsc::verify;
using Bytes = std::vector<uint8_t>;
constexpr size_t kG1 = 65, kG2 = 129;

static uint32_t rd32(FILE* f) { uint8_t b[4]; if (fread(b, 1, 4, f) != 4) return 0; return b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24; }
static void line(const char* name, const uint8_t* p, size_t n) { printf("%s ", name); for (size_t i = 0; i < n; i++) printf("%02x", p[i]); printf("\n"); }

// k_verify_point_bytes
static void coord(const e1& c, bool inf, uint8_t* o) {
    const fe w = F::pack(F::from_mont(c));
    for (int j = 0; j < 8; j++) for (int b = 0; b < 4; b++) o[4 * j + b] = inf ? 0 : (uint8_t)(w.l[7 - j] >> (24 - 8 * b));
}
static void put1(const VP1& p, uint8_t* o) { coord(p.x, p.inf, o); coord(p.y, p.inf, o + 32); o[64] = p.inf ? 1 : 0; }
static void put2(const VP2& p, uint8_t* o) { coord(p.x.a1, p.inf, o); coord(p.x.a0, p.inf, o + 32); coord(p.y.a1, p.inf, o + 64); coord(p.y.a0, p.inf, o + 96); o[128] = p.inf ? 1 : 0; }

// block_sum (csrc/block_sum.hpp) over the values of one block's threads
static G1X tree(std::vector<G1X> v) {
    for (size_t h = v.size() / 2; h > 0; h >>= 1) for (size_t t = 0; t < h; t++) v[t] = g1_add(v[t], v[t + h]);
    return v[0];
}

int main() {
    const int algo = fgetc(stdin), mode = fgetc(stdin), fill = fgetc(stdin);
    const bool pair = !(mode & 1), tables = mode & 2;
    Bytes vk(rd32(stdin));
    if (fread(vk.data(), 1, vk.size(), stdin) != vk.size()) return 2;
    // build_key: the points in slots of 64 / 128 bytes, k_verify_key_points
    V::VkLayout lay;
    if (algo < 0 || algo > 2 || !V::parse_vk_layout(vk.data(), vk.size(), lay, nullptr)) { printf("key -2\n"); return 0; }
    Bytes b1, b2;
    auto add = [&](Bytes& v, size_t at, size_t cb) {
        const size_t len = V::point_is_raw(&vk[at]) ? 2 * cb : cb, o = v.size();
        v.resize(o + 2 * cb, 0); memcpy(v.data() + o, &vk[at], len);
    };
    add(b1, lay.alpha, 32); add(b1, lay.g1_beta, 32); add(b1, lay.g1_delta, 32);
    for (size_t at : lay.K) add(b1, at, 32);
    add(b2, lay.beta, 64); add(b2, lay.gamma, 64); add(b2, lay.delta, 64);
    if (lay.has_commitment) { add(b2, lay.ped_g, 64); add(b2, lay.ped_gsn, 64); }
    const size_t n1 = b1.size() / 64, n2 = b2.size() / 128;
    std::vector<VP1> p1(n1); VP2 q[5];
    std::vector<int8_t> st(n1 + n2);
    for (int i = 0; i < 5; i++) q[i].inf = 1;
    bool good = true;
    for (size_t i = 0; i < n1; i++) good = (st[i] = (int8_t)decode_g1_key(&b1[64 * i], p1[i])) >= 0 && good;
    for (size_t i = 0; i < n2; i++) good = (st[n1 + i] = (int8_t)decode_g2_key(&b2[128 * i], q[i])) >= 0 && good;
    if (!good) { printf("key -2\n"); return 0; }
    KeyDev k{};
    k.fits = V::key_fits(algo, lay.K.size(), lay.has_commitment);
    k.has_commitment = lay.has_commitment;
    if (!k.fits) { printf("key -3\n"); return 0; }
    const VP1* K = &p1[3];
    k.alpha = p1[0]; k.k0 = K[0];
    std::vector<VP1> table(V::kWindows * 256), ctable(kCommitWindows * 256);
    std::vector<uint8_t> have(table.size(), 0), chave(ctable.size(), 0);
    auto entry = [&](size_t j, uint32_t v) {      // k_verify_tables, one entry
        if (have[256 * j + v]) return;
        uint32_t first, shift; V::window_base(algo, j, first, shift);
        table[256 * j + v] = table_entry(algo == 0, K, first, shift, v); have[256 * j + v] = 1;
    };
    auto centry = [&](int j, uint32_t v) {
        if (chave[256 * j + v]) return;
        ctable[256 * j + v] = table_entry(false, K, (uint32_t)(1 + V::num_public(algo)), 8 * j, v); chave[256 * j + v] = 1;
    };
    if (tables) {
        for (size_t j = 0; j < V::kWindows; j++) for (uint32_t v = 0; v < 256; v++) entry(j, v);
        if (lay.has_commitment) for (int j = 0; j < kCommitWindows; j++) for (uint32_t v = 0; v < 256; v++) centry(j, v);
    }
    std::vector<Line> lines(5 * kLineSteps);
    for (int i = 0; i < 5; i++) { k.qinf[i] = q[i].inf; k.lines[i] = &lines[i * kLineSteps]; if (pair && !q[i].inf) lines_of(q[i], &lines[i * kLineSteps]); }
    k.table = table.data(); k.ctable = ctable.data();
    printf("key 0\n");
    line("key_status", (const uint8_t*)st.data(), st.size());
    if (tables) {
        Bytes t(table.size() * kG1), c(ctable.size() * kG1, (uint8_t)fill);
        for (size_t i = 0; i < table.size(); i++) put1(table[i], &t[kG1 * i]);
        if (lay.has_commitment) for (size_t i = 0; i < ctable.size(); i++) put1(ctable[i], &c[kG1 * i]);
        line("table", t.data(), t.size()); line("ctable", c.data(), c.size());
    }

    // prep_chunk and k_verify_prep, then k_verify_batch_scale's own part, one item at a time
    const bool com = lay.has_commitment;
    const int nsums = com ? kBatchSums : 2;
    const uint32_t n = rd32(stdin);
    std::vector<ProofDev> pd(n);
    std::vector<uint32_t> rnd((size_t)kRandWords * n);
    std::vector<VP1> ra(n);
    Bytes ok(n), g1(n * 6 * kG1, (uint8_t)fill), g2(n * kG2, (uint8_t)fill);
    std::vector<G1X> terms((size_t)kBatchSums * n, g1_inf());
    std::vector<F12> f(n);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t slot[kProofSlot], sig[V::kSignalBytes], win[V::kWindows];
        const uint32_t len = rd32(stdin);
        if (fread(slot, 1, sizeof slot, stdin) != sizeof slot || fread(sig, 1, sizeof sig, stdin) != sizeof sig) return 2;
        for (int w = 0; w < kRandWords; w++) rnd[(size_t)kRandWords * i + w] = rd32(stdin);
        pd[i] = ProofDev{};
        V::public_windows(algo, sig, win);
        for (size_t j = 0; j < V::kWindows; j++) entry(j, win[j]);
        VP1 d;
        if (com && decode_g1(slot + 132, d) >= 0) { uint8_t c[32]; commitment_challenge(d, c); for (int j = 0; j < kCommitWindows; j++) centry(j, c[j]); }
        if (len <= (uint32_t)kProofSlot && V::proof_shape_ok(slot, len, com)) prep_one(k, slot, win, pd[i]);
        ok[i] = pd[i].ok ? 1 : 0;
        const uint32_t* r = &rnd[(size_t)kRandWords * i];
        claims::scale_one(pd[i], r, nsums, ra[i], &terms[(size_t)kBatchSums * i]);      // batch_scaled_a and batch_term, as both scale kernels call them
        if (pd[i].ok) {
            uint8_t* o = &g1[6 * kG1 * i];
            put1(pd[i].A, o); put1(pd[i].C, o + kG1); put1(pd[i].L, o + 2 * kG1); if (com) put1(pd[i].D, o + 3 * kG1); put1(pd[i].pok, o + 4 * kG1);
            put2(pd[i].B, &g2[kG2 * i]);
        }
        put1(ra[i], &g1[6 * kG1 * i + 5 * kG1]);
        if (pair) f[i] = batch_miller_proof(pd[i], ra[i]);
    }
    line("ok", ok.data(), n); line("g1", g1.data(), g1.size()); line("g2", g2.data(), g2.size()); line("okv", ok.data(), n);

    // k_verify_batch_scale's block sums and k_verify_batch_sum: lane partials over the blocks, the 64-lane tree, the column sums of rho
    const size_t nblk = (n + 63) / 64;
    std::vector<G1X> part(nblk * kBatchSums, g1_inf());
    std::vector<uint64_t> rpart(nblk * 4, 0);
    for (size_t b = 0; b < nblk; b++) {
        for (int j = 0; j < nsums; j++) {
            std::vector<G1X> v(64, g1_inf());
            for (size_t t = 0; t < 64 && 64 * b + t < n; t++) if (ok[64 * b + t]) v[t] = terms[kBatchSums * (64 * b + t) + j];
            part[kBatchSums * b + j] = tree(v);
        }
        for (size_t t = 0; t < 64 && 64 * b + t < n; t++) if (ok[64 * b + t]) for (int w = 0; w < 4; w++) rpart[4 * b + w] += rnd[kRandWords * (64 * b + t) + w];
    }
    G1X sums[kBatchSums]; uint32_t rho[5];
    for (int j = 0; j < kBatchSums; j++) {
        std::vector<G1X> v(64, g1_inf());
        for (size_t lane = 0; lane < 64; lane++) for (size_t b = lane; b < nblk; b += 64) v[lane] = g1_add(v[lane], part[kBatchSums * b + j]);
        sums[j] = tree(v);
    }
    uint64_t col[4] = {0, 0, 0, 0};
    for (size_t b = 0; b < nblk; b++) for (int c = 0; c < 4; c++) col[c] += rpart[4 * b + c];
    rho_sum_words(col, rho);
    VP1 fixed[kBatchFixed]; Bytes fx(kBatchFixed * kG1);
    for (int j = 0; j < kBatchFixed; j++) { fixed[j] = batch_fixed_point(k, j, sums, rho); put1(fixed[j], &fx[kG1 * j]); }
    line("fixed", fx.data(), fx.size());
    uint8_t flag = 2;
    if (pair) {
        F12 prod = one12();
        for (uint32_t i = 0; i < n; i++) prod = mul12(prod, f[i]);
        for (int j = 0; j < kBatchFixed; j++) prod = mul12(prod, batch_miller_fixed(k, j, fixed[j]));
        flag = batch_accept(prod) ? 1 : 0;
    }
    line("flag", &flag, 1);

    // the parts: k_verify_claims_sums and k_verify_claims_fixed
    const uint32_t np = rd32(stdin);
    Bytes pfixed(np * kBatchFixed * kG1, (uint8_t)fill), prho(np * 20), pflag(np, 2);
    const int npairs = claims::fixed_pairs(com);
    uint32_t prev = 0;
    for (uint32_t p = 0; p < np; p++) {
        const claims::Part pt{prev, rd32(stdin)};
        if (pt.end <= pt.begin || pt.end > n) return 2;
        prev = pt.end;
        const int width = claims::tree_width(pt.end - pt.begin);
        G1X ps[kBatchSums] = {g1_inf(), g1_inf(), g1_inf(), g1_inf()};
        for (int j = 0; j < nsums; j++) {
            G1X red[claims::kLanes];
            for (int lane = 0; lane < claims::kLanes; lane++) red[lane] = claims::lane_sum(terms.data(), j, pt, lane);
            for (int h = width / 2; h > 0; h >>= 1) for (int lane = 0; lane < h; lane++) red[lane] = g1_add(red[lane], red[lane + h]);
            ps[j] = red[0];
        }
        uint64_t pc[4] = {0, 0, 0, 0};
        for (int lane = 0; lane < width; lane++) {
            uint64_t c[4]; claims::lane_rho(rnd.data(), ok.data(), pt, lane, c);
            for (int w = 0; w < 4; w++) pc[w] += c[w];
        }
        uint32_t pr[5]; rho_sum_words(pc, pr);
        for (int c = 0; c < 5; c++) for (int b = 0; b < 4; b++) prho[20 * p + 4 * c + b] = (uint8_t)(pr[c] >> (8 * b));
        VP1 pf[kBatchFixed];
        for (int j = 0; j < kBatchFixed; j++) { pf[j] = batch_fixed_point(k, j, ps, pr); if (j < npairs) put1(pf[j], &pfixed[kG1 * (kBatchFixed * p + j)]); }
        if (pair) {
            F12 prod = one12();
            for (uint32_t i = pt.begin; i < pt.end; i++) prod = mul12(prod, f[i]);
            for (int j = 0; j < npairs; j++) prod = mul12(prod, batch_miller_fixed(k, j, pf[j]));
            pflag[p] = batch_accept(prod) ? 1 : 0;
        }
    }
    if (prev != (np ? n : 0)) return 2;
    line("pfixed", pfixed.data(), pfixed.size()); line("prho", prho.data(), prho.size()); line("pflag", pflag.data(), pflag.size());
    return 0;
}
