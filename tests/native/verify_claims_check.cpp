// Host build of the claim-wise batched check's device code (csrc/verify_claims_dev.hpp, compiled by g++ with the HIP headers): builds a
// key the way k_verify.hip does, prepares every item with prep_one, then runs the steps of k_verify_claims.hip with the threads, the
// lanes of a wave and the 8-lane groups walked in loops, and prints one verdict per claim.  tests/test_verify_claims_host.py drives it.
//   stdin : algorithm (0/1/2) | mode (bit 0: every randomizer 1 instead of OS entropy; bit 1: the fixed pairs by 8-lane groups, as on the
//           few-proof path, instead of one thread per pair) | vk length (u32 LE) | vk | n (u32 LE) |
//           n x (proof length u32 LE | 196-byte slot | 144 signal bytes) | m (u32 LE) | m x claim end (u32 LE)
//   stdout: "ok <items that decode>" then "claims" and m verdicts (0 / 1); "key 0" when the key is refused, "ends 0" for bad claim ends
#include "verify_claims_dev.hpp"
#include "verify_common.hpp"
#include <cstdio>
#include <random>
#include <vector>

using namespace gsc::vfy;
namespace V = gsc::verify;
using HG = few::HostGroup;

static uint32_t rd32(FILE* f) { uint8_t b[4]; if (fread(b, 1, 4, f) != 4) return 0; return b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24; }

int main() {
    const int algo = fgetc(stdin), mode = fgetc(stdin);
    const bool ones = mode & 1, groups = mode & 2;
    std::vector<uint8_t> vk(rd32(stdin));
    if (fread(vk.data(), 1, vk.size(), stdin) != vk.size()) return 2;
    V::VkLayout lay;
    std::vector<VP1> K; VP1 alpha, skip; VP2 q[5];
    bool good = V::parse_vk_layout(vk.data(), vk.size(), lay, nullptr);
    if (good) {
        good = decode_g1(&vk[lay.alpha], alpha) >= 0 && decode_g1(&vk[lay.g1_beta], skip) >= 0 && decode_g2(&vk[lay.beta], q[0]) >= 0 &&
               decode_g2(&vk[lay.gamma], q[1]) >= 0 && decode_g1(&vk[lay.g1_delta], skip) >= 0 && decode_g2(&vk[lay.delta], q[2]) >= 0;
        K.resize(lay.K.size());
        for (size_t i = 0; good && i < K.size(); i++) good = decode_g1(&vk[lay.K[i]], K[i]) >= 0;
        q[3].inf = q[4].inf = 1;
        if (good && lay.has_commitment) good = decode_g2(&vk[lay.ped_g], q[3]) >= 0 && decode_g2(&vk[lay.ped_gsn], q[4]) >= 0;
    }
    if (!good) { printf("key 0\n"); return 0; }
    KeyDev k{};
    k.fits = V::key_fits(algo, K.size(), lay.has_commitment);
    k.has_commitment = lay.has_commitment;
    std::vector<VP1> table(V::kWindows * 256), ctable(kCommitWindows * 256);
    std::vector<Line> lines(5 * kLineSteps);
    if (k.fits) {
        k.k0 = K[0];
        for (size_t j = 0; j < V::kWindows; j++) {
            uint32_t first, shift; V::window_base(algo, j, first, shift);
            for (uint32_t v = 0; v < 256; v++) table[256 * j + v] = table_entry(algo == 0, K.data(), first, shift, v);
        }
        if (lay.has_commitment)
            for (int j = 0; j < kCommitWindows; j++) for (uint32_t v = 0; v < 256; v++) ctable[256 * j + v] = table_entry(false, K.data(), (uint32_t)(1 + V::num_public(algo)), 8 * j, v);
    }
    k.alpha = alpha;
    for (int i = 0; i < 5; i++) { k.qinf[i] = q[i].inf; k.lines[i] = &lines[i * kLineSteps]; if (!q[i].inf) lines_of(q[i], &lines[i * kLineSteps]); }
    k.table = table.data(); k.ctable = ctable.data();

    // k_verify_prep and k_verify_claims_scale, one item at a time
    std::random_device dev;
    const int nsums = k.has_commitment ? kBatchSums : 2;
    const uint32_t n = rd32(stdin);
    std::vector<ProofDev> pd(n);
    std::vector<uint32_t> rnd((size_t)kRandWords * n, 0);
    std::vector<VP1> ra(n);
    std::vector<uint8_t> okv(n);
    std::vector<G1X> terms((size_t)kBatchSums * n, g1_inf());
    std::vector<F12> f(n);
    int nok = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint8_t slot[kProofSlot], sig[V::kSignalBytes], win[V::kWindows];
        const uint32_t len = rd32(stdin);
        if (fread(slot, 1, sizeof slot, stdin) != sizeof slot || fread(sig, 1, sizeof sig, stdin) != sizeof sig) return 2;
        pd[i] = ProofDev{};
        if (V::proof_shape_ok(slot, len, lay.has_commitment)) { V::public_windows(algo, sig, win); prep_one(k, slot, win, pd[i]); }
        uint32_t* r = &rnd[(size_t)kRandWords * i];
        for (int h = 0; h < nsums / 2; h++) {
            uint32_t any = 0;
            while (!any) for (int w = 0; w < 4; w++) any |= r[4 * h + w] = ones ? (w == 0) : (uint32_t)dev();
        }
        okv[i] = pd[i].ok ? 1 : 0;
        nok += okv[i];
        claims::scale_one(pd[i], r, nsums, ra[i], &terms[(size_t)kBatchSums * i]);
        f[i] = batch_miller_proof(pd[i], ra[i]);      // k_verify_batch_miller's proof branch
    }
    // the parts: the claims that hold items (an empty claim is answered 1 without an equation)
    const uint32_t m = rd32(stdin);
    std::vector<claims::Part> parts;
    std::vector<uint32_t> owner;
    std::vector<int> verdict(m, 1);
    uint32_t prev = 0;
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t end = rd32(stdin);
        if (end < prev || end > n) { printf("ends 0\n"); return 0; }
        if (end > prev) { parts.push_back(claims::Part{prev, end}); owner.push_back(j); }
        prev = end;
    }
    if (prev != n) { printf("ends 0\n"); return 0; }

    const int npairs = claims::fixed_pairs(k.has_commitment != 0), nfix = groups ? claims::fixed_groups(k.has_commitment != 0) : npairs;
    std::vector<e2> slots(few::kSlots * few::kGroup);
    const HG g{slots.data()};
    for (size_t p = 0; p < parts.size(); p++) {
        const claims::Part pt = parts[p];
        const uint32_t len = pt.end - pt.begin;
        // k_verify_claims_sums: lane partials, then the tree over the lanes that hold one
        int width = claims::tree_width(len);
        G1X sums[kBatchSums] = {g1_inf(), g1_inf(), g1_inf(), g1_inf()};
        for (int j = 0; j < nsums; j++) {
            G1X red[claims::kLanes];
            for (int lane = 0; lane < claims::kLanes; lane++) red[lane] = claims::lane_sum(terms.data(), j, pt, lane);
            for (int h = width / 2; h > 0; h >>= 1) for (int lane = 0; lane < h; lane++) red[lane] = g1_add(red[lane], red[lane + h]);
            sums[j] = red[0];
        }
        uint64_t col[4] = {0, 0, 0, 0};
        for (int lane = 0; lane < width; lane++) {
            uint64_t c[4]; claims::lane_rho(rnd.data(), okv.data(), pt, lane, c);
            for (int w = 0; w < 4; w++) col[w] += c[w];
        }
        uint32_t rho[5]; rho_sum_words(col, rho);
        // k_verify_claims_fixed, then the Miller values of the fixed pairs: by pair, or by 8-lane group
        VP1 fixed[kBatchFixed];
        for (int j = 0; j < kBatchFixed; j++) fixed[j] = batch_fixed_point(k, j, sums, rho);
        F12 pf[kBatchFixed];
        for (int t = 0; t < nfix; t++) {
            if (groups) few::store12(g, claims::miller_fixed_few(g, k, fixed, t, true), &pf[t]);
            else pf[t] = batch_miller_fixed(k, t, fixed[t]);
        }
        // k_verify_claims_product and k_verify_claims_final
        F12 red[claims::kLanes];
        width = claims::tree_width(len > (uint32_t)nfix ? len : (uint32_t)nfix);
        for (int lane = 0; lane < claims::kLanes; lane++) red[lane] = claims::lane_product(f.data(), pf, nfix, pt, lane);
        for (int h = width / 2; h > 0; h >>= 1) for (int lane = 0; lane < h; lane++) red[lane] = mul12(red[lane], red[lane + h]);
        bool accept = claims::final_few(g, &red[0], true);
        for (uint32_t i = pt.begin; i < pt.end; i++) accept = accept && okv[i];
        if (!accept) verdict[owner[p]] = 0;
    }
    printf("ok %d\nclaims", nok);
    for (uint32_t j = 0; j < m; j++) printf(" %d", verdict[j]);
    printf("\n");
    return 0;
}
