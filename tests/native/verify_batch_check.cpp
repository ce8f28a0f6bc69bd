// Host build of the batched check's per-thread code (csrc/verify_batch_dev.hpp, compiled by g++ with the HIP headers): builds a key
// the way k_verify.hip does, prepares every item with prep_one, then runs the steps of k_verify_batch.hip one item at a time and
// prints the chunk's verdict.  tests/test_verify_batch_host.py drives it.
//   stdin : algorithm (0/1/2) | randomizers (0: OS entropy, 1: all ones) | vk length (u32 LE) | vk | n (u32 LE) |
//           n x (proof length u32 LE | 196-byte slot | 144 signal bytes)
//   stdout: "ok <items that decode>" then "batch 0" / "batch 1"; "key 0" when the key is refused
#include "verify_batch_dev.hpp"
#include "verify_common.hpp"
#include <cstdio>
#include <random>
#include <vector>

using namespace gsc::vfy;
namespace V = gsc::verify;

static uint32_t rd32(FILE* f) { uint8_t b[4]; if (fread(b, 1, 4, f) != 4) return 0; return b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24; }

int main() {
    const int algo = fgetc(stdin), ones = fgetc(stdin);
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

    // k_verify_batch_scale / _miller, one item at a time; the sums in one accumulator each (the device adds them up in a tree)
    std::random_device dev;
    const int nsums = k.has_commitment ? kBatchSums : 2;
    G1X sums[kBatchSums] = {g1_inf(), g1_inf(), g1_inf(), g1_inf()};
    uint64_t col[4] = {0, 0, 0, 0};
    F12 prod = one12();
    int nok = 0;
    const uint32_t n = rd32(stdin);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t slot[kProofSlot], sig[V::kSignalBytes], win[V::kWindows];
        const uint32_t len = rd32(stdin);
        if (fread(slot, 1, sizeof slot, stdin) != sizeof slot || fread(sig, 1, sizeof sig, stdin) != sizeof sig) return 2;
        ProofDev p{};
        if (V::proof_shape_ok(slot, len, lay.has_commitment)) { V::public_windows(algo, sig, win); prep_one(k, slot, win, p); }
        if (!p.ok) continue;
        nok++;
        uint32_t r[kRandWords] = {0};
        for (int h = 0; h < nsums / 2; h++) {
            uint32_t any = 0;
            while (!any) for (int w = 0; w < 4; w++) any |= r[4 * h + w] = ones ? (w == 0) : (uint32_t)dev();
        }
        const VP1 ra = batch_scaled_a(p, r);
        for (int j = 0; j < nsums; j++) sums[j] = g1_add(sums[j], batch_term(p, j, r));
        for (int w = 0; w < 4; w++) col[w] += r[w];
        prod = mul12(prod, batch_miller_proof(p, ra));
    }
    // k_verify_batch_sum, the fixed pairs of k_verify_batch_miller, k_verify_batch_final
    uint32_t rho[5]; rho_sum_words(col, rho);
    for (int j = 0; j < kBatchFixed; j++) prod = mul12(prod, batch_miller_fixed(k, j, batch_fixed_point(k, j, sums, rho)));
    printf("ok %d\nbatch %d\n", nok, (int)batch_accept(prod));
    return 0;
}
