// Host build of the self-check's per-thread code (csrc/verify_dev.hpp prep_affine_one, the body of k_check_prep, compiled by g++ with the HIP
// headers) beside prep_one, the body of k_verify_prep.  The key's tables are built the way k_verify.hip builds them.
//   argv[1] = "twin":   stdin algorithm (0/1/2) | vk length (u32 LE) | vk | n (u32 LE) | n x (proof length u32 LE | 196-byte slot | 144 signal bytes)
//                       stdout per item: "<ok of prep_one> <ok of prep_affine_one> <1: the two ProofDev are equal word for word> <hex image>", where the
//                       image is the prover's layout of the points prep_one decoded: 256 B A | B | C as little-endian words, 64 B D, 64 B PoK big-endian
//   argv[1] = "affine": the same header, then n x (384-byte image | 144 signal bytes); stdout per item: ok of prep_affine_one
// tests/test_prove_check_host.py drives both.  Stand-alone: it can be built with -fsanitize=address,undefined as it is.
#include "verify_common.hpp"
#include "verify_dev.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace gsc::vfy;
namespace V = gsc::verify;

static uint32_t rd32(FILE* f) { uint8_t b[4]; if (fread(b, 1, 4, f) != 4) return 0; return b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24; }
static void put_le(const e1& v, uint8_t* o) { const fe w = F::pack(F::from_mont(v)); for (int i = 0; i < 8; i++) for (int j = 0; j < 4; j++) o[4 * i + j] = (uint8_t)(w.l[i] >> (8 * j)); }
static void put_be(const e1& v, uint8_t* o) { uint8_t le[32]; put_le(v, le); for (int i = 0; i < 32; i++) o[i] = le[31 - i]; }

int main(int argc, char** argv) {
    const bool twin = argc > 1 && !strcmp(argv[1], "twin");
    if (!twin && !(argc > 1 && !strcmp(argv[1], "affine"))) return 2;
    const int algo = fgetc(stdin);
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
    for (int i = 0; i < 5; i++) { k.qinf[i] = q[i].inf; k.lines[i] = nullptr; }      // (no pairing here: the lines are not needed)
    k.table = table.data(); k.ctable = ctable.data();
    const uint32_t n = rd32(stdin);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t sig[V::kSignalBytes], win[V::kWindows], img[384];
        ProofDev a, b;
        memset(&a, 0, sizeof a); memset(&b, 0, sizeof b); memset(img, 0, sizeof img);
        if (twin) {
            uint8_t slot[kProofSlot];
            const uint32_t len = rd32(stdin);
            if (fread(slot, 1, sizeof slot, stdin) != sizeof slot || fread(sig, 1, sizeof sig, stdin) != sizeof sig) return 2;
            V::public_windows(algo, sig, win);
            if (V::proof_shape_ok(slot, len, lay.has_commitment)) prep_one(k, slot, win, a);
            if (a.ok) {
                put_le(a.A.x, img); put_le(a.A.y, img + 32);
                put_le(a.B.x.a0, img + 64); put_le(a.B.x.a1, img + 96); put_le(a.B.y.a0, img + 128); put_le(a.B.y.a1, img + 160);
                put_le(a.C.x, img + 192); put_le(a.C.y, img + 224);
                if (k.has_commitment) { put_be(a.D.x, img + 256); put_be(a.D.y, img + 288); put_be(a.pok.x, img + 320); put_be(a.pok.y, img + 352); }
                prep_affine_one(k, img, img + 256, img + 320, win, b);
            }
            printf("%d %d %d ", (int)a.ok, (int)b.ok, (int)(memcmp(&a, &b, sizeof a) == 0));
            for (uint8_t v : img) printf("%02x", v);
            printf("\n");
        } else {
            if (fread(img, 1, sizeof img, stdin) != sizeof img || fread(sig, 1, sizeof sig, stdin) != sizeof sig) return 2;
            V::public_windows(algo, sig, win);
            prep_affine_one(k, img, img + 256, img + 320, win, b);
            printf("%d\n", (int)b.ok);
        }
    }
    return 0;
}
