// Key ceremony, second phase (phase2_gpu.hpp): a contribution to a Groth16 key pair and the check of one.
// The host walks and splices the key files and handles the record (phase2.hpp); every point is decoded on the device by the verifier's
// key-point kernel (canonical coordinates, the curve equation, G2 in the subgroup); the scaling by the secret, the verifier's random
// combinations and the pairings run on the device (k_phase2.hip, k_verify*.hip).  Every call has a stream and buffers of its own on
// GSC_DEVICE / the first of GSC_DEVICES, so calls may run beside each other and beside proving.
#include "phase2_gpu.hpp"
#include "phase2.hpp"
#include "ceremony_gpu.hpp"

long long gsc_verify_debug_pairing_impl(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out, bool few);      // verify_gpu.cpp

namespace gsc {
using namespace vfy;
using hostf::Fr;
namespace P2 = phase2;
using namespace cer;

namespace {

#define HIP_CHECK GSC_CER_HIP_CHECK

// scalars that are toxic waste: cleared when the scope is left, normally or by an exception
struct Secrets {
    Fr x = Fr::zero(), x_inv = Fr::zero(), k = Fr::zero(), t = Fr::zero();
    uint8_t words[3][32];      // x, 1/x, k as little-endian canonical bytes: the device's scalar images
    Secrets() { memset(words, 0, sizeof words); }
    Secrets(const Secrets&) = delete; Secrets& operator=(const Secrets&) = delete;
    ~Secrets() { explicit_bzero(&x, sizeof x); explicit_bzero(&x_inv, sizeof x_inv); explicit_bzero(&k, sizeof k); explicit_bzero(&t, sizeof t); explicit_bzero(words, sizeof words); }
};

// G1.Delta (64 B) and G2.Delta (128 B) of a decoded file; false when either is the point at infinity
bool deltas(const DevKey& k, uint8_t d1[64], uint8_t d2[128], hipStream_t s) {
    uint8_t i1 = 0, i2 = 0;
    download(k.p1() + k.w.d1, 1, d1, &i1, s); download(k.p2() + k.w.d2, 1, d2, &i2, s);
    return !i1 && !i2;
}
}  // namespace

int phase2_contribute(const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len, const uint8_t* seed32, Phase2Step& out) {
    const char* who = "gsc_setup_contribute";
    P2::Walk wp, wv; std::string err;
    if (!P2::walk_pk(pk, pk_len, wp, err) || !P2::walk_vk(vk, vk_len, wv, err)) return refuse(who, err, -2);
    need_device();
    Stream st; hipStream_t s = st.s;
    DevKey kp(wp), kv(wv);
    if (!decode_file(pk, kp, s)) return refuse(who, "pk: bad point", -2);
    if (!decode_file(vk, kv, s)) return refuse(who, "vk: bad point", -2);
    uint8_t d1[64], d2[128], e1[64], e2[128];
    if (!deltas(kp, d1, d2, s) || !deltas(kv, e1, e2, s)) return refuse(who, "delta is the point at infinity", -2);
    if (memcmp(d1, e1, 64) || memcmp(d2, e2, 128)) return refuse(who, "pk and vk disagree on delta", -2);

    Secrets sec;
    if (seed32) {
        if (!P2::seeded_scalar("gsc-phase2-x", seed32, sec.x) || !P2::seeded_scalar("gsc-phase2-k", seed32, sec.k)) return refuse(who, "the seed gives a zero scalar", -2);
    } else { sec.x = random_nonzero_fr(); sec.k = random_nonzero_fr(); }
    sec.x_inv = sec.x.inv();
    fr_to_le(sec.x, sec.words[0]); fr_to_le(sec.x_inv, sec.words[1]); fr_to_le(sec.k, sec.words[2]);
    Buf d_sec(sizeof sec.words, true);      // the scalars on the device: zeroed before the buffer is freed, whatever happens below
    HIP_CHECK(hipMemcpyAsync(d_sec.p, sec.words, sizeof sec.words, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint32_t *dx = d_sec.as<uint32_t>(), *dxi = dx + 8, *dk = dx + 16;

    // the rewritten G1 points in the walk's order: Delta' = x Delta, then Z' and K' = (1/x) Z, K (the two sets lie side by side in the walk)
    const size_t nzk = wp.nz + wp.nk, n1 = 1 + nzk;
    if (wp.k0 != wp.z0 + wp.nz) throw std::runtime_error("internal: Z and K apart");
    Buf o1(sizeof(VP1) * n1), o2(sizeof(VP2)), oT(sizeof(VP1));
    launch_scale_points(kp.p1() + wp.d1, 1, dx, o1.as<VP1>(), s);
    launch_scale_points(kp.p1() + wp.z0, nzk, dxi, o1.as<VP1>() + 1, s);
    launch_scale_points(kp.p2() + wp.d2, 1, dx, o2.as<VP2>(), s);
    launch_scale_points(kp.p1() + wp.d1, 1, dk, oT.as<VP1>(), s);
    HIP_CHECK(hipGetLastError());
    std::vector<uint8_t> g1(64 * n1), inf1(n1);
    uint8_t nd2[128], T[64], i2, iT;
    download(o1.as<VP1>(), n1, g1.data(), inf1.data(), s);
    download(o2.as<VP2>(), 1, nd2, &i2, s);
    download(oT.as<VP1>(), 1, T, &iT, s);
    if (inf1[0] || i2 || iT) throw std::runtime_error("internal: a multiple of delta is the point at infinity");

    out.pk = P2::splice(pk, pk_len, wp, g1.data(), inf1.data(), nd2);
    out.vk = P2::splice(vk, vk_len, wv, g1.data(), inf1.data(), nd2);
    P2::Record r;
    sha256_digest(pk, pk_len, r.h_prev); sha256_digest(out.pk.data(), out.pk.size(), r.h_next);
    memcpy(r.delta, g1.data(), 64); memcpy(r.T, T, 64);
    uint8_t c_be[32]; P2::challenge(r.h_prev, d1, r.delta, r.T, c_be);
    Fr c; Fr::from_be(c_be, c);
    sec.t = sec.k + c * sec.x;
    sec.t.to_be(r.z);
    P2::encode_record(r, out.record);
    return 0;
}

int phase2_verify(const uint8_t* pk_prev, size_t pk_prev_len, const uint8_t* vk_prev, size_t vk_prev_len, const uint8_t* pk_next, size_t pk_next_len,
                  const uint8_t* vk_next, size_t vk_next_len, const uint8_t* record) {
    const char* who = "gsc_setup_verify_contribution";
    // rule 1: the four files parse and every point decodes; neither delta is the point at infinity
    P2::Walk wpp, wvp, wpn, wvn; std::string err;
    if (!P2::walk_pk(pk_prev, pk_prev_len, wpp, err) || !P2::walk_vk(vk_prev, vk_prev_len, wvp, err)) return refuse(who, "rule 1: prev " + err);
    if (!P2::walk_pk(pk_next, pk_next_len, wpn, err) || !P2::walk_vk(vk_next, vk_next_len, wvn, err)) return refuse(who, "rule 1: next " + err);
    need_device();
    Stream st; hipStream_t s = st.s;
    DevKey kpp(wpp), kvp(wvp), kpn(wpn), kvn(wvn);
    if (!decode_file(pk_prev, kpp, s) || !decode_file(vk_prev, kvp, s)) return refuse(who, "rule 1: prev: bad point");
    if (!decode_file(pk_next, kpn, s) || !decode_file(vk_next, kvn, s)) return refuse(who, "rule 1: next: bad point");
    uint8_t dp1[64], dp2[128], dvp1[64], dvp2[128], dn1[64], dn2[128], dvn1[64], dvn2[128];
    if (!deltas(kpp, dp1, dp2, s) || !deltas(kvp, dvp1, dvp2, s) || !deltas(kpn, dn1, dn2, s) || !deltas(kvn, dvn1, dvn2, s)) return refuse(who, "rule 1: delta is the point at infinity");
    // rule 2: everything but delta, Z and K is unchanged, byte for byte
    if (!P2::same_outside(pk_prev, pk_prev_len, wpp, pk_next, pk_next_len, wpn)) return refuse(who, "rule 2: the proving keys differ outside delta, Z and K");
    if (!P2::same_outside(vk_prev, vk_prev_len, wvp, vk_next, vk_next_len, wvn)) return refuse(who, "rule 2: the verifying keys differ outside delta");
    // rule 3: pk and vk of a pair carry the same deltas
    if (memcmp(dn1, dvn1, 64) || memcmp(dn2, dvn2, 128)) return refuse(who, "rule 3: next pk and vk disagree on delta");
    if (memcmp(dp1, dvp1, 64) || memcmp(dp2, dvp2, 128)) return refuse(who, "rule 3: prev pk and vk disagree on delta");
    // rule 4: the record speaks of these files
    const P2::Record r = P2::decode_record(record);
    uint8_t h[32];
    sha256_digest(pk_prev, pk_prev_len, h); if (memcmp(h, r.h_prev, 32)) return refuse(who, "rule 4: the record's hash of the previous proving key");
    sha256_digest(pk_next, pk_next_len, h); if (memcmp(h, r.h_next, 32)) return refuse(who, "rule 4: the record's hash of the next proving key");
    if (memcmp(r.delta, dn1, 64)) return refuse(who, "rule 4: the record's delta");
    // rule 5: z Delta_prev == T + c Delta'
    {
        Fr z; if (!Fr::from_be(r.z, z)) return refuse(who, "rule 5: z is not below r");
        std::vector<uint8_t> ts(r.T, r.T + 64), none; Buf dT(sizeof(VP1));
        if ((r.T[0] & 0xC0) || P2::all_zero(r.T, 64) || !decode_slots(ts, 1, none, 0, dT.as<VP1>(), nullptr, s)) return refuse(who, "rule 5: T is not a finite raw G1 point");
        uint8_t c_be[32], lhs[64], cd[64], rhs[64];
        P2::challenge(r.h_prev, dp1, r.delta, r.T, c_be);
        scale_one(kpp.p1() + wpp.d1, r.z, lhs, s);
        scale_one(kpn.p1() + wpn.d1, c_be, cd, s);
        if (!P2::g1_add_raw(r.T, cd, rhs) || memcmp(lhs, rhs, 64)) return refuse(who, "rule 5: the proof of knowledge does not hold");
    }
    // rules 6 and 7: four reduced pairings on the device, compared in pairs (two products, not one joined by a random factor)
    const size_t n = wpp.nz + wpp.nk;
    uint8_t sums[2][64] = {{0}}, sinf[2] = {1, 1};
    if (n) {
        const std::vector<uint32_t> rho = random_rho(n);
        Buf d_rho(16 * n), part(sizeof(G1X) * 2 * phase2_rlc_blocks(n)), d_sums(2 * sizeof(VP1));
        HIP_CHECK(hipMemcpyAsync(d_rho.p, rho.data(), 16 * n, hipMemcpyHostToDevice, s));
        launch_phase2_rlc(kpp.p1() + wpp.z0, kpn.p1() + wpn.z0, d_rho.as<uint32_t>(), n, part.as<G1X>(), d_sums.as<VP1>(), s);
        HIP_CHECK(hipGetLastError());
        download(d_sums.as<VP1>(), 2, &sums[0][0], sinf, s);
    }
    uint8_t p1[4][64], p2[4][128], f[4][384];
    generators(p1[1], p2[0]);
    memcpy(p1[0], dn1, 64);                                    // e(Delta'_1, G_2)
    memcpy(p2[1], dn2, 128);                                   // e(G_1, Delta'_2)
    memcpy(p1[2], sums[1], 64); memcpy(p2[2], dn2, 128);       // e(sum rho P', Delta'_2)
    memcpy(p1[3], sums[0], 64); memcpy(p2[3], dp2, 128);       // e(sum rho P, Delta_prev_2)
    HIP_CHECK(hipStreamSynchronize(s));
    if (gsc_verify_debug_pairing_impl(&p1[0][0], &p2[0][0], 4, &f[0][0], true) != 4) throw std::runtime_error("the pairings failed on the device");
    if (memcmp(f[0], f[1], 384)) return refuse(who, "rule 6: the two deltas of the next key are not the same multiple of the generators");
    if (memcmp(f[2], f[3], 384)) return refuse(who, "rule 7: Z and K were not scaled by the inverse of delta's factor");
    return 1;
}

void phase2_debug_scale(int group, const uint8_t* pts, const uint8_t* inf, size_t n, const uint8_t* scalar_be32, uint8_t* out, uint8_t* out_inf) {
    if (group < 0 || group > 1 || n > (1u << 20)) throw std::runtime_error("gsc_debug_scale_points: no such group / too many points");
    Fr k; if (!Fr::from_be(scalar_be32, k)) throw std::runtime_error("gsc_debug_scale_points: the scalar is not below r");
    if (!n) return;
    need_device();
    Stream st; hipStream_t s = st.s;
    const size_t W = group ? 128 : 64;
    std::vector<uint8_t> slots(W * n, 0), none;
    for (size_t i = 0; i < n; i++) if (!inf[i]) {
        if ((pts[W * i] & 0xC0) || P2::all_zero(pts + W * i, W)) throw std::runtime_error("gsc_debug_scale_points: a point that is not raw and finite");
        memcpy(slots.data() + W * i, pts + W * i, W);
    }
    uint8_t le[32]; for (int i = 0; i < 32; i++) le[i] = scalar_be32[31 - i];
    Buf dk(32, true);
    HIP_CHECK(hipMemcpyAsync(dk.p, le, 32, hipMemcpyHostToDevice, s));
    explicit_bzero(le, sizeof le);
    if (group == 0) {
        Buf in(sizeof(VP1) * n), o(sizeof(VP1) * n);
        if (!decode_slots(slots, n, none, 0, in.as<VP1>(), nullptr, s)) throw std::runtime_error("gsc_debug_scale_points: bad point");
        launch_scale_points(in.as<VP1>(), n, dk.as<uint32_t>(), o.as<VP1>(), s);
        HIP_CHECK(hipGetLastError());
        download(o.as<VP1>(), n, out, out_inf, s);
    } else {
        Buf in(sizeof(VP2) * n), o(sizeof(VP2) * n);
        if (!decode_slots(none, 0, slots, n, nullptr, in.as<VP2>(), s)) throw std::runtime_error("gsc_debug_scale_points: bad point");
        launch_scale_points(in.as<VP2>(), n, dk.as<uint32_t>(), o.as<VP2>(), s);
        HIP_CHECK(hipGetLastError());
        download(o.as<VP2>(), n, out, out_inf, s);
    }
}

}  // namespace gsc
