// Key ceremony, the Pedersen sigma of a commitment key (sigma_gpu.hpp): the check of a pair's Pedersen relation, a sigma
// contribution, the check of one, and the check of a pair against the Setup from a powers file.  The host walks and splices the key files
// and handles the record (sigma.hpp on phase2.hpp); the device work is the ceremony's and the verifier's kernels through their launchers —
// the key-point decoder, the uniform-scalar ladder, the random combinations, the few-proof pairing — and no kernel of its own.  Every call
// has a stream and buffers of its own on GSC_DEVICE / the first of GSC_DEVICES, so calls may run beside each other and beside proving.
#include "sigma_gpu.hpp"
#include "sigma.hpp"
#include "srs_gpu.hpp"
#include "ceremony_gpu.hpp"
#include <memory>

long long gsc_verify_debug_pairing_impl(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out, bool few);      // verify_gpu.cpp

namespace gsc {
using namespace vfy;
using hostf::Fr;
namespace P2 = phase2;
namespace S = sigma;
using namespace cer;

namespace {

#define HIP_CHECK GSC_CER_HIP_CHECK

// scalars that are toxic waste: cleared when the scope is left, normally or by an exception
struct Secrets {
    Fr x = Fr::zero(), k = Fr::zero(), t = Fr::zero();
    uint8_t words[2][32];      // x, k as little-endian canonical bytes: the device's scalar images
    Secrets() { memset(words, 0, sizeof words); }
    Secrets(const Secrets&) = delete; Secrets& operator=(const Secrets&) = delete;
    ~Secrets() { explicit_bzero(&x, sizeof x); explicit_bzero(&k, sizeof k); explicit_bzero(&t, sizeof t); explicit_bzero(words, sizeof words); }
};

// one pair (pk, vk), walked on the host and decoded on the device
struct Pair {
    const uint8_t *pk = nullptr, *vk = nullptr; size_t pk_len = 0, vk_len = 0;
    P2::Walk wp, wv;
    std::unique_ptr<DevKey> kp, kv;
    // the host half of rule 1: both files parse and each holds its commitment key.  Empty: accepted; else the reason.
    std::string parse(const uint8_t* p, size_t pn, const uint8_t* v, size_t vn) {
        pk = p; pk_len = pn; vk = v; vk_len = vn;
        std::string err;
        if (!P2::walk_pk(pk, pk_len, wp, err) || !P2::walk_vk(vk, vk_len, wv, err)) return err;
        if (!wp.ped || !wv.ped) return "no commitment key";
        return std::string();
    }
    // the device half: every point of both files decodes; then what sigma.hpp pair_shape asks
    std::string decode(hipStream_t s, bool with_infinities = true) {
        kp.reset(new DevKey(wp)); kv.reset(new DevKey(wv));
        if (!decode_file(pk, *kp, s)) return "pk: bad point";
        if (!decode_file(vk, *kv, s)) return "vk: bad point";
        return S::pair_shape(pk, wp, vk, wv, with_infinities);
    }
    VP1* basis() const { return kp->p1() + wp.pb0; }
    VP1* bes() const { return kp->p1() + wp.ps0; }
};

// Rule 2 of gsc_pedersen_verify: e(sum rho_j BasisExpSigma_j, G) == e(-sum rho_j Basis_j, GSigmaNeg), the rho_j drawn as the verifier draws
// its own; one launch of the random combinations, two reduced pairings in one launch of the few-proof kernels, compared as canonical values
bool relation_holds(const Pair& p, hipStream_t s) {
    const size_t n = p.wp.npb;
    uint8_t sums[2][64] = {{0}}, sinf[2] = {1, 1};
    if (n) {
        const std::vector<uint32_t> rho = verifier_rho(n);
        Buf d_rho(16 * n), part(sizeof(G1X) * 2 * phase2_rlc_blocks(n)), d_sums(2 * sizeof(VP1));
        HIP_CHECK(hipMemcpyAsync(d_rho.p, rho.data(), 16 * n, hipMemcpyHostToDevice, s));
        launch_phase2_rlc(p.basis(), p.bes(), d_rho.as<uint32_t>(), n, part.as<G1X>(), d_sums.as<VP1>(), s);
        HIP_CHECK(hipGetLastError());
        download(d_sums.as<VP1>(), 2, &sums[0][0], sinf, s);
    }
    uint8_t p1[2][64], p2[2][128], f[2][384], i2[2];
    memcpy(p1[0], sums[1], 64);
    if (!S::g1_neg_raw(sums[0], p1[1])) throw std::runtime_error("internal: a sum with a coordinate not below p");
    download(p.kv->p2() + p.wv.pg, 2, &p2[0][0], i2, s);      // G and GSigmaNeg lie side by side in the walk
    if (p.wv.pgsn != p.wv.pg + 1) throw std::runtime_error("internal: G and GSigmaNeg apart");
    HIP_CHECK(hipStreamSynchronize(s));
    if (gsc_verify_debug_pairing_impl(&p1[0][0], &p2[0][0], 2, &f[0][0], true) != 2) throw std::runtime_error("the pairings failed on the device");
    return !memcmp(f[0], f[1], 384);
}

}  // namespace

int pedersen_verify(const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len) {
    const char* who = "gsc_pedersen_verify";
    Pair p; std::string err = p.parse(pk, pk_len, vk, vk_len);
    if (!err.empty()) return refuse(who, "rule 1: " + err);
    need_device();
    Stream st; hipStream_t s = st.s;
    err = p.decode(s);
    if (!err.empty()) return refuse(who, "rule 1: " + err);
    if (!relation_holds(p, s)) return refuse(who, "rule 2: the Pedersen relation does not hold");
    return 1;
}

int sigma_contribute(const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len, const uint8_t* seed32, SigmaStep& out) {
    const char* who = "gsc_setup_contribute_sigma";
    Pair p; std::string err = p.parse(pk, pk_len, vk, vk_len);
    if (!err.empty()) return refuse(who, err, -2);
    need_device();
    Stream st; hipStream_t s = st.s;
    err = p.decode(s);
    if (!err.empty()) return refuse(who, err, -2);
    const P2::Walk &wp = p.wp, &wv = p.wv;
    const size_t n = wp.npb, j0 = S::first_finite(pk, wp);      // pair_shape: some element is finite, so j0 < n

    Secrets sec;
    if (seed32) { if (!S::seeded_scalars(seed32, sec.x, sec.k)) return refuse(who, "the seed gives a zero scalar", -2); }
    else { sec.x = random_nonzero_fr(); sec.k = random_nonzero_fr(); }
    fr_to_le(sec.x, sec.words[0]); fr_to_le(sec.k, sec.words[1]);
    Buf d_sec(sizeof sec.words, true);      // the scalars on the device: zeroed before the buffer is freed, whatever happens below
    HIP_CHECK(hipMemcpyAsync(d_sec.p, sec.words, sizeof sec.words, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint32_t *dx = d_sec.as<uint32_t>(), *dk = dx + 8;

    // BasisExpSigma' = x BasisExpSigma, GSigmaNeg' = x GSigmaNeg, T = k base (the nonce is a secret too: it goes the ladder's way from the
    // wiped buffer, not through scale_one's public one)
    Buf o1(sizeof(VP1) * n), o2(sizeof(VP2)), oT(sizeof(VP1));
    launch_scale_points(p.bes(), n, dx, o1.as<VP1>(), s);
    launch_scale_points(p.kv->p2() + wv.pgsn, 1, dx, o2.as<VP2>(), s);
    launch_scale_points(p.bes() + j0, 1, dk, oT.as<VP1>(), s);
    HIP_CHECK(hipGetLastError());
    std::vector<uint8_t> g1(64 * n), inf1(n);
    uint8_t base[64], gsn[128], T[64], ib, i2, iT;
    download(o1.as<VP1>(), n, g1.data(), inf1.data(), s);
    download(o2.as<VP2>(), 1, gsn, &i2, s);
    download(oT.as<VP1>(), 1, T, &iT, s);
    download(p.bes() + j0, 1, base, &ib, s);
    if (ib || inf1[j0] || i2 || iT) throw std::runtime_error("internal: a multiple of a finite point is the point at infinity");

    out.pk = S::splice_pk(pk, pk_len, wp, g1.data(), inf1.data());
    out.vk = S::splice_vk(vk, vk_len, wv, gsn);
    S::Record r;
    sha256_digest(pk, pk_len, r.h_prev); sha256_digest(out.pk.data(), out.pk.size(), r.h_next);
    memcpy(r.delta, g1.data() + 64 * j0, 64); memcpy(r.T, T, 64);
    uint8_t c_be[32]; S::challenge(r.h_prev, base, r.delta, r.T, c_be);
    Fr c; Fr::from_be(c_be, c);
    sec.t = sec.k + c * sec.x;
    sec.t.to_be(r.z);
    S::encode_record(r, out.record);
    return 0;
}

int sigma_verify(const uint8_t* pk_prev, size_t pk_prev_len, const uint8_t* vk_prev, size_t vk_prev_len, const uint8_t* pk_next, size_t pk_next_len,
                 const uint8_t* vk_next, size_t vk_next_len, const uint8_t* record) {
    const char* who = "gsc_setup_verify_sigma_contribution";
    // rule 1: rule 1 of gsc_pedersen_verify on both pairs.  (On next the clause on the infinities' positions is rule 3's: with rule 1 on
    // prev and rule 2 it says the same.)
    Pair prev, next; std::string err;
    if (!(err = prev.parse(pk_prev, pk_prev_len, vk_prev, vk_prev_len)).empty()) return refuse(who, "rule 1: prev: " + err);
    if (!(err = next.parse(pk_next, pk_next_len, vk_next, vk_next_len)).empty()) return refuse(who, "rule 1: next: " + err);
    need_device();
    Stream st; hipStream_t s = st.s;
    if (!(err = prev.decode(s)).empty()) return refuse(who, "rule 1: prev: " + err);
    if (!(err = next.decode(s, false)).empty()) return refuse(who, "rule 1: next: " + err);
    // rule 2: everything but BasisExpSigma and GSigmaNeg is unchanged, byte for byte
    if (!S::same_outside_sigma(pk_prev, pk_prev_len, prev.wp, pk_next, pk_next_len, next.wp)) return refuse(who, "rule 2: the proving keys differ outside BasisExpSigma");
    if (!S::same_outside_sigma(vk_prev, vk_prev_len, prev.wv, vk_next, vk_next_len, next.wv)) return refuse(who, "rule 2: the verifying keys differ outside GSigmaNeg");
    // rule 3: the record speaks of these files
    const S::Record r = S::decode_record(record);
    uint8_t h[32];
    sha256_digest(pk_prev, pk_prev_len, h); if (memcmp(h, r.h_prev, 32)) return refuse(who, "rule 3: the record's hash of the previous proving key");
    sha256_digest(pk_next, pk_next_len, h); if (memcmp(h, r.h_next, 32)) return refuse(who, "rule 3: the record's hash of the next proving key");
    if (!S::same_infinities(pk_prev, prev.wp, pk_next, next.wp)) return refuse(who, "rule 3: BasisExpSigma has its infinities at other positions");
    const size_t j0 = S::first_finite(pk_prev, prev.wp);
    uint8_t base[64], nw[64], ib, in;
    download(prev.bes() + j0, 1, base, &ib, s); download(next.bes() + j0, 1, nw, &in, s);
    if (ib || in) throw std::runtime_error("internal: the first finite element is the point at infinity");
    if (memcmp(r.delta, nw, 64)) return refuse(who, "rule 3: the record's new element");
    // rule 4: z base == T + c new
    {
        Fr z; if (!Fr::from_be(r.z, z)) return refuse(who, "rule 4: z is not below r");
        std::vector<uint8_t> ts(r.T, r.T + 64), none; Buf dT(sizeof(VP1));
        if ((r.T[0] & 0xC0) || P2::all_zero(r.T, 64) || !decode_slots(ts, 1, none, 0, dT.as<VP1>(), nullptr, s)) return refuse(who, "rule 4: T is not a finite raw G1 point");
        uint8_t c_be[32], lhs[64], cn[64], rhs[64];
        S::challenge(r.h_prev, base, r.delta, r.T, c_be);
        scale_one(prev.bes() + j0, r.z, lhs, s);
        scale_one(next.bes() + j0, c_be, cn, s);
        if (!P2::g1_add_raw(r.T, cn, rhs) || memcmp(lhs, rhs, 64)) return refuse(who, "rule 4: the proof of knowledge does not hold");
    }
    // rule 5: the Pedersen relation on next.  PREV'S IS DELIBERATELY NOT RE-CHECKED (include/libprove.h).
    if (!relation_holds(next, s)) return refuse(who, "rule 5: the Pedersen relation does not hold on the next pair");
    return 1;
}

int setup_verify_from_srs(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* srs, size_t srs_len, const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len) {
    const char* who = "gsc_setup_verify_from_srs";
    const SetupKeys k = setup_from_srs(r1cs, r1cs_len, srs, srs_len, nullptr);      // the production path, as it is
    // rule 1: the given pair is the recomputed one outside what a production Setup draws afresh
    P2::Walk wp, wv, gp, gv; std::string err;
    if (!P2::walk_pk(k.pk.data(), k.pk.size(), wp, err) || !P2::walk_vk(k.vk.data(), k.vk.size(), wv, err)) throw std::runtime_error("internal: the recomputed pair does not parse: " + err);
    if (!P2::walk_pk(pk, pk_len, gp, err) || !P2::walk_vk(vk, vk_len, gv, err)) return refuse(who, "rule 1: " + err);
    if (!S::same_outside_fresh(k.pk.data(), k.pk.size(), wp, pk, pk_len, gp)) return refuse(who, "rule 1: the proving key is not the powers file's outside BasisExpSigma");
    if (!S::same_outside_fresh(k.vk.data(), k.vk.size(), wv, vk, vk_len, gv)) return refuse(who, "rule 1: the verifying key is not the powers file's outside G and GSigmaNeg");
    if (!wp.ped) return 1;
    // rule 2: gsc_pedersen_verify's rules on the given pair
    Pair p;
    if (!(err = p.parse(pk, pk_len, vk, vk_len)).empty()) return refuse(who, "rule 2: " + err);
    Stream st; hipStream_t s = st.s;
    if (!(err = p.decode(s)).empty()) return refuse(who, "rule 2: " + err);
    if (!relation_holds(p, s)) return refuse(who, "rule 2: the Pedersen relation does not hold");
    return 1;
}

}  // namespace gsc
