// Key ceremony, first phase (srs_contrib_gpu.hpp): a contribution to a powers file and the check of one.  The host walks
// the files (srs.hpp) and handles the record (srs_contrib.hpp); every element is decoded on the device by the verifier's key-point kernel;
// the powers m x^i of the secrets are computed on the device (k_fr_powers) and never reach the host; every element is multiplied by its own
// power in the branch-free ladder (k_scale_points, per-point scalars).  The host holds the three secrets, the three nonces and the three z.
#include "srs_contrib_gpu.hpp"
#include "srs_contrib.hpp"
#include "srs_gpu.hpp"
#include "ceremony_gpu.hpp"
#include <chrono>
#include <cstdlib>

namespace gsc {
using namespace vfy;
using namespace cer;
using hostf::Fr;
namespace SC = srsc;

namespace {

#define HIP_CHECK GSC_CER_HIP_CHECK

// scalars that are toxic waste: cleared when the scope is left, normally or by an exception
struct Secrets {
    Fr s[3], k[3], z[3];       // tau', alpha', beta'; their Schnorr nonces; z_s = k_s + c_s s'
    uint8_t words[7][32];      // s[0..3), 1, k[0..3) as little-endian canonical bytes: the device's scalar images
    Secrets() { for (int i = 0; i < 3; i++) s[i] = k[i] = z[i] = Fr::zero(); memset(words, 0, sizeof words); }
    Secrets(const Secrets&) = delete; Secrets& operator=(const Secrets&) = delete;
    ~Secrets() { explicit_bzero(s, sizeof s); explicit_bzero(k, sizeof k); explicit_bzero(z, sizeof z); explicit_bzero(words, sizeof words); }
};

// GSC_SRS_TRACE=1: wall time per kind of work on stdout (every stage then waits for the stream; tools/time_srs_contribute.py reads the lines)
struct Trace {
    const char* who; bool on; std::chrono::steady_clock::time_point last;
    enum { kDecode, kPowers, kLadder1, kLadder2, kDownload, kKinds };
    double ms[kKinds] = {0, 0, 0, 0, 0};
    explicit Trace(const char* w) : who(w), on(getenv("GSC_SRS_TRACE") != nullptr), last(std::chrono::steady_clock::now()) {}
    void add(int kind, hipStream_t s) {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        ms[kind] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    }
    void print() const {
        if (on) printf("%s: decode %.1f ms, powers %.1f ms, G1 ladders %.1f ms, G2 ladders %.1f ms, download %.1f ms\n", who, ms[kDecode], ms[kPowers], ms[kLadder1], ms[kLadder2], ms[kDownload]);
    }
};

// out[i] = m x^(first + i) in[i] for i < n: the powers into `rows` (a secret buffer of at least 32 n bytes), then the per-point ladder.  The
// one launch sequence: a contribution calls it per section, gsc_debug_scale_powers calls it on a caller's points.
template <class P> void scale_by_powers(const P* in, size_t n, const uint32_t* x, const uint32_t* m, uint64_t first, const Buf& rows, P* out, hipStream_t s, Trace& tr) {
    if (rows.bytes < 32 * n) throw std::runtime_error("internal: the row buffer is too small for its section");
    launch_fr_powers(x, m, first, n, rows.as<uint32_t>(), s);
    HIP_CHECK(hipGetLastError());
    tr.add(Trace::kPowers, s);
    launch_scale_points_each(in, n, rows.as<uint32_t>(), out, s);
    HIP_CHECK(hipGetLastError());
    tr.add(sizeof(P) == sizeof(VP2) ? Trace::kLadder2 : Trace::kLadder1, s);
}

const char* const kNotAPoint = " is not a point of its group (a coordinate not below p, off the curve, or G2 outside the subgroup)";

}  // namespace

int srs_contribute(const uint8_t* f, size_t len, const uint8_t* seed32, std::vector<uint8_t>& out, uint8_t* record) {
    const char* who = "gsc_srs_contribute";
    // the input gets rule 1 of gsc_srs_verify: the host walk, and every element decoded on the device
    srs::Layout l; std::string err;
    if (!srs::walk(f, len, l, err)) return refuse(who, err, -2);
    need_device();
    Stream st; hipStream_t s = st.s;
    Trace tr(who);
    const size_t N = l.N, n1 = l.n_g1(), n2 = l.n_g2(), idx[3] = {1, l.i_alpha1(), l.i_beta1()};      // tauG1[1], alphaG1[0], betaG1[0]
    std::vector<uint8_t> s1, s2;
    srs::slots(f, l, s1, s2);
    Buf g1(sizeof(VP1) * n1), g2(sizeof(VP2) * n2);
    const long long bad = decode_slots_first_bad(s1, n1, s2, n2, g1.as<VP1>(), g2.as<VP2>(), s);
    if (bad >= 0) return refuse(who, "srs: " + ((size_t)bad < n1 ? srs::g1_name(l, (size_t)bad) : srs::g2_name(l, (size_t)bad - n1)) + kNotAPoint, -2);
    tr.add(Trace::kDecode, s);

    Secrets sec;
    for (int i = 0; i < 3; i++) {
        if (seed32) { if (!SC::seeded_scalars(i, seed32, sec.s[i], sec.k[i])) return refuse(who, "the seed gives a zero scalar", -2); }
        else { sec.s[i] = random_nonzero_fr(); sec.k[i] = random_nonzero_fr(); }
        fr_to_le(sec.s[i], sec.words[i]); fr_to_le(sec.k[i], sec.words[4 + i]);
    }
    fr_to_le(Fr::one(), sec.words[3]);
    Buf d_sec(sizeof sec.words, true);      // the scalars on the device: zeroed before the buffer is freed, whatever happens below
    HIP_CHECK(hipMemcpyAsync(d_sec.p, sec.words, sizeof sec.words, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint32_t *d_tau = d_sec.as<uint32_t>(), *d_alpha = d_tau + 8, *d_beta = d_tau + 16, *d_one = d_tau + 24, *d_k = d_tau + 32;

    // section by section, in stream order, through one row buffer sized for the longest section (tauG1, 2N - 1 rows)
    Buf rows(32 * l.n_tau1(), true), o1(sizeof(VP1) * n1), o2(sizeof(VP2) * n2), oT(3 * sizeof(VP1));
    const VP1* p1 = g1.as<VP1>(); const VP2* p2 = g2.as<VP2>();
    VP1* q1 = o1.as<VP1>(); VP2* q2 = o2.as<VP2>();
    scale_by_powers(p1, l.n_tau1(), d_tau, d_one, 0, rows, q1, s, tr);                                // tauG1'[i] = tau'^i tauG1[i]
    scale_by_powers(p1 + l.i_alpha1(), N, d_tau, d_alpha, 0, rows, q1 + l.i_alpha1(), s, tr);         // alphaG1'[i] = alpha' tau'^i alphaG1[i]
    scale_by_powers(p1 + l.i_beta1(), N, d_tau, d_beta, 0, rows, q1 + l.i_beta1(), s, tr);            // betaG1'[i] = beta' tau'^i betaG1[i]
    for (int i = 0; i < 3; i++) launch_scale_points(p1 + idx[i], 1, d_k + 8 * i, oT.as<VP1>() + i, s);   // T_s = k_s base_s
    HIP_CHECK(hipGetLastError());
    tr.add(Trace::kLadder1, s);
    scale_by_powers(p2, N, d_tau, d_one, 0, rows, q2, s, tr);                                         // tauG2'[i] = tau'^i tauG2[i]
    launch_scale_points(p2 + l.i_beta2(), 1, d_beta, q2 + l.i_beta2(), s);                            // betaG2' = beta' betaG2
    HIP_CHECK(hipGetLastError());
    tr.add(Trace::kLadder2, s);

    std::vector<uint8_t> b1(64 * n1), i1(n1), b2(128 * n2), i2(n2);
    uint8_t T[3][64], iT[3];
    download(q1, n1, b1.data(), i1.data(), s);
    download(q2, n2, b2.data(), i2.data(), s);
    download(oT.as<VP1>(), 3, &T[0][0], iT, s);
    tr.add(Trace::kDownload, s);
    for (uint8_t v : i1) if (v) throw std::runtime_error("internal: a multiple of an element is the point at infinity");
    for (uint8_t v : i2) if (v) throw std::runtime_error("internal: a multiple of an element is the point at infinity");
    if (iT[0] || iT[1] || iT[2]) throw std::runtime_error("internal: a multiple of an element is the point at infinity");
    out = srs::assemble(l, b1.data(), b2.data());

    SC::Record r;
    sha256_digest(f, len, r.h_prev); sha256_digest(out.data(), out.size(), r.h_next);
    for (int i = 0; i < 3; i++) {
        memcpy(r.s[i].elem, &b1[64 * idx[i]], 64); memcpy(r.s[i].T, T[i], 64);
        uint8_t c_be[32]; SC::challenge(i, r.h_prev, &s1[64 * idx[i]], r.s[i].elem, r.s[i].T, c_be);      // prev's bytes are canonical: the decoder accepted them
        Fr c; Fr::from_be(c_be, c);
        sec.z[i] = sec.k[i] + c * sec.s[i];
        sec.z[i].to_be(r.s[i].z);
    }
    SC::encode_record(r, record);
    tr.print();
    return 0;
}

int srs_verify_contribution(const uint8_t* prev, size_t prev_len, const uint8_t* next, size_t next_len, const uint8_t* record) {
    const char* who = "gsc_srs_verify_contribution";
    // rule 1: both files pass the host walk and have the same L; prev's tauG1[1], alphaG1[0], betaG1[0] decode
    srs::Layout lp, ln; std::string err;
    if (!srs::walk(prev, prev_len, lp, err)) return refuse(who, "rule 1: prev: " + err);
    if (!srs::walk(next, next_len, ln, err)) return refuse(who, "rule 1: next: " + err);
    if (lp.L != ln.L) return refuse(who, "rule 1: prev and next differ in L");
    need_device();
    Stream st; hipStream_t s = st.s;
    const size_t idx[3] = {1, lp.i_alpha1(), lp.i_beta1()};
    const uint8_t *base[3], *elem[3];
    for (int i = 0; i < 3; i++) { base[i] = prev + srs::g1_offset(lp, idx[i]); elem[i] = next + srs::g1_offset(ln, idx[i]); }
    std::vector<uint8_t> sl(64 * 6), none;
    for (int i = 0; i < 3; i++) { memcpy(&sl[64 * i], base[i], 64); memcpy(&sl[64 * (3 + i)], elem[i], 64); }
    Buf pts(6 * sizeof(VP1));
    const long long bad = decode_slots_first_bad(sl, 6, none, 0, pts.as<VP1>(), nullptr, s);
    if (bad >= 0 && bad < 3) return refuse(who, "rule 1: prev: srs: " + srs::g1_name(lp, idx[bad]) + kNotAPoint);
    // rule 2: the record speaks of these files
    const SC::Record r = SC::decode_record(record);
    uint8_t h[32];
    sha256_digest(prev, prev_len, h); if (memcmp(h, r.h_prev, 32)) return refuse(who, "rule 2: the record's hash of the previous file");
    sha256_digest(next, next_len, h); if (memcmp(h, r.h_next, 32)) return refuse(who, "rule 2: the record's hash of the next file");
    // rule 3: the record's new elements are the next file's
    for (int i = 0; i < 3; i++) if (memcmp(r.s[i].elem, elem[i], 64)) return refuse(who, std::string("rule 3: the record's ") + SC::name_of(i) + " element is not the next file's " + srs::g1_name(ln, idx[i]));
    // rule 4: z_s base_s == T_s + c_s new_s.  (A new element that does not decode leaves the equation without a side: rule 5 names it.)
    for (int i = 0; i < 3 && bad < 0; i++) {
        const std::string rule = std::string("rule 4: ") + SC::name_of(i) + ": ";
        Fr z; if (!SC::z_below_r(r.s[i].z, z)) return refuse(who, rule + "z is not below r");
        std::vector<uint8_t> ts(r.s[i].T, r.s[i].T + 64); Buf dT(sizeof(VP1));
        if (!SC::T_is_raw_and_finite(r.s[i].T) || !decode_slots(ts, 1, none, 0, dT.as<VP1>(), nullptr, s)) return refuse(who, rule + "T is not a finite raw G1 point");
        uint8_t c_be[32], lhs[64], cn[64], rhs[64];
        SC::challenge(i, r.h_prev, base[i], r.s[i].elem, r.s[i].T, c_be);
        scale_one(pts.as<VP1>() + i, r.s[i].z, lhs, s);
        scale_one(pts.as<VP1>() + 3 + i, c_be, cn, s);
        if (!phase2::g1_add_raw(r.s[i].T, cn, rhs) || memcmp(lhs, rhs, 64)) return refuse(who, rule + "the proof of knowledge does not hold");
    }
    // rule 5: next is a powers file, all of gsc_srs_verify.  With rule 4: the powers of (tau tau', alpha alpha', beta beta').
    const int ok = srs_verify(next, next_len, who, "rule 5: next: ");
    if (ok == 1 && bad >= 0) throw std::runtime_error("internal: an element that does not decode was accepted");
    return ok;
}

void srs_debug_scale_powers(int group, const uint8_t* pts, const uint8_t* inf, size_t n, const uint8_t* x_be32, const uint8_t* m_be32, uint64_t first,
                            uint8_t* out, uint8_t* out_inf) {
    const char* who = "gsc_debug_scale_powers";
    if (group < 0 || group > 1 || n > (1u << 20) || first > (1ull << 62)) throw std::runtime_error(std::string(who) + ": no such group / too many points / first too large");
    Fr x, m;
    if (!Fr::from_be(x_be32, x) || !Fr::from_be(m_be32, m)) throw std::runtime_error(std::string(who) + ": a scalar is not below r");
    if (!n) return;
    need_device();
    Stream st; hipStream_t s = st.s;
    Trace tr(who);
    const size_t W = group ? 128 : 64;
    std::vector<uint8_t> slots(W * n, 0), none;
    for (size_t i = 0; i < n; i++) if (!inf[i]) {
        if ((pts[W * i] & 0xC0) || phase2::all_zero(pts + W * i, W)) throw std::runtime_error(std::string(who) + ": a point that is not raw and finite");
        memcpy(slots.data() + W * i, pts + W * i, W);
    }
    uint8_t le[2][32];
    fr_to_le(x, le[0]); fr_to_le(m, le[1]);
    Buf d_xm(sizeof le, true), rows(32 * n, true);
    HIP_CHECK(hipMemcpyAsync(d_xm.p, le, sizeof le, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    explicit_bzero(le, sizeof le);
    const uint32_t *dx = d_xm.as<uint32_t>(), *dm = dx + 8;
    if (group == 0) {
        Buf in(sizeof(VP1) * n), o(sizeof(VP1) * n);
        if (!decode_slots(slots, n, none, 0, in.as<VP1>(), nullptr, s)) throw std::runtime_error(std::string(who) + ": bad point");
        scale_by_powers(in.as<VP1>(), n, dx, dm, first, rows, o.as<VP1>(), s, tr);
        download(o.as<VP1>(), n, out, out_inf, s);
    } else {
        Buf in(sizeof(VP2) * n), o(sizeof(VP2) * n);
        if (!decode_slots(none, 0, slots, n, nullptr, in.as<VP2>(), s)) throw std::runtime_error(std::string(who) + ": bad point");
        scale_by_powers(in.as<VP2>(), n, dx, dm, first, rows, o.as<VP2>(), s, tr);
        download(o.as<VP2>(), n, out, out_inf, s);
    }
}

}  // namespace gsc
