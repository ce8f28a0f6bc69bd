// The check of a powers file (srs_gpu.hpp).  The host finds the sections (srs.hpp); every element is decoded on the
// device by the verifier's key-point kernel (canonical coordinates, the curve equation, G2 in the subgroup); the random combinations of
// each vector with itself shifted by one (k_phase2.hip, G1 and G2) and the ten pairings (k_verify_few.hip) run on the device.  The host
// does no group and no field arithmetic on the file's points: it compares bytes.
// Then the Setup from such a file (setup_from_srs): the Lagrange bases at tau by the group transform (group_idft.hpp), the column sums
// A, B, K and Z by k_srs_columns.hip over the host's term lists (srs_columns.hpp), the keys by setup.cpp's one writer; and the test hooks.
#include "srs_gpu.hpp"
#include "srs.hpp"
#include "setup.hpp"
#include "ceremony_gpu.hpp"
#include "group_idft.hpp"
#include "srs_columns.hpp"
#include "srs_columns_kernels.hpp"
#include <chrono>
#include <cstdlib>

long long gsc_verify_debug_pairing_impl(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out, bool few);      // verify_gpu.cpp

namespace gsc {
using namespace vfy;
using namespace cer;
using hostf::Fr;

#define HIP_CHECK GSC_CER_HIP_CHECK

int srs_verify(const uint8_t* f, size_t len, const char* who, const std::string& prefix) {
    auto no = [&](const std::string& why) { return refuse(who, prefix + why); };
    // rule 1: magic, L, length; every element raw and finite (host), canonical, on the curve, G2 in the subgroup (device)
    srs::Layout l; std::string err;
    if (!srs::walk(f, len, l, err)) return no("rule 1: " + err);
    need_device();
    Stream st; hipStream_t s = st.s;
    const size_t N = l.N, n1 = l.n_g1(), n2 = l.n_g2();
    std::vector<uint8_t> s1, s2;
    srs::slots(f, l, s1, s2);
    Buf g1(sizeof(VP1) * n1), g2(sizeof(VP2) * n2);
    const long long bad = decode_slots_first_bad(s1, n1, s2, n2, g1.as<VP1>(), g2.as<VP2>(), s);
    if (bad >= 0) {
        const std::string name = (size_t)bad < n1 ? srs::g1_name(l, (size_t)bad) : srs::g2_name(l, (size_t)bad - n1);
        return no("rule 1: srs: " + name + " is not a point of its group (a coordinate not below p, off the curve, or G2 outside the subgroup)");
    }
    // rule 2: the vectors start at the generators (the bytes are canonical by rule 1, so equal points are equal bytes)
    uint8_t G1[64], G2[128];
    generators(G1, G2);
    if (memcmp(s1.data(), G1, 64)) return no("rule 2: tauG1[0] is not the G1 generator");
    if (memcmp(s2.data(), G2, 128)) return no("rule 2: tauG2[0] is not the G2 generator");

    // rules 3-6: for each vector v of m + 1 elements, S0 = sum rho_i v[i] and S1 = sum rho_i v[i + 1] over i < m, fresh rho for each
    const size_t m_tau = 2 * N - 2, m = N - 1;
    const std::vector<uint32_t> rho = random_rho(m_tau + 3 * m);
    Buf d_rho(16 * (m_tau + 3 * m)), part1(sizeof(G1X) * 2 * phase2_rlc_blocks(m_tau)), part2(sizeof(G2X) * 2 * phase2_rlc_blocks(m)), d_s1(6 * sizeof(VP1)), d_s2(2 * sizeof(VP2));
    HIP_CHECK(hipMemcpyAsync(d_rho.p, rho.data(), 16 * (m_tau + 3 * m), hipMemcpyHostToDevice, s));
    const uint32_t* r = d_rho.as<uint32_t>();
    const VP1 *tau1 = g1.as<VP1>(), *alpha1 = tau1 + l.i_alpha1(), *beta1 = tau1 + l.i_beta1();
    const VP2* tau2 = g2.as<VP2>();
    launch_phase2_rlc(tau1, tau1 + 1, r, m_tau, part1.as<G1X>(), d_s1.as<VP1>(), s);
    launch_phase2_rlc(alpha1, alpha1 + 1, r + 4 * m_tau, m, part1.as<G1X>(), d_s1.as<VP1>() + 2, s);
    launch_phase2_rlc(beta1, beta1 + 1, r + 4 * (m_tau + m), m, part1.as<G1X>(), d_s1.as<VP1>() + 4, s);
    launch_phase2_rlc(tau2, tau2 + 1, r + 4 * (m_tau + 2 * m), m, part2.as<G2X>(), d_s2.as<VP2>(), s);
    HIP_CHECK(hipGetLastError());
    uint8_t sum1[6][64], inf1[6], sum2[2][128], inf2[2];
    download(d_s1.as<VP1>(), 6, &sum1[0][0], inf1, s);
    download(d_s2.as<VP2>(), 2, &sum2[0][0], inf2, s);

    // ten reduced pairings in one launch, compared in pairs as canonical values (an all-zero point is infinity: its pairing is 1)
    const uint8_t *tau1_1 = s1.data() + 64, *tau2_1 = s2.data() + 128, *beta1_0 = s1.data() + 64 * l.i_beta1(), *beta2 = s2.data() + 128 * l.i_beta2();
    uint8_t p1[10][64], p2[10][128];
    std::vector<uint8_t> fv(10 * 384);
    auto pair = [&](int i, const uint8_t* a, const uint8_t* b) { memcpy(p1[i], a, 64); memcpy(p2[i], b, 128); };
    pair(0, sum1[1], G2);      pair(1, sum1[0], tau2_1);      // rule 3: e(sum rho tauG1[i+1], G2) = e(sum rho tauG1[i], tauG2[1])
    pair(2, G1, sum2[1]);      pair(3, tau1_1, sum2[0]);      // rule 4: e(G1, sum rho tauG2[i+1]) = e(tauG1[1], sum rho tauG2[i])
    pair(4, sum1[3], G2);      pair(5, sum1[2], tau2_1);      // rule 5: alphaG1
    pair(6, sum1[5], G2);      pair(7, sum1[4], tau2_1);      // rule 6: betaG1
    pair(8, beta1_0, G2);      pair(9, G1, beta2);            // rule 7: e(betaG1[0], G2) = e(G1, betaG2)
    if (gsc_verify_debug_pairing_impl(&p1[0][0], &p2[0][0], 10, fv.data(), true) != 10) throw std::runtime_error("the pairings failed on the device");
    auto same = [&](int i) { return !memcmp(fv.data() + 384 * i, fv.data() + 384 * (i + 1), 384); };
    if (!same(0)) return no("rule 3: tauG1 is not the powers of tauG2[1]'s tau over the G1 generator");
    if (!same(2)) return no("rule 4: tauG2 is not the powers of tauG1[1]'s tau over the G2 generator");
    if (!same(4)) return no("rule 5: alphaG1 is not alphaG1[0] times the powers of tau");
    if (!same(6)) return no("rule 6: betaG1 is not betaG1[0] times the powers of tau");
    if (!same(8)) return no("rule 7: betaG2 and betaG1[0] are not the same multiple of the generators");
    return 1;
}

namespace {
// n raw finite points of one group (G1: 64 B, G2: 128 B) -> decoded points on the device; throws when one is refused
template <class P> void upload_points(const char* who, const uint8_t* pts, size_t n, P* out, hipStream_t s) {
    constexpr bool g2 = sizeof(P) == sizeof(VP2);
    constexpr size_t W = g2 ? 128 : 64;
    for (size_t i = 0; i < n; i++) if ((pts[W * i] & 0xC0) || srs::detail::all_zero(pts + W * i, W)) throw std::runtime_error(std::string(who) + ": a point that is not raw and finite");
    const std::vector<uint8_t> slots(pts, pts + W * n), none;
    const bool ok = g2 ? decode_slots(none, 0, slots, n, nullptr, reinterpret_cast<VP2*>(out), s) : decode_slots(slots, n, none, 0, reinterpret_cast<VP1*>(out), nullptr, s);
    if (!ok) throw std::runtime_error(std::string(who) + ": bad point");
}
template <class P> void debug_idft(int L, const uint8_t* pts, uint8_t* out, uint8_t* out_inf, hipStream_t s) {
    const size_t n = (size_t)1 << L;
    Buf in(sizeof(P) * n), o(sizeof(P) * n), scratch(group_idft_scratch_bytes(L, sizeof(P) == sizeof(VP2)));
    upload_points("gsc_debug_group_idft", pts, n, in.as<P>(), s);
    launch_group_idft(in.as<P>(), L, scratch.p, o.as<P>(), s);
    HIP_CHECK(hipGetLastError());
    download(o.as<P>(), n, out, out_inf, s);
}
template <class T> void upload(Buf& b, const std::vector<T>& v, hipStream_t s) { if (!v.empty()) HIP_CHECK(hipMemcpyAsync(b.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, s)); }
// one matrix by columns on the device: the checked term lists and their segments (srs_columns.hpp)
struct DevMatrix {
    srs::Segments seg; uint32_t n_cols;
    Buf seg_begin, seg_end, col_seg, term_row, term_coeff;
    static const srs::Segments& cut(srs::Segments& sg, const char* who, const uint32_t* col_start, size_t n_cols, const uint32_t* rows, const uint32_t* coeffs, size_t n_terms, size_t n_rows, size_t n_coeff) {
        if (n_cols >= (1u << 28) || n_terms >= (1u << 30) || !srs::cut_columns(col_start, n_cols, n_terms, sg)) throw std::runtime_error(std::string(who) + ": column offsets that are not a partition of the terms");
        for (size_t i = 0; i < n_terms; i++) if (rows[i] >= n_rows || coeffs[i] >= n_coeff) throw std::runtime_error(std::string(who) + ": a term's row or coefficient id out of range");
        return sg;
    }
    DevMatrix(const char* who, const uint32_t* col_start, size_t ncols, const uint32_t* rows, const uint32_t* coeffs, size_t n_terms, size_t n_rows, size_t n_coeff, hipStream_t s)
        : n_cols((uint32_t)ncols), seg_begin(4 * cut(seg, who, col_start, ncols, rows, coeffs, n_terms, n_rows, n_coeff).begin.size()), seg_end(4 * seg.end.size()),
          col_seg(4 * seg.col_seg.size()), term_row(4 * n_terms), term_coeff(4 * n_terms) {
        upload(seg_begin, seg.begin, s); upload(seg_end, seg.end, s); upload(col_seg, seg.col_seg, s);
        if (n_terms) { HIP_CHECK(hipMemcpyAsync(term_row.p, rows, 4 * n_terms, hipMemcpyHostToDevice, s)); HIP_CHECK(hipMemcpyAsync(term_coeff.p, coeffs, 4 * n_terms, hipMemcpyHostToDevice, s)); }
        HIP_CHECK(hipStreamSynchronize(s));
    }
    ColumnArgs args(const Buf& mag, const Buf& meta) const {
        return ColumnArgs{seg_begin.as<uint32_t>(), seg_end.as<uint32_t>(), col_seg.as<uint32_t>(), term_row.as<uint32_t>(), term_coeff.as<uint32_t>(), mag.as<uint32_t>(), meta.as<uint32_t>(),
                          (uint32_t)seg.begin.size(), n_cols};
    }
};
template <class P> void debug_columns(const uint8_t* rows, size_t n_rows, const DevMatrix& m, const Buf& mag, const Buf& meta, uint8_t* out, uint8_t* out_inf, hipStream_t s) {
    constexpr bool g2 = sizeof(P) == sizeof(VP2);
    Buf in(sizeof(P) * n_rows), o(sizeof(P) * m.n_cols), part(column_part_bytes((uint32_t)m.seg.begin.size(), g2));
    upload_points("gsc_debug_column_sums", rows, n_rows, in.as<P>(), s);
    launch_column_sums(in.as<P>(), m.args(mag, meta), part.p, o.as<P>(), s);
    HIP_CHECK(hipGetLastError());
    download(o.as<P>(), m.n_cols, out, out_inf, s);
}
}  // namespace

void srs_debug_column_sums(int group, uint32_t n_rows, const uint8_t* rows, uint32_t n_cols, const uint32_t* col_start, const uint32_t* term_row, const uint32_t* term_coeff,
                           uint32_t n_coeff, const uint8_t* coeff_be, uint8_t* out, uint8_t* out_inf) {
    const char* who = "gsc_debug_column_sums";
    if (group < 0 || group > 1 || n_rows > (1u << 20) || n_cols > (1u << 20)) throw std::runtime_error(std::string(who) + ": no such group / too many rows or columns");
    if (!n_cols) return;
    srs::CoeffTable ct;
    if (!srs::prepare_coeffs(coeff_be, n_coeff, ct)) throw std::runtime_error(std::string(who) + ": a coefficient that is not below r");
    need_device();
    Stream st; hipStream_t s = st.s;
    const DevMatrix m(who, col_start, n_cols, term_row, term_coeff, col_start[n_cols], n_rows, n_coeff, s);
    Buf mag(4 * ct.mag.size()), meta(4 * ct.meta.size());
    upload(mag, ct.mag, s); upload(meta, ct.meta, s);
    if (group == 0) debug_columns<VP1>(rows, n_rows, m, mag, meta, out, out_inf, s);
    else debug_columns<VP2>(rows, n_rows, m, mag, meta, out, out_inf, s);
}

namespace {
void rev32(const uint8_t* a, uint8_t* b) { for (int i = 0; i < 32; i++) b[i] = a[31 - i]; }
// raw big-endian points (download) -> the writer's canonical little-endian lists (G2: X.A1 | X.A0 | Y.A1 | Y.A0 -> x.a0, x.a1, y.a0, y.a1)
void be_to_le_g1(const uint8_t* be, uint8_t* le) { rev32(be, le); rev32(be + 32, le + 32); }
void be_to_le_g2(const uint8_t* be, uint8_t* le) { rev32(be + 32, le); rev32(be, le + 32); rev32(be + 96, le + 64); rev32(be + 64, le + 96); }
void fr_le(const Fr& v, uint8_t* out) { hostf::U256 c = v.canon(); memcpy(out, c.w, 32); explicit_bzero(&c, sizeof c); }
template <class P> void columns_into(const P* rows, const DevMatrix& m, const Buf& mag, const Buf& meta, P* out, hipStream_t s) {
    Buf part(column_part_bytes((uint32_t)m.seg.begin.size(), sizeof(P) == sizeof(VP2)));
    launch_column_sums(rows, m.args(mag, meta), part.p, out, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));      // part is freed here
}
void print_columns(const char* name, const srs::Matrix& M) {
    const size_t nw = M.col_start.size() - 1;
    printf("gsc_setup_from_srs: matrix %s: %zu terms in %zu columns, longest %zu, mean %.2f\n", name, M.n_terms(), nw, M.longest(), nw ? (double)M.n_terms() / (double)nw : 0.0);
}
}  // namespace

SetupKeys setup_from_srs(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* f, size_t len, const uint8_t* seed32) {
    const char* who = "gsc_setup_from_srs";
    Fr::init(); hostf::Fp::init();
    R1csFile cs; srs::Matrix M[3];
    try { cs = parse_r1cs(r1cs, r1cs_len); srs::build_matrices(cs, M); } catch (const std::exception& e) { throw SrsRefused(e.what()); }
    if (cs.n_public_committed) throw SrsRefused("setup: public committed wires are not supported");
    const size_t m = cs.n_constraints, nw = cs.n_wires(), npub = cs.n_public, ncp = cs.commit_private.size(), nc = cs.n_coeff();
    size_t n = 1; int lg = 0; while (n < m) { n <<= 1; lg++; }
    if (lg > srs::kMaxLog) throw SrsRefused("setup: constraint system too large");
    if (lg < 1) throw SrsRefused("setup: a circuit of fewer than two constraints");
    const bool trace = getenv("GSC_SETUP_TRACE") != nullptr;      // stage wall times and the column histogram on stdout
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](const char* name, hipStream_t st_) {
        if (!trace) return;
        if (st_) (void)hipStreamSynchronize(st_);
        const auto now = std::chrono::steady_clock::now();
        printf("gsc_setup_from_srs: %s %.1f ms\n", name, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    if (srs_verify(f, len) != 1) throw SrsRefused("the powers file is refused");
    stage("file check", nullptr);
    srs::Layout l; std::string err;
    if (!srs::walk(f, len, l, err)) throw SrsRefused(err);
    if (l.L < lg) throw SrsRefused("the powers file is too small for this circuit (L < log2 n)");
    if (trace) { print_columns("L", M[0]); print_columns("R", M[1]); print_columns("O", M[2]); }
    const SetupLists ls(nw, n, ncp);

    // coefficients: the circuit's (stored in Montgomery form) as canonical bytes, then 1 and r - 1 for Z
    std::vector<uint8_t> cbe(32 * (nc + 2), 0);
    for (size_t i = 0; i < nc; i++) { Fr c; memcpy(c.v.w, cs.coeff_limbs.data() + 8 * i, 32); c.to_be(&cbe[32 * i]); }
    Fr::one().to_be(&cbe[32 * nc]); Fr::one().neg().to_be(&cbe[32 * (nc + 1)]);
    srs::CoeffTable ct;
    if (!srs::prepare_coeffs(cbe.data(), nc + 2, ct)) throw std::runtime_error("internal: a coefficient not below r");

    need_device();
    Stream st; hipStream_t s = st.s;
    // the elements this circuit uses: tauG1[0, 2n-1) | alphaG1[0, n) | betaG1[0, n) and tauG2[0, n) | betaG2
    const size_t u1 = 4 * n - 1, u2 = n + 1;
    std::vector<uint8_t> s1(64 * u1), s2(128 * u2);
    memcpy(s1.data(), f + l.off_tau1, 64 * (2 * n - 1)); memcpy(s1.data() + 64 * (2 * n - 1), f + l.off_alpha1, 64 * n); memcpy(s1.data() + 64 * (3 * n - 1), f + l.off_beta1, 64 * n);
    memcpy(s2.data(), f + l.off_tau2, 128 * n); memcpy(s2.data() + 128 * n, f + l.off_beta2, 128);
    Buf g1(sizeof(VP1) * u1), g2(sizeof(VP2) * u2);
    if (!decode_slots(s1, u1, s2, u2, g1.as<VP1>(), g2.as<VP2>(), s)) throw std::runtime_error("internal: a verified element does not decode");
    const VP1 *tau1 = g1.as<VP1>(), *alpha1 = tau1 + (2 * n - 1), *beta1 = alpha1 + n;
    const VP2 *tau2 = g2.as<VP2>(), *beta2 = tau2 + n;

    // Lagrange bases at tau: [L beta | L alpha | L G1] side by side (the rows of K's matrix), and L G2
    Buf lag1(sizeof(VP1) * 3 * n), lag2(sizeof(VP2) * n), scratch(group_idft_scratch_bytes(lg, true));
    launch_group_idft(beta1, lg, scratch.p, lag1.as<VP1>(), s);
    launch_group_idft(alpha1, lg, scratch.p, lag1.as<VP1>() + n, s);
    launch_group_idft(tau1, lg, scratch.p, lag1.as<VP1>() + 2 * n, s);
    launch_group_idft(tau2, lg, scratch.p, lag2.as<VP2>(), s);
    HIP_CHECK(hipGetLastError());
    const VP1* LG1 = lag1.as<VP1>() + 2 * n;
    stage("decode and four transforms", s);

    // the matrices: L, R by wire; K = L over L beta + R over L alpha + O over L G1 as one matrix over the 3n rows; Z[pos] = tauG1[k + n] - tauG1[k]
    srs::Matrix MK, MZ;
    MK.col_start.assign(nw + 1, 0);
    for (size_t w = 0; w < nw; w++) {
        for (int side = 0; side < 3; side++) for (uint32_t t = M[side].col_start[w]; t < M[side].col_start[w + 1]; t++) { MK.row.push_back(M[side].row[t] + (uint32_t)(side * n)); MK.coeff.push_back(M[side].coeff[t]); }
        MK.col_start[w + 1] = (uint32_t)MK.row.size();
    }
    MZ.col_start.assign(n, 0);
    for (size_t pos = 0; pos + 1 < n; pos++) {
        size_t k = 0; for (int b = 0; b < lg; b++) if ((pos >> b) & 1) k |= (size_t)1 << (lg - 1 - b);
        MZ.row.push_back((uint32_t)(k + n)); MZ.coeff.push_back((uint32_t)nc); MZ.row.push_back((uint32_t)k); MZ.coeff.push_back((uint32_t)nc + 1);
        MZ.col_start[pos + 1] = (uint32_t)MZ.row.size();
    }
    Buf mag(4 * ct.mag.size()), meta(4 * ct.meta.size());
    upload(mag, ct.mag, s); upload(meta, ct.meta, s);
    Buf pts1(sizeof(VP1) * ls.n1), pts2(sizeof(VP2) * (ls.o2P));
    VP1* q1 = pts1.as<VP1>(); VP2* q2 = pts2.as<VP2>();
    {
        const DevMatrix dL(who, M[0].col_start.data(), nw, M[0].row.data(), M[0].coeff.data(), M[0].n_terms(), n, nc + 2, s);
        columns_into(LG1, dL, mag, meta, q1 + ls.oA, s);
    }
    {
        const DevMatrix dR(who, M[1].col_start.data(), nw, M[1].row.data(), M[1].coeff.data(), M[1].n_terms(), n, nc + 2, s);
        columns_into(LG1, dR, mag, meta, q1 + ls.oB, s);
        columns_into(lag2.as<VP2>(), dR, mag, meta, q2 + ls.o2B, s);
    }
    {
        const DevMatrix dK(who, MK.col_start.data(), nw, MK.row.data(), MK.coeff.data(), MK.n_terms(), 3 * n, nc + 2, s);
        columns_into(lag1.as<VP1>(), dK, mag, meta, q1 + ls.oK, s);
    }
    {
        const DevMatrix dZ(who, MZ.col_start.data(), n - 1, MZ.row.data(), MZ.coeff.data(), MZ.n_terms(), 2 * n - 1, nc + 2, s);
        columns_into(tau1, dZ, mag, meta, q1 + ls.oZ, s);
    }
    stage("column sums A, B1, B2, K and Z", s);
    // single points: alpha, beta, and delta = gamma = the generators (delta = gamma = 1; a seeded TEST Setup replaces them below)
    HIP_CHECK(hipMemcpyAsync(q1 + 0, alpha1, sizeof(VP1), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(q1 + 1, beta1, sizeof(VP1), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(q1 + 2, tau1, sizeof(VP1), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(q2 + 0, beta2, sizeof(VP2), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(q2 + 1, tau2, sizeof(VP2), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(q2 + 2, tau2, sizeof(VP2), hipMemcpyDeviceToDevice, s));

    // secrets: sigma and g of the Pedersen key (whoever runs this call holds sigma), and gamma, delta of a seeded TEST Setup
    uint8_t seed[32];
    struct SeedWipe { uint8_t* p; ~SeedWipe() { explicit_bzero(p, 32); } } seed_wipe{seed};
    if (seed32) memcpy(seed, seed32, 32); else os_random(seed, 32);
    Fr sigma = toxic(seed, "sigma"), ped_g = toxic(seed, "pedersen-g"), gamma = seed32 ? toxic(seed, "gamma") : Fr::one(), delta = seed32 ? toxic(seed, "delta") : Fr::one();
    Fr gamma_inv = gamma.inv(), delta_inv = delta.inv(), nsg = (ped_g * sigma).neg();
    struct FrWipe { std::vector<Fr*> v; ~FrWipe() { for (Fr* x : v) explicit_bzero(x, sizeof *x); } } fr_wipe{{&sigma, &ped_g, &gamma, &delta, &gamma_inv, &delta_inv, &nsg}};
    explicit_bzero(seed, 32);
    uint8_t words[3][32];      // sigma, 1 / gamma, 1 / delta: the device's scalar images
    struct WordsWipe { void* p; ~WordsWipe() { explicit_bzero(p, 96); } } words_wipe{words};
    fr_le(sigma, words[0]); fr_le(gamma_inv, words[1]); fr_le(delta_inv, words[2]);
    Buf d_sec(sizeof words, true);
    HIP_CHECK(hipMemcpyAsync(d_sec.p, words, sizeof words, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint32_t *d_sigma = d_sec.as<uint32_t>(), *d_ginv = d_sigma + 8, *d_dinv = d_sigma + 16;

    std::vector<uint8_t> committed(nw, 0);
    for (uint32_t w : cs.commit_private) committed[w] = 1;
    auto to_vk = [&](size_t i) { return i < npub || (cs.has_commitment && i == cs.commit_wire) || committed[i] != 0; };
    if (seed32) {      // K / gamma or K / delta by wire class, Z / delta: both quotients of K on the device, the choice per wire in place
        Buf Kg(sizeof(VP1) * nw), Kd(sizeof(VP1) * nw), Zd(sizeof(VP1) * (n - 1));
        launch_scale_points(q1 + ls.oK, nw, d_ginv, Kg.as<VP1>(), s);
        launch_scale_points(q1 + ls.oK, nw, d_dinv, Kd.as<VP1>(), s);
        launch_scale_points(q1 + ls.oZ, n - 1, d_dinv, Zd.as<VP1>(), s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(q1 + ls.oK, Kd.p, sizeof(VP1) * nw, hipMemcpyDeviceToDevice, s));
        for (size_t i = 0; i < nw; i++) if (to_vk(i)) HIP_CHECK(hipMemcpyAsync(q1 + ls.oK + i, Kg.as<VP1>() + i, sizeof(VP1), hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(q1 + ls.oZ, Zd.p, sizeof(VP1) * (n - 1), hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    if (ncp) {         // Pedersen: Basis_j = K of the committed wires, BasisExpSigma = sigma Basis (branch-free ladder: sigma is secret)
        Buf basis(sizeof(VP1) * ncp);
        for (size_t j = 0; j < ncp; j++) HIP_CHECK(hipMemcpyAsync(basis.as<VP1>() + j, q1 + ls.oK + cs.commit_private[j], sizeof(VP1), hipMemcpyDeviceToDevice, s));
        launch_scale_points(basis.as<VP1>(), ncp, d_sigma, q1 + ls.oS, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    }

    // down to the host as bytes, into the writer's lists
    std::vector<uint8_t> b1(64 * ls.n1), i1(ls.n1), b2(128 * ls.o2P), i2(ls.n2, 0), p1(64 * ls.n1), p2(128 * ls.n2, 0);
    download(q1, ls.n1, b1.data(), i1.data(), s);
    download(q2, ls.o2P, b2.data(), i2.data(), s);
    for (size_t i = 0; i < ls.n1; i++) be_to_le_g1(&b1[64 * i], &p1[64 * i]);
    for (size_t i = 0; i < ls.o2P; i++) be_to_le_g2(&b2[128 * i], &p2[128 * i]);
    const int device = gsc_verify_device_impl();
    uint8_t g1m[64], g2m[128];
    setup_generators_mont(g1m, g2m);
    {      // generator multiples by scalars this call knows: the Pedersen pair of the vk; delta G1, gamma G2, delta G2 of a seeded TEST Setup
        uint8_t sc[4][32];
        struct ScWipe { void* p; ~ScWipe() { explicit_bzero(p, 128); } } sc_wipe{sc};
        fr_le(ped_g, sc[0]); fr_le(nsg, sc[1]); fr_le(gamma, sc[2]); fr_le(delta, sc[3]);
        uint8_t o2[4][128], f2[4], o1[64], f1;
        if (cs.has_commitment) {
            setup_generator_muls(device, true, g2m, &sc[0][0], 2, &o2[0][0], f2);
            memcpy(&p2[128 * ls.o2P], o2, 256); i2[ls.o2P] = f2[0]; i2[ls.o2P + 1] = f2[1];
        }
        if (seed32) {
            setup_generator_muls(device, true, g2m, &sc[2][0], 2, &o2[0][0], f2);
            memcpy(&p2[128 * 1], o2[0], 128); memcpy(&p2[128 * 2], o2[1], 128);
            setup_generator_muls(device, false, g1m, &sc[3][0], 1, o1, &f1);
            memcpy(&p1[64 * 2], o1, 64);
        }
    }
    stage("scalings, Pedersen, download", s);
    return write_setup_keys(cs, n, p1.data(), i1.data(), p2.data(), i2.data());
}

void srs_debug_group_idft(int group, int L, const uint8_t* pts, uint8_t* out, uint8_t* out_inf) {
    if (group < 0 || group > 1 || L < 1 || L > 17) throw std::runtime_error("gsc_debug_group_idft: no such group / L outside [1, 17]");
    need_device();
    Stream st;
    if (group == 0) debug_idft<VP1>(L, pts, out, out_inf, st.s);
    else debug_idft<VP2>(L, pts, out, out_inf, st.s);
}

std::vector<uint8_t> srs_debug_generate(int L, const uint8_t* seed32, int device) {
    srs::Layout l;
    if (L > 20 || !srs::layout_of(L, l)) throw std::runtime_error("gsc_debug_srs_generate: L outside [1, 20]");
    Fr::init(); hostf::Fp::init();
    const size_t N = l.N, n1 = l.n_g1(), n2 = l.n_g2();
    struct Wipe { std::vector<uint8_t>& v; ~Wipe() { explicit_bzero(v.data(), v.size()); } };
    std::vector<uint8_t> sc1(32 * n1), sc2(32 * n2);
    Wipe w1{sc1}, w2{sc2};
    {
        Fr tau = toxic(seed32, "tau"), alpha = toxic(seed32, "alpha"), beta = toxic(seed32, "beta"), t = Fr::one();
        auto le = [](const Fr& v, uint8_t* out) { hostf::U256 c = v.canon(); memcpy(out, c.w, 32); explicit_bzero(&c, sizeof c); };
        for (size_t i = 0; i < 2 * N - 1; i++, t = t * tau) {
            le(t, &sc1[32 * i]);
            if (i < N) { le(alpha * t, &sc1[32 * (l.i_alpha1() + i)]); le(beta * t, &sc1[32 * (l.i_beta1() + i)]); le(t, &sc2[32 * i]); }
        }
        le(beta, &sc2[32 * l.i_beta2()]);
        for (Fr* v : {&tau, &alpha, &beta, &t}) explicit_bzero(v, sizeof *v);
    }
    uint8_t g1m[64], g2m[128];
    setup_generators_mont(g1m, g2m);
    std::vector<uint8_t> p1(64 * n1), i1(n1), p2(128 * n2), i2(n2);
    setup_generator_muls(device, false, g1m, sc1.data(), n1, p1.data(), i1.data());
    setup_generator_muls(device, true, g2m, sc2.data(), n2, p2.data(), i2.data());
    // canonical little-endian coordinates -> the raw big-endian encoding (G2: x.a0, x.a1, y.a0, y.a1 -> X.A1 | X.A0 | Y.A1 | Y.A0)
    std::vector<uint8_t> b1(64 * n1), b2(128 * n2);
    auto rev = [](const uint8_t* le, uint8_t* be) { for (int i = 0; i < 32; i++) be[i] = le[31 - i]; };
    for (size_t i = 0; i < n1; i++) { rev(&p1[64 * i], &b1[64 * i]); rev(&p1[64 * i + 32], &b1[64 * i + 32]); }
    for (size_t i = 0; i < n2; i++) {
        const uint8_t* p = &p2[128 * i]; uint8_t* o = &b2[128 * i];
        rev(p + 32, o); rev(p, o + 32); rev(p + 96, o + 64); rev(p + 64, o + 96);
    }
    for (uint8_t v : i1) if (v) throw std::runtime_error("gsc_debug_srs_generate: a power of tau is zero");
    for (uint8_t v : i2) if (v) throw std::runtime_error("gsc_debug_srs_generate: a power of tau is zero");
    return srs::assemble(l, b1.data(), b2.data());
}

}  // namespace gsc
