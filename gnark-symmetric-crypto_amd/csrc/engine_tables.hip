// InitAlgorithm-time half of the engine: the solver program, the calibration witness, key decoding and the fixed-base tables, and the
// batch buffers of a lane.  See engine_impl.hpp; reference: prove_impl.go:86-110 (pk.ReadFrom / r1cs.ReadFrom / SetParams).
#include "engine_impl.hpp"
#include "host_ciphers.hpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>

namespace gsc {

AlgorithmImpl::AlgorithmImpl(Cipher c, const uint8_t* pk, size_t pk_len, const uint8_t* r1cs, size_t r1cs_len, const EngineConfig& cf) : cipher(c), cfg(cf) {
    // measured crossover with the batch kernels (one 64-column batch: 12.9 ms ChaCha20, 43.7 ms AES): 32 statements for ChaCha20 (10.2 ms), ~23 for AES (8.2 ms + 1.6 ms each: 38.4 ms for 20)
    if (!cfg.few_max) cfg.few_max = cipher == CHACHA20 ? 32 : 20;
    // the latency kernels' layouts hold MSM_FEW_PROOFS statements, and the route of a chunk (chunk_route.hpp) takes such a call for one 64-column batch
    if (cfg.few_max < 0 || cfg.few_max > (int)MSM_FEW_PROOFS) throw std::runtime_error("EngineConfig::few_max must be in [0, " + std::to_string(MSM_FEW_PROOFS) + "]");
    msm_opts.win_slice = (size_t)cfg.win_slice;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device available: the GPU prover has no CPU fallback");
    HIP_CHECK(hipSetDevice(cfg.device));
    stream = stream_take(cfg.device, STREAM_PLAIN, STREAM_ROLE_INIT);
    // a refused key (a point off the curve or outside the subgroup, a wrong circuit) throws out of this constructor: the members free their
    // device memory as they unwind, and this gives the init stream back, so that a failed InitAlgorithm leaves nothing behind
    struct StreamGuard { hipStream_t& s; int device; bool armed = true; ~StreamGuard() { if (armed && s) { stream_give(device, STREAM_PLAIN, STREAM_ROLE_INIT, s); s = nullptr; } } } stream_guard{stream, cfg.device};
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg.device) == hipSuccess && cus > 0) cu_count = cus; }
    const bool trace = cfg.trace_host;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    R1csFile cs = parse_r1cs(r1cs, r1cs_len);
    PkFile key = parse_pk(pk, pk_len);
    const auto t1 = now();
    {
        const std::unique_ptr<SolverProgram> sp = init_program(cs);
        calibrate();
        init_small(*sp);
    }
    const auto t2 = now();
    init_key(cs, key);
    const auto t3 = now();
    if (trace) fprintf(stderr, "InitAlgorithm(%d): parse %.0f ms, solver program + calibration %.0f ms, key tables %.0f ms (%.1f GiB)\n", (int)c, ms(t0, t1), ms(t1, t2), ms(t2, t3), table_bytes / 1073741824.0);
    // Lanes: every lane can hold a full batch (GSC_MAX_BATCH), so concurrent calls each get a lane of their own and the chunks of a
    // big call spread over the free ones.  Default: one lane for ChaCha20-V3 (its MSMs fill the chip: a second lane gains
    // nothing), two for AES-V2, whose witness stage (445+ level launches of ~56 us and the commitment round trip) is latency-bound and
    // hides under the other lane's NTT / MSM kernels.
    if (cfg.lanes <= 0) cfg.lanes = has_commitment ? 2 : 1;
    const size_t nl = (size_t)cfg.lanes, lane_cap = (cfg.max_batch + 63) / 64 * 64;
    for (size_t i = 0; i < nl; i++) { lanes.emplace_back(new Lane); alloc_lane(*lanes.back(), lane_cap); }
    full_lanes = nl;
    // Small lanes: calls of a few dozen to a few hundred statements leave the chip under-filled in every stage (163 dependent solver
    // levels of ~26 us, Horner and scalar-multiplication chains that do not shrink with the batch), so several of them must be in
    // flight at once — without paying a full lane's memory for each (46 GB at 8192 proofs): extra lanes of SMALL_LANE_CAP proofs
    // (~3 GB each for ChaCha20-V3), taken by calls that fit them.  GSC_SMALL_LANES: default 2 for ChaCha20-V3; AES-V2 has two full lanes already.
    if (cfg.small_lanes < 0) cfg.small_lanes = has_commitment ? 0 : 2;
    // Capacity: 1024 where the full lane is larger than that (two 1024-statement calls side by side prove 6 % more than one after the other on the
    // full lane, profiles/r04m_lanes.txt), 512 otherwise — with GSC_MAX_BATCH <= 1024 the all-resident configuration (three algorithms, 268 GiB)
    // has 4.7 GiB to spare, and 2 x 2.9 GB more would cost the third algorithm one bit of its Z digits (tools/r04_mem_probe.py).
    const size_t small_want = cfg.small_lane_cap ? (size_t)cfg.small_lane_cap : lane_cap > SMALL_LANE_CAP ? SMALL_LANE_CAP : SMALL_LANE_CAP / 2, small_cap = lane_cap > small_want ? small_want : lane_cap;
    for (int i = 0; i < cfg.small_lanes; i++) { lanes.emplace_back(new Lane); alloc_lane(*lanes.back(), small_cap); }
    lane_busy.assign(lanes.size(), 0);
    cap = lane_cap;
    if (trace) fprintf(stderr, "InitAlgorithm(%d): %zu lane(s) of %zu proofs + %d of %zu, %.0f ms\n", (int)c, nl, lane_cap, cfg.small_lanes, small_cap, ms(t3, now()));
    HIP_CHECK(hipStreamSynchronize(stream));
    stream_guard.armed = false;
    // complete: from here to the destructor the replica's tables and lanes count as held on its device (gsc_memory_info)
    accounted = held_bytes();
    prover_bytes_on(cfg.device) += accounted;
}

namespace {
struct StreamPool { std::mutex mu; std::map<std::tuple<int, int, int>, std::vector<hipStream_t>> idle; };
StreamPool& stream_pool() { static StreamPool* const p = new StreamPool; return *p; }      // never destroyed: engines may go after the static destructors
}  // namespace
hipStream_t stream_take(int device, int kind, int role) {
    {
        StreamPool& p = stream_pool(); std::lock_guard<std::mutex> l(p.mu);
        auto it = p.idle.find(std::make_tuple(device, kind, role));
        if (it != p.idle.end() && !it->second.empty()) { hipStream_t s = it->second.back(); it->second.pop_back(); return s; }
    }
    hipStream_t s = nullptr;
    if (kind == STREAM_PLAIN) HIP_CHECK(hipStreamCreate(&s)); else HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamDefault, kind));
    return s;
}
void stream_give(int device, int kind, int role, hipStream_t s) {
    (void)hipStreamSynchronize(s);
    StreamPool& p = stream_pool(); std::lock_guard<std::mutex> l(p.mu);
    p.idle[std::make_tuple(device, kind, role)].push_back(s);
}

std::atomic<size_t>& prover_bytes_on(int device) {
    static std::atomic<size_t> held[64];
    return held[device >= 0 && device < 64 ? device : 63];
}

std::unique_ptr<SolverProgram> AlgorithmImpl::init_program(const R1csFile& cs) {
    const size_t expect_in = cipher == CHACHA20 ? 1408 : cipher == AES_128 ? 157 : 173;
    if (cs.n_public - 1 + cs.n_secret != expect_in) throw std::runtime_error("r1cs: witness size does not match the cipher's circuit");
    return build_tables(cs, stream);
}

// The small-integer witness program (wit_small.hpp) from the calibration classes, when the circuit qualifies (solver_tables.hip)
void AlgorithmImpl::init_small(const SolverProgram& sp) {
    if (!cfg.small_witness) return;
    std::vector<uint8_t> ca = row_class_a, cb = row_class_b, cc = row_class_c;
    if (cfg.small_witness == 2) { std::fill(ca.begin(), ca.end(), 0); std::fill(cb.begin(), cb.end(), 0); std::fill(cc.begin(), cc.end(), 0); }      // test: wrong on purpose
    build_small_tables(sp, row_class, ca, cb, cc, stream);
    if (cfg.trace_host) fprintf(stderr, "InitAlgorithm(%d): small-integer witness path: %s%s\n", (int)cipher, small.ok ? "yes" : "no — ", small.ok ? "" : small.why.c_str());
}

void AlgorithmImpl::pack_inputs(const ProofRequest* reqs, size_t n, size_t B, uint8_t* h_in, uint8_t* h_rs) {
    memset(h_in, 0, 176 * B); memset(h_rs, 0, 64 * B);
    for (size_t i = 0; i < B; i++) {
        const ProofRequest& q = reqs[i < n ? i : n - 1];
        uint8_t* rec = h_in + 176 * i;
        memcpy(rec, q.key, q.keylen);
        memcpy(rec + 32, q.nonce, 12);
        rec[44] = (uint8_t)q.counter; rec[45] = (uint8_t)(q.counter >> 8); rec[46] = (uint8_t)(q.counter >> 16); rec[47] = (uint8_t)(q.counter >> 24);
        memcpy(rec + 48, q.plaintext, 64); memcpy(rec + 112, q.ciphertext, 64);
        memcpy(h_rs + 64 * i, q.r, 32); memcpy(h_rs + 64 * i + 32, q.s, 32);
    }
}

void AlgorithmImpl::calibrate() {
    row_class.assign(n_wires + 4, 255);
    row_class[n_wires] = row_class[n_wires + 1] = row_class[n_wires + 2] = 254;     // r, s, -rs: uniform scalars
    row_class_c.assign(n_constraints, 255);                                         // the rows of c (evaluation-form quotient): same prediction, same fallbacks
    row_class_a.assign(n_constraints, 255); row_class_b.assign(n_constraints, 255);  // the rows of a and b (byte planes of the small-integer witness path)
    if (cfg.bit_groups <= 0) return;
    if (cfg.bit_groups >= 2) { std::fill(row_class.begin(), row_class.begin() + n_wires, 0); std::fill(row_class_c.begin(), row_class_c.end(), 0); std::fill(row_class_a.begin(), row_class_a.end(), 0); std::fill(row_class_b.begin(), row_class_b.end(), 0); return; }
    const size_t B = 64;
    std::vector<ProofRequest> reqs(B);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (auto& q : reqs) {
        q = ProofRequest{};
        q.keylen = cipher == AES_128 ? 16 : 32;
        for (uint32_t i = 0; i < q.keylen; i++) q.key[i] = (uint8_t)next();
        for (auto& b : q.nonce) b = (uint8_t)next();
        for (auto& b : q.plaintext) b = (uint8_t)next();
        q.counter = (uint32_t)(next() & 0xFFFF);
        if (cipher == CHACHA20) chacha20_xor_stream(q.key, q.nonce, q.counter, q.plaintext, q.ciphertext, 64);
        else aes_ctr_xor_stream(q.key, q.keylen, q.nonce, q.counter, q.plaintext, q.ciphertext, 64);
        q.r[0] = 3; q.s[0] = 5; q.mask[0] = 7;
    }
    std::vector<uint8_t> h_in(176 * B), h_rs(64 * B); pack_inputs(reqs.data(), B, B, h_in.data(), h_rs.data());
    // (the calibration witness is a made-up key, but its buffers are cleared before they are freed like any call's)
    DevBuf<uint8_t> d_inputs(h_in.size(), true), d_rs(h_rs.size(), true), d_mask_in(32 * B, true); DevBuf<uint32_t> d_status(B);
    DevBuf<fe> d_W((n_wires + 4) * B, true), d_A(n_constraints * B, true), d_B(n_constraints * B, true), d_C(n_constraints * B, true), d_mask(B, true), d_commit(B, true);
    d_inputs.upload(h_in.data(), h_in.size(), stream); d_rs.upload(h_rs.data(), h_rs.size(), stream);
    if (cipher == CHACHA20) launch_assign_chacha(d_inputs.p, d_W.p, B, stream);
    else launch_assign_aes(d_inputs.p, cipher == AES_128 ? 16 : 32, d_W.p, B, stream);
    HIP_CHECK(hipMemsetAsync(d_mask_in.p, 1, d_mask_in.bytes(), stream));
    HIP_CHECK(hipMemsetAsync(d_commit.p, 1, d_commit.bytes(), stream));      // stands in for the commitment challenge: any residue will do
    launch_prep_rs(d_rs.p, d_W.p, n_wires, B, has_commitment ? d_mask_in.p : nullptr, d_mask.p, stream);
    HIP_CHECK(hipMemsetAsync(d_status.p, 0xFF, B * 4, stream));
    SolverArgs sa{prog.p, sched.p, 0, n_levels, coeff.p, coeff_inv.p, lookup_coeff.p, d_W.p, d_A.p, d_B.p, d_C.p, B, d_status.p,
                  has_commitment ? d_mask.p : nullptr, has_commitment ? d_commit.p : nullptr, has_div, 0u, nullptr};
    { SolverWalk walk; walk.n = B; solver_run_levels(*this, sa, walk, 0, n_levels, stream); }      // one launch per level
    DevBuf<uint8_t> d_cls(n_wires);
    launch_classify_wires(d_W.p, n_wires, B, d_status.p, d_cls.p, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(row_class.data(), d_cls.p, n_wires, hipMemcpyDeviceToHost, stream));
    DevBuf<uint8_t> d_cls_c(n_constraints);
    launch_classify_wires(d_C.p, n_constraints, B, d_status.p, d_cls_c.p, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(row_class_c.data(), d_cls_c.p, n_constraints, hipMemcpyDeviceToHost, stream));
    DevBuf<uint8_t> d_cls_a(n_constraints), d_cls_b(n_constraints);
    launch_classify_wires(d_A.p, n_constraints, B, d_status.p, d_cls_a.p, stream);
    launch_classify_wires(d_B.p, n_constraints, B, d_status.p, d_cls_b.p, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(row_class_a.data(), d_cls_a.p, n_constraints, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(row_class_b.data(), d_cls_b.p, n_constraints, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

namespace {
template <class AffT, size_t STRIDE, class Compressed, class Raw, class After>
std::vector<uint8_t> decode_points(const KeyPoints& pts, AffT* out, hipStream_t stream, Compressed compressed, Raw raw, After after) {
    const size_t n = pts.x.size() / STRIDE; std::vector<uint8_t> st(n);
    if (!n) return st;
    if (!pts.y.empty() && pts.y.size() != pts.x.size()) throw std::runtime_error("key points: the y bytes do not match the x bytes");
    DevBuf<uint8_t> d_x(pts.x.size()), d_y(pts.y.size()), d_st(n);
    d_x.upload(pts.x.data(), pts.x.size(), stream);
    compressed(d_x.p, out, d_st.p, n, stream);
    if (!pts.y.empty()) {      // raw elements (flag bits 00) take their Y from the companion bytes; the compressed ones keep what they have
        d_y.upload(pts.y.data(), pts.y.size(), stream);
        raw(d_x.p, d_y.p, out, d_st.p, n, stream);
    }
    after(out, d_st.p, n, stream);      // G2: the subgroup test over what decoded
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(st.data(), d_st.p, n, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    return st;
}
}  // namespace

std::vector<uint8_t> decode_g1_points(const KeyPoints& pts, G1Aff* out, hipStream_t stream) {
    return decode_points<G1Aff, 32>(pts, out, stream, launch_decompress_g1, launch_decode_raw_g1, [](G1Aff*, uint8_t*, size_t, hipStream_t) {});
}
std::vector<uint8_t> decode_g2_points(const KeyPoints& pts, G2Aff* out, hipStream_t stream) {
    return decode_points<G2Aff, 64>(pts, out, stream, launch_decompress_g2, launch_decode_raw_g2, launch_g2_subgroup);
}

template <class AffT, class XyzzT, class Decomp>
void AlgorithmImpl::build_set(MsmSet<AffT>& set, const KeyPoints& raw, size_t point_bytes, const std::vector<uint32_t>& rows, int c, const char* what, Decomp decomp, bool uniform, int expand_cv,
                              const std::vector<uint8_t>* classes, uint32_t zero_row, bool latency_layout) {
    const std::vector<uint8_t>& cls = classes ? *classes : row_class;
    const size_t n = raw.x.size() / point_bytes;
    if (rows.size() != n) throw std::runtime_error(std::string("pk: row map size mismatch for ") + what);
    set.nbases = n;
    DevBuf<AffT> bases(n ? n : 1);
    const std::vector<uint8_t> st = decomp(raw, bases.p);
    for (size_t i = 0; i < n; i++) if (st[i] == 1) throw std::runtime_error(std::string("pk: invalid point in ") + what);
    const uint32_t ROW_ZERO = zero_row != 0xFFFFFFFFu ? zero_row : (uint32_t)(n_wires + 3);
    // The layout (msm_layout.hpp); the point at infinity contributes nothing: dropped.
    // flat part: [bits][narrow][padding to an octet][window octets of the expanded wide wires]; expand_cv > 0: EVERY base becomes window octets of that
    // digit width (the latency-path layout of the quotient bases: no Horner pass)
    const MsmFlatPlan plan = msm_plan_flat(msm_sort_bases(st, rows, cls, uniform, cfg.bit_groups, cfg.row_margin_bits, NARROW_MAX_BITS), rows, ROW_ZERO, uniform, expand_cv, EXPAND_MAX, EXPAND_C, msm_windows);
    msm_build_tables<AffT, XyzzT>(set, bases.p, plan, rows, c, stream, &table_bytes);
    // the windowed part once more in the latency layout (the quotient bases have their own budgeted layout: init_key)
    if (set.nwide && !uniform && cfg.few_path && cfg.few_wide && latency_layout) {
        const std::vector<uint32_t>& wide = plan.wide;
        KeyPoints raw_w; raw_w.x.resize(set.nwide * point_bytes); if (!raw.y.empty()) raw_w.y.resize(set.nwide * point_bytes);
        std::vector<uint32_t> rows_w(set.nwide);
        for (size_t i = 0; i < set.nwide; i++) {
            memcpy(raw_w.x.data() + i * point_bytes, raw.x.data() + (size_t)wide[i] * point_bytes, point_bytes); rows_w[i] = rows[wide[i]];
            if (!raw.y.empty()) memcpy(raw_w.y.data() + i * point_bytes, raw.y.data() + (size_t)wide[i] * point_bytes, point_bytes);
        }
        set.few_wide.reset(new MsmSet<AffT>());
        build_set<AffT, XyzzT>(*set.few_wide, raw_w, point_bytes, rows_w, c, what, decomp, true, 8, classes, zero_row);
    }
}

// The fold (k_quot_bases.hip): U' and V' from U and V by three group transforms (launch_quot_fold_dft) — 3 n points and the weights as scratch.
bool AlgorithmImpl::fold_quotient_bases(const DevBuf<G1Aff>& d_U, const std::vector<uint8_t>& stU, const DevBuf<G1Aff>& d_V, const std::vector<uint8_t>& stV, const std::vector<uint32_t>& rowsZ,
                                        DevBuf<G1Aff>& d_U2, std::vector<uint8_t>& stU2, DevBuf<G1Aff>& d_V2, std::vector<uint8_t>& stV2) {
    const size_t m = n_constraints;
    DevBuf<uint32_t> d_perm(domain_n); d_perm.upload(rowsZ.data(), domain_n, stream);
    DevBuf<uint8_t> d_stU(m), d_stV(domain_n), d_stU2(m), d_stV2(m - 1), scratch(quot_fold_dft_scratch_bytes(L, (uint32_t)m));
    d_stU.upload(stU.data(), m, stream); d_stV.upload(stV.data(), domain_n, stream);
    d_U2.alloc(m); d_V2.alloc(m - 1); stU2.resize(m); stV2.resize(m - 1);
    hipEvent_t ev[3]; for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
    struct Free { hipEvent_t* e; ~Free() { for (int i = 0; i < 3; i++) (void)hipEventDestroy(e[i]); } } free_ev{ev};
    HIP_CHECK(hipEventRecord(ev[0], stream));
    launch_quot_fold_dft(L, (uint32_t)m, d_perm.p, d_U.p, d_stU.p, d_V.p, d_stV.p, d_U2.p, d_stU2.p, d_V2.p, d_stV2.p, scratch.p, stream, ev[1]);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev[2], stream));
    HIP_CHECK(hipMemcpyAsync(stU2.data(), d_stU2.p, m, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(stV2.data(), d_stV2.p, m - 1, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (cfg.trace_host) {
        float w = 0, t = 0; HIP_CHECK(hipEventElapsedTime(&w, ev[0], ev[1])); HIP_CHECK(hipEventElapsedTime(&t, ev[1], ev[2]));
        fprintf(stderr, "  tables G1.Z fold (dft): weights %.0f ms, transforms %.0f ms\n", w, t);
    }
    if (std::count(stV2.begin(), stV2.end(), (uint8_t)0) != (ptrdiff_t)(m - 1)) { fold_why = "a folded V base is the point at infinity"; return false; }
    fold_why.clear();
    return true;
}

void AlgorithmImpl::init_key(const R1csFile& cs, const PkFile& key) {
    if (key.n_wires != n_wires) throw std::runtime_error("pk: wire count does not match the r1cs");
    domain_n = key.domain_n; L = 0; while (((size_t)1 << L) < domain_n) L++;
    if (domain_n < n_constraints || domain_n != (size_t)1 << L) throw std::runtime_error("pk: domain too small for the constraint system");
    if (L < NTT_MIN_LOG2 || L > NTT_MAX_LOG2) throw std::runtime_error("pk: unsupported domain size 2^" + std::to_string(L) + " (the quotient kernels cover 2^15 .. 2^17: ChaCha20-V3 and AES-V2)");
    if (cs.has_commitment != key.has_commitment_key) throw std::runtime_error("pk: commitment keys do not match the r1cs");
    // NTT constants
    {
        uint8_t be[5 * 32];
        memcpy(be, key.omega, 32); memcpy(be + 32, key.omega_inv, 32); memcpy(be + 64, key.coset_g, 32); memcpy(be + 96, key.coset_g_inv, 32); memcpy(be + 128, key.n_inv, 32);
        DevBuf<uint8_t> d_be(sizeof be); d_be.upload(be, sizeof be, stream);
        dom.alloc(6);
        launch_fr_from_be(d_be.p, dom.p, 5, stream);
        tw_fwd.alloc(domain_n / 2 * 12); tw_inv.alloc(domain_n / 2 * 12); scale_mid.alloc(domain_n); scale_mid_plain.alloc(domain_n); tw_inv_plain.alloc(domain_n / 2 * 12); scale_out.alloc(domain_n); qr.alloc((2 * NTT_QMAX + 1) * 12);
        DevBuf<uint32_t> d_flag(1); uint32_t flag = 0;
        HIP_CHECK(hipMemsetAsync(d_flag.p, 0, 4, stream));
        launch_ntt_constants(dom.p, dom.p + 1, dom.p + 4, L, tw_fwd.p, tw_inv.p, scale_mid.p, scale_out.p, dom.p + 5, qr.p, d_flag.p, tw_inv_plain.p, scale_mid_plain.p, stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        if (flag) throw std::runtime_error("pk: the domain generator is not gnark-crypto's root of unity for this size");
    }
    // a slice and single points behind it as one set; the y bytes follow along when any part has raw elements (zeros for the parts that have none)
    auto cat = [](KeyPoints a, std::initializer_list<KeyPoints> more) {
        bool any_y = !a.y.empty();
        for (auto& m : more) any_y = any_y || !m.y.empty();
        if (any_y) a.y.resize(a.x.size(), 0);
        for (auto& m : more) {
            a.x.insert(a.x.end(), m.x.begin(), m.x.end());
            if (any_y) { a.y.insert(a.y.end(), m.y.begin(), m.y.end()); a.y.resize(a.x.size(), 0); }
        }
        return a;
    };
    const uint32_t ROW_ONE = 0, ROW_R = (uint32_t)n_wires, ROW_S = ROW_R + 1, ROW_NRS = ROW_R + 2;
    std::vector<uint32_t> rowsA, rowsB, rowsK;
    for (size_t i = 0; i < n_wires; i++) { if (!key.inf_A[i]) rowsA.push_back((uint32_t)i); if (!key.inf_B[i]) rowsB.push_back((uint32_t)i); }
    {
        std::vector<uint8_t> skip(n_wires, 0);
        if (cs.has_commitment) { for (uint32_t w : cs.commit_private) skip[w] = 1; skip[cs.commit_wire] = 1; }
        for (size_t i = cs.n_public; i < n_wires; i++) if (!skip[i]) rowsK.push_back((uint32_t)i);
        if (rowsK.size() * 32 != key.g1_K.size()) throw std::runtime_error("pk: G1.K size does not match the private wires");
    }
    rowsA.push_back(ROW_ONE); rowsA.push_back(ROW_R);
    std::vector<uint32_t> rowsB2 = rowsB;
    rowsB.push_back(ROW_ONE); rowsB.push_back(ROW_S); rowsB2.push_back(ROW_ONE); rowsB2.push_back(ROW_S);
    rowsK.push_back(ROW_NRS);
    quotient_eval = cfg.quotient_eval != 0;
    // coefficient form: the n - 1 bases of the key, scalars h; evaluation form: the n bases V_i, scalars d (k_quot_bases.hip)
    // (evaluation form: table position t holds V of index quot_digit_index(L, t), the order in which the last quotient kernel's threads hold d)
    std::vector<uint32_t> rowsZ(quotient_eval ? domain_n : domain_n - 1); for (size_t i = 0; i < rowsZ.size(); i++) rowsZ[i] = quotient_eval ? quot_digit_index(L, (uint32_t)i) : (uint32_t)i;
    std::vector<uint32_t> rowsZkey(domain_n - 1); for (size_t i = 0; i < rowsZkey.size(); i++) rowsZkey[i] = (uint32_t)i;
    std::vector<uint32_t> rowsC; if (quotient_eval) { rowsC.resize(n_constraints); for (size_t i = 0; i < n_constraints; i++) rowsC[i] = (uint32_t)i; }
    // Digit widths: explicit (GSC_WINDOW_Z / GSC_WINDOW_W) or the largest that keeps the tables inside the per-algorithm HBM
    // budget (the defaults leave room for all three algorithms of the reference on one 288 GB device: 3 x (48 + 16) GB).
    // Z: uniform rows of 2^(c-1) entries of 64 B: c = 16 is 69 GB for ChaCha20-V3 (2^15 - 1 bases), c = 14 is 69 GB for AES-V2 (2^17 - 1)
    if (!cfg.window_z) {
        // ... and inside what the device has free right now: the budget is an upper bound, not a promise (another tenant of the device, a host that
        // loads several algorithms).  Left out of the Z rows: the batch buffers of the lanes (~ 5.7 KiB per wire-or-domain row and proof, see
        // alloc_lane), the other sets' tables and the latency layouts (their own budgets), and 8 GiB of slack.
        double budget = cfg.z_table_gb * 1e9;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double nlanes = cfg.lanes > 0 ? cfg.lanes : (cs.has_commitment ? 2 : 1);
            const double lane = nlanes * (double)cfg.max_batch * ((double)n_wires * 32 + 3.0 * (double)domain_n * 32 + (double)domain_n * 2 * 20 + 1e5) * 1.15;
            const double others = (cfg.w_table_gb + (cfg.few_path ? cfg.few_z_gb + (cs.has_commitment ? 8 : 0) : 0)) * 1e9 + 8.0 * 1073741824.0;
            // (a replacement: what the outgoing engine holds on this device counts as free — the widths of a fresh InitAlgorithm once it is gone;
            // whether both fit side by side until then is for the allocations below to find out)
            const double room = (double)free_b + (double)cfg.reclaim_bytes - lane - others;
            if (room < budget) budget = room > 0 ? room : 0;
        }
        cfg.window_z = 4;
        for (int c = MSM_MAX_WINDOW; c >= 4; c--) if ((double)rowsZ.size() * (double)((size_t)1 << (c - 1)) * 64.0 <= budget) { cfg.window_z = c; break; }
    }
    if (!cfg.window_w) {      // wire sets: only the wide wires that get the windowed kernel (more than EXPAND_MAX per set) pay for c
        auto wide_in = [&](const std::vector<uint32_t>& rows, const std::vector<uint8_t>& cls) {
            size_t k = 0;
            for (uint32_t r : rows) { const int cl = r < cls.size() ? cls[r] : 255; if (cfg.bit_groups <= 0 || cl == 255 || cl + cfg.row_margin_bits > NARROW_MAX_BITS) k++; }
            return k > EXPAND_MAX ? (double)k : 0.0;
        };
        auto wide_of = [&](const std::vector<uint32_t>& rows) { return wide_in(rows, row_class); };
        const double g1 = wide_of(rowsA) + wide_of(rowsB) + wide_of(rowsK) + 2 * wide_of(cs.commit_private) + wide_in(rowsC, row_class_c), g2 = wide_of(rowsB2);
        cfg.window_w = 4;
        for (int c = 16; c >= 4; c--) if ((g1 * 64.0 + g2 * 128.0) * (double)((size_t)1 << (c - 1)) <= cfg.w_table_gb * 1e9) { cfg.window_w = c; break; }
    }
    auto dec1 = [this](const KeyPoints& raw, G1Aff* out) { return decompress_g1(raw, out); };
    auto dec2 = [this](const KeyPoints& raw, G2Aff* out) { return decompress_g2(raw, out); };
    const bool trace = cfg.trace_host;
    auto timed = [&](const char* what, auto&& fn) {
        const auto a0 = std::chrono::steady_clock::now(); const size_t b0 = table_bytes; fn();
        if (trace) fprintf(stderr, "  tables %-8s %7.0f ms %8.2f GiB\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a0).count(), (table_bytes - b0) / 1073741824.0);
    };
    timed("G1.A", [&] { build_set<G1Aff, G1Xyzz>(mA, cat({key.g1_A, key.g1_A_y}, {{key.g1_alpha, key.g1_alpha_y}, {key.g1_delta, key.g1_delta_y}}), 32, rowsA, cfg.window_w, "G1.A", dec1, false); });
    timed("G1.B", [&] { build_set<G1Aff, G1Xyzz>(mB1, cat({key.g1_B, key.g1_B_y}, {{key.g1_beta, key.g1_beta_y}, {key.g1_delta, key.g1_delta_y}}), 32, rowsB, cfg.window_w, "G1.B", dec1, false); });
    timed("G1.K", [&] { build_set<G1Aff, G1Xyzz>(mK, cat({key.g1_K, key.g1_K_y}, {{key.g1_delta, key.g1_delta_y}}), 32, rowsK, cfg.window_w, "G1.K", dec1, false); });
    if (!quotient_eval) timed("G1.Z", [&] { build_set<G1Aff, G1Xyzz>(mZ, KeyPoints(key.g1_Z, key.g1_Z_y), 32, rowsZ, cfg.window_z, "G1.Z", dec1, true); });      // uniform full-width scalars
    else {
        // The key's Z in evaluation form: U (scalars: the solver's c rows) and V (scalars: d on the zeta-coset), computed on the device from the
        // decompressed points; build_set then lays them out like any other set — "decompression" is a device copy of the finished bases.
        const size_t nz = key.g1_Z.size() / 32;
        if (nz + 1 != domain_n) throw std::runtime_error("pk: G1.Z does not hold n - 1 points");
        DevBuf<G1Aff> d_U(domain_n), d_V(domain_n); std::vector<uint8_t> stU(domain_n), stV(domain_n);
        timed("G1.Z -> U, V", [&] {
            DevBuf<G1Aff> zb(nz); const std::vector<uint8_t> st = decompress_g1(KeyPoints(key.g1_Z, key.g1_Z_y), zb.p);
            for (size_t i = 0; i < nz; i++) if (st[i] == 1) throw std::runtime_error("pk: invalid point in G1.Z");
            DevBuf<uint8_t> d_st(nz), d_stU(domain_n), d_stV(domain_n); d_st.upload(st.data(), nz, stream);
            DevBuf<fe> tw(domain_n / 2); DevBuf<G1Xyzz> scratch(domain_n); DevBuf<uint32_t> d_perm(domain_n);
            d_perm.upload(rowsZ.data(), domain_n, stream);
            launch_quot_bases(zb.p, d_st.p, L, 0, dom.p + 1, dom.p + 4, tw.p, scratch.p, nullptr, d_U.p, d_stU.p, stream);
            launch_quot_bases(zb.p, d_st.p, L, 1, dom.p + 1, dom.p + 4, tw.p, scratch.p, d_perm.p, d_V.p, d_stV.p, stream);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(stU.data(), d_stU.p, domain_n, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(stV.data(), d_stV.p, domain_n, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        });
        auto from_dev = [this](const DevBuf<G1Aff>& src, const std::vector<uint8_t>& st) {
            return [this, &src, &st](const KeyPoints& raw, G1Aff* out) {
                const size_t n = raw.x.size() / 32;
                HIP_CHECK(hipMemcpyAsync(out, src.p, n * sizeof(G1Aff), hipMemcpyDeviceToDevice, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
                return std::vector<uint8_t>(st.begin(), st.begin() + n);
            };
        };
        // The fold: positions m - 1 .. n - 1 of the table order leave the Z set, their bases go into U and into the live V (k_quot_bases.hip).
        // Gated on a key without points at infinity among V (positions must not shift) and on there being something to drop.
        DevBuf<G1Aff> d_U2, d_V2; std::vector<uint8_t> stU2, stV2;
        size_t live = domain_n;
        if (cfg.quotient_fold) {
            if (n_constraints < 2 || domain_n - n_constraints + 1 < domain_n / 64) fold_why = "nothing to drop";
            else if (std::count(stV.begin(), stV.end(), (uint8_t)0) != (ptrdiff_t)domain_n) fold_why = "a V base is the point at infinity";
            else timed("G1.Z fold", [&] { if (fold_quotient_bases(d_U, stU, d_V, stV, rowsZ, d_U2, stU2, d_V2, stV2)) live = n_constraints - 1; });
        }
        const bool folded = live != domain_n;
        const std::vector<uint8_t> rawV(live * 32, 0), rawU(n_constraints * 32, 0);      // build_set only takes the point count from these
        const std::vector<uint32_t> rowsV(rowsZ.begin(), rowsZ.begin() + live);
        timed("G1.Z (V)", [&] { build_set<G1Aff, G1Xyzz>(mZ, rawV, 32, rowsV, cfg.window_z, "G1.Z (evaluation form)", folded ? from_dev(d_V2, stV2) : from_dev(d_V, stV), true); });
        fuse_z_digits = mZ.nwide == live && cfg.fuse_z_digits != 0;      // (a V_i at infinity would be dropped from the table: positions would shift)
        if (folded) mZ.digit_bases = domain_n;      // the digit buffer keeps all n positions (the last quotient kernel's own indexing); the dropped ones are not read ...
        quot_live = folded && cfg.quotient_live_tiles ? live : 0;      // ... nor, with this, written: whole tiles of that kernel hold nothing else and are not run
        timed("G1.Z (U)", [&] { build_set<G1Aff, G1Xyzz>(mC, rawU, 32, rowsC, cfg.window_w, "G1.Z (evaluation form, c)", folded ? from_dev(d_U2, stU2) : from_dev(d_U, stU), false, 0, &row_class_c, (uint32_t)domain_n, false); });
    }
    if (cfg.few_path && cfg.few_z_gb > 0) {
        // calls with a handful of statements: the quotient bases once more as (base, window) pairs with their own rows 2^(cv j) d P — more
        // additions per proof than the wide rows above, but no 254-doubling Horner chain behind them (1.4 ms of a 6 ms Prove)
        const size_t nz = key.g1_Z.size() / 32;
        int cv = 0;
        for (int t : {8, 6, 4}) if ((double)nz * msm_windows(t) * (double)((size_t)1 << (t - 1)) * sizeof(G1Aff) <= (double)cfg.few_z_gb * 1e9) { cv = t; break; }
        if (cv) timed("G1.Z (latency layout)", [&] { build_set<G1Aff, G1Xyzz>(mZfew, KeyPoints(key.g1_Z, key.g1_Z_y), 32, rowsZkey, cfg.window_z, "G1.Z", dec1, true, cv); });
    }
    timed("G2.B", [&] { build_set<G2Aff, G2Xyzz>(mB2, cat({key.g2_B, key.g2_B_y}, {{key.g2_beta, key.g2_beta_y}, {key.g2_delta, key.g2_delta_y}}), 64, rowsB2, cfg.window_w, "G2.B", dec2, false); });
    if (cs.has_commitment) {
        if (cs.n_public_committed) throw std::runtime_error("r1cs: public committed wires are not supported");
        if (key.ped_basis.size() != cs.commit_private.size() * 32) throw std::runtime_error("pk: commitment basis size does not match the r1cs");
        build_set<G1Aff, G1Xyzz>(mPed, KeyPoints(key.ped_basis, key.ped_basis_y), 32, cs.commit_private, cfg.window_w, "commitment basis", dec1, false);
        build_set<G1Aff, G1Xyzz>(mPedSigma, KeyPoints(key.ped_basis_sigma, key.ped_basis_sigma_y), 32, cs.commit_private, cfg.window_w, "commitment basis (sigma)", dec1, false);
    }
}

void AlgorithmImpl::alloc_lane(Lane& ln, size_t B) {
    ln.cap = B;
    // every device allocation from here to the end of the function is counted (DevBuf::alloc) and must be in the region table at the end
    struct Tally { Tally(size_t* t) { devbuf_tally = t; } ~Tally() { devbuf_tally = nullptr; } } tally{&ln.allocated};
    // HIP spreads a process's streams over GPU_MAX_HW_QUEUES (4) hardware queues PER PRIORITY LEVEL, round-robin: with ten streams of one
    // priority (a full lane and two small ones, three streams each) a lane's side stream lands in the queue of another lane's main stream and
    // that lane's kernels wait behind a 3 ms chain of sixteen waves.  The three roles therefore take the three priority levels — three pools
    // of queues, no sharing with the default lane counts — and the levels suit them: the side stream carries thin chains on a call's
    // critical path (scalar multiplications, G2 Horner), the third stream bulk work that only has to finish before the Z sum (the quotient
    // of a big call) or beside an otherwise idle chip (a single Prove's B2 sum).  Measured against GPU_MAX_HW_QUEUES=8 in
    // profiles/r04l_hw_queues.txt.  GSC_STREAM_PRIORITIES=0: plain streams.
    int least = 0, greatest = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (cfg.stream_priorities && least != greatest) {
        const int code = cfg.stream_priorities == 1 ? 213 : cfg.stream_priorities;      // digits: main, side, third; 1 high, 2 normal, 3 low
        auto level = [&](int d) { return d == 1 ? greatest : d == 3 ? least : (least + greatest) / 2; };
        ln.kind[0] = level(code / 100); ln.kind[1] = level(code / 10 % 10); ln.kind[2] = level(code % 10);
    }
    ln.device = cfg.device; ln.index = (int)lanes.size() - 1;      // (the lane is the last of `lanes`: AlgorithmImpl's constructor)
    ln.stream = stream_take(ln.device, ln.kind[0], 3 * ln.index); ln.side = stream_take(ln.device, ln.kind[1], 3 * ln.index + 1); ln.side2 = stream_take(ln.device, ln.kind[2], 3 * ln.index + 2);
    for (auto& e : ln.ev) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventCreate(&ln.ev_ws));
    HIP_CHECK(hipEventCreateWithFlags(&ln.ev_wa, hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&ln.ev_wa_done, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ln.ev_few, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ln.ev_ab, hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&ln.ev_fs, hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&ln.ev_b2, hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&ln.ev_s2, hipEventDisableTiming));
    ln.h_in.alloc(176 * B); ln.h_rs.alloc(64 * B); ln.h_glv.alloc(2 * MSM_FEW_PROOFS); ln.h_out.alloc(256 * B); ln.h_flags.alloc((B + 3) / 4 * 4); ln.h_status.alloc(B); ln.h_words.alloc(56);
    ln.d_clk.alloc(48); HIP_CHECK(hipMemsetAsync(ln.d_clk.p, 0, 48 * 8, ln.stream));      // [0, 32): the Z kernel's eight samples; [32, 44): the three transform kernels
    ln.d_inputs.alloc(176 * B); ln.d_rs.alloc(64 * B); ln.d_out.alloc(256 * B); ln.d_flags.alloc((B + 3) / 4 * 4); ln.d_status.alloc(B); ln.d_fsync.alloc(2); ln.d_glv.alloc(2 * MSM_FEW_PROOFS);
    // (every buffer that will hold key-derived values starts out at its idle image — the wipe at the end of this function — so that "nothing of a call
    // is left" can be checked from the first call on)
    HIP_CHECK(hipMemsetAsync(ln.d_out.p, 0, ln.d_out.bytes(), ln.stream)); HIP_CHECK(hipMemsetAsync(ln.d_flags.p, 0, ln.d_flags.bytes(), ln.stream));
    HIP_CHECK(hipMemsetAsync(ln.d_status.p, 0, ln.d_status.bytes(), ln.stream)); HIP_CHECK(hipMemsetAsync(ln.d_fsync.p, 0, ln.d_fsync.bytes(), ln.stream));
    ln.d_W.alloc((n_wires + 4) * B); ln.d_A.alloc(domain_n * B); ln.d_B.alloc(domain_n * B); ln.d_C.alloc((domain_n + 1) * B);      // (+ one row that stays zero: the padding slots of mC)
    // calls with a handful of statements (k_solver_few) write their own columns only: the others must always hold field elements
    // (zero: every call leaves them so) because the transforms and MSMs run over whole 64-column batches
    if (small.ok) {      // byte planes of the small-integer witness path (values 0, 1, 0xFF)
        ln.d_W8.alloc((size_t)small.rows_per_group * B); ln.d_A8.alloc(n_constraints * B); ln.d_B8.alloc(n_constraints * B); ln.d_C8.alloc(n_constraints * B); ln.d_wsflag.alloc(1);
        HIP_CHECK(hipMemsetAsync(ln.d_wsflag.p, 0, 4, ln.stream));
        // rows predicted wide: their plane entries say "see the 32-byte element" for good (the rows kernel never writes them): the planes' idle image,
        // restored by every wipe of a plane (k_wipe's plane image writes the same marks by the same row classes)
        launch_wit_mark_wide(ln.d_A8.p, n_constraints, n_constraints, ws_cls_a.p, B, ln.stream); launch_wit_mark_wide(ln.d_B8.p, n_constraints, n_constraints, ws_cls_b.p, B, ln.stream);
        launch_wit_mark_wide(ln.d_C8.p, n_constraints, n_constraints, ws_cls_c.p, B, ln.stream);
        HIP_CHECK(hipGetLastError());
    }
    // partial-sum / digit buffers: the largest need over every batch size this context can be asked for
    size_t p1 = 0, p1b = 0, p2 = 0, p2b = 0, dg = 0, dgz = 0, sj2 = 0, gk = 0; size_t sj1[Lane::NSETS] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto need = [&](auto& m, size_t b, size_t& pa, size_t& pb, size_t& sj) {      // a batch call of b columns; 64 columns: a latency call as well
        for (int latency = 0; latency <= (b == 64 ? 1 : 0); latency++) {
            const MsmGeometry g = msm_geometry(m.shape(), b, latency != 0, msm_opts);
            pa = std::max(pa, g.pa); pb = std::max(pb, g.pb); sj = std::max(sj, g.sj); dg = std::max(dg, g.digit_words); gk = std::max(gk, g.gok_bytes);
        }
    };
    MsmSet<G1Aff>* g1sets[Lane::NSETS] = {&mA, &mB1, &mK, &mZ, &mPed, &mPedSigma, &mZfew, &mC};
    ln.need_at.clear();
    for (size_t b = 64; b <= B; b += 64) {
        for (int k = 0; k < Lane::NSETS; k++) if (g1sets[k] != &mZfew || b == 64) {      // the latency layout only serves 64-column batches
            if (fuse_z_digits && g1sets[k] == &mZ) { const size_t keep = dg; dg = 0; need(mZ, b, p1, p1b, sj1[k]); if (dg > dgz) dgz = dg; dg = keep; }      // Z's digits: a buffer of their own
            else need(*g1sets[k], b, p1, p1b, sj1[k]);
        }
        need(mB2, b, p2, p2b, sj2);
        // the needs up to this batch size: what a chunk of b columns can have written (the wipe's extents, wipe_plan.hpp)
        Lane::ScratchNeed nd;
        nd.part1a = p1 * sizeof(G1Xyzz); nd.part1b = p1b * sizeof(G1Xyzz); nd.part2a = p2 * sizeof(G2Xyzz); nd.part2b = p2b * sizeof(G2Xyzz);
        nd.digits = (fuse_z_digits ? dgz : dg) * sizeof(uint4); nd.digits_w = fuse_z_digits ? (dg ? dg : 1) * sizeof(uint4) : 0; nd.gok = gk ? gk : 1; nd.sj2 = (sj2 ? sj2 : 1) * sizeof(G2Xyzz);
        for (int k = 0; k < Lane::NSETS; k++) nd.sj1[k] = (sj1[k] ? sj1[k] : 1) * sizeof(G1Xyzz);
        ln.need_at.push_back(nd);
    }
    if (fuse_z_digits) { ln.d_digits_w.alloc(dg ? dg : 1); dg = dgz; }
    ln.d_part1a.alloc(p1); ln.d_part1b.alloc(p1b); ln.d_part2a.alloc(p2); ln.d_part2b.alloc(p2b);
    ln.d_digits.alloc(dg); ln.d_gok.alloc(gk ? gk : 1);
    {
        size_t dgs = 1, gks = 1, ps = 1;
        for (const MsmSet<G1Aff>* m : {&mA, &mB1}) {
            const size_t noct = (m->nflat + 7) / 8, nsl = (noct + 63) / 64, noctw = m->few_wide ? (m->few_wide->nflat + 7) / 8 : 0, nslw = (noctw + 63) / 64;
            if (noct * 64 > dgs) dgs = noct * 64;
            if (noctw * 64 > dgs) dgs = noctw * 64;
            if (m->nbit / 8 * MSM_FEW_PROOFS > gks) gks = m->nbit / 8 * MSM_FEW_PROOFS;
            if ((nsl + nslw) * 64 > ps) ps = (nsl + nslw) * 64;
        }
        { const size_t o1 = (mB2.nflat + 7) / 8, o2 = mB2.few_wide ? (mB2.few_wide->nflat + 7) / 8 : 0; ln.d_digits_s2.alloc((o1 > o2 ? o1 : o2) * 64 + 1); }
        ln.d_gok_s2.alloc(mB2.nbit / 8 * MSM_FEW_PROOFS + 1);
        ln.d_digits_s.alloc(dgs); ln.d_gok_s.alloc(gks); ln.d_part1c.alloc(ps); ln.d_part1d.alloc((ps / 64 + MSM_REDUCE_FANIN - 1) / MSM_REDUCE_FANIN * 64 + 64);
    }
    for (int k = 0; k < Lane::NSETS; k++) { ln.d_sj1[k].alloc(sj1[k] ? sj1[k] : 1); ln.d_flat1[k].alloc(g1sets[k]->nflat && g1sets[k]->nwide ? B : 1); }
    ln.d_sj2.alloc(sj2 ? sj2 : 1); ln.d_flat2.alloc(B);
    ln.d_sumA.alloc(B); ln.d_sumB1.alloc(B); ln.d_sumK.alloc(B); ln.d_sumZ.alloc(B); ln.d_sumC.alloc(B); ln.d_sumB2.alloc(B); ln.d_tmp.alloc(2 * B);
    if (has_commitment) {
        ln.d_mask_in.alloc(32 * B); ln.d_mask.alloc(B); ln.d_commit.alloc(B); ln.d_cpts.alloc(128 * B); ln.d_sumD.alloc(B); ln.d_sumPok.alloc(B);
        ln.h_mask.alloc(32 * B); ln.h_cpts.alloc(128 * B);
        HIP_CHECK(hipMemsetAsync(ln.d_cpts.p, 0, ln.d_cpts.bytes(), ln.stream));
    }
    // The region table: every allocation above by name.  Public: results, verdicts, timing words (the closed list of wipe_plan.hpp); all else is secret.
    ln.regions.clear();
    ln.reg(WR_INPUTS, ln.d_inputs); ln.reg(WR_RS, ln.d_rs); ln.reg(WR_GLV, ln.d_glv); ln.reg(WR_MASK_IN, ln.d_mask_in); ln.reg(WR_MASK, ln.d_mask); ln.reg(WR_COMMIT, ln.d_commit);
    ln.reg(WR_SUM_D, ln.d_sumD); ln.reg(WR_SUM_POK, ln.d_sumPok);
    ln.reg(WR_W, ln.d_W); ln.reg(WR_A, ln.d_A); ln.reg(WR_B, ln.d_B); ln.reg(WR_C, ln.d_C); ln.reg(WR_W8, ln.d_W8); ln.reg(WR_A8, ln.d_A8); ln.reg(WR_B8, ln.d_B8); ln.reg(WR_C8, ln.d_C8);
    ln.reg(WR_PART1A, ln.d_part1a); ln.reg(WR_PART1B, ln.d_part1b); ln.reg(WR_PART2A, ln.d_part2a); ln.reg(WR_PART2B, ln.d_part2b); ln.reg(WR_PART1C, ln.d_part1c); ln.reg(WR_PART1D, ln.d_part1d);
    ln.reg(WR_DIGITS, ln.d_digits); ln.reg(WR_DIGITS_W, ln.d_digits_w); ln.reg(WR_DIGITS_S, ln.d_digits_s); ln.reg(WR_DIGITS_S2, ln.d_digits_s2);
    ln.reg(WR_GOK, ln.d_gok); ln.reg(WR_GOK_S, ln.d_gok_s); ln.reg(WR_GOK_S2, ln.d_gok_s2);
    for (int k = 0; k < Lane::NSETS; k++) { ln.reg(WR_SJ1 + k, ln.d_sj1[k]); ln.reg(WR_FLAT1 + k, ln.d_flat1[k]); }
    ln.reg(WR_SJ2, ln.d_sj2); ln.reg(WR_FLAT2, ln.d_flat2);
    ln.reg(WR_SUM_A, ln.d_sumA); ln.reg(WR_SUM_B1, ln.d_sumB1); ln.reg(WR_SUM_K, ln.d_sumK); ln.reg(WR_SUM_Z, ln.d_sumZ); ln.reg(WR_SUM_C, ln.d_sumC); ln.reg(WR_SUM_B2, ln.d_sumB2); ln.reg(WR_TMP, ln.d_tmp);
    ln.reg(WR_OUT, ln.d_out); ln.reg(WR_FLAGS, ln.d_flags); ln.reg(WR_STATUS, ln.d_status); ln.reg(WR_CPTS, ln.d_cpts); ln.reg(WR_CLK, ln.d_clk); ln.reg(WR_FSYNC, ln.d_fsync); ln.reg(WR_WSFLAG, ln.d_wsflag);
    wipe_whole(ln, ln.stream);      // every secret region to its idle image (the planes: the marks of the rows predicted wide)
    HIP_CHECK(hipStreamSynchronize(ln.stream));
}
}  // namespace gsc
