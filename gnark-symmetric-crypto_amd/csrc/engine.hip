// Engine front: configuration from the environment, the per-device replicas of an algorithm and the dispatch of calls over them.
// See engine.hpp for the reference interface this mirrors; engine_impl.hpp for the per-device engine.
#include "engine_impl.hpp"
#include "dispatch.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace gsc {

namespace {
int env_int(const char* name, int dflt) { const char* v = getenv(name); return v && *v ? atoi(v) : dflt; }
}  // namespace

bool test_hooks_enabled() {
    static const bool on = [] { const char* e = getenv("GSC_ENABLE_TEST_HOOKS"); return e && e[0] == '1' && e[1] == 0; }();
    return on;
}
namespace { const bool g_hooks_read_at_load = test_hooks_enabled(); }      // forces the evaluation when the library is loaded

EngineConfig config_from_env() {
    EngineConfig c;
    c.device = env_int("GSC_DEVICE", 0);
    if (const char* dv = getenv("GSC_DEVICES")) {      // "0,1,2,3": one engine replica per listed device, batches split over them
        for (const char* q = dv; *q;) { while (*q == ',' || *q == ' ') q++; if (!*q) break; char* end = nullptr; const long v = strtol(q, &end, 10); if (end == q) throw std::runtime_error("GSC_DEVICES: expected a comma-separated list of device ordinals"); c.devices.push_back((int)v); q = end; }
    }
    c.max_batch = (size_t)env_int("GSC_MAX_BATCH", 1024);
    c.lanes = env_int("GSC_LANES", 0);
    c.small_lanes = env_int("GSC_SMALL_LANES", -1);
    if (c.small_lanes > 8) throw std::runtime_error("GSC_SMALL_LANES must be at most 8");
    c.small_lane_cap = env_int("GSC_SMALL_LANE_CAP", 0);
    if (c.small_lane_cap < 0 || c.small_lane_cap % 64) throw std::runtime_error("GSC_SMALL_LANE_CAP must be a multiple of 64");
    // test-only knobs (no product setting, no profile uses a non-default value): honoured with the load-time test-hooks flag only
    const bool hooks = test_hooks_enabled();
    c.min_split = (size_t)(hooks ? env_int("GSC_MIN_SPLIT", 0) : 0);
    c.bit_groups = env_int("GSC_BIT_GROUPS", 1);
    c.window_z = env_int("GSC_WINDOW_Z", 0);
    c.window_w = env_int("GSC_WINDOW_W", 0);
    c.z_table_gb = env_int("GSC_Z_TABLE_GB", 48);
    c.w_table_gb = env_int("GSC_W_TABLE_GB", 16);
    c.row_margin_bits = hooks ? env_int("GSC_ROW_MARGIN_BITS", 1) : 1;
    c.few_path = env_int("GSC_FEW_PATH", 1);
    c.few_solver = env_int("GSC_FEW_SOLVER", 1);
    c.few_max = env_int("GSC_FEW_MAX", 0);
    if (c.few_max < 0 || c.few_max > (int)MSM_FEW_PROOFS) throw std::runtime_error("GSC_FEW_MAX must be in [0, 32]");
    c.few_workgroups = hooks ? env_int("GSC_FEW_WGS", 0) : 0;
    c.few_z_gb = env_int("GSC_FEW_Z_GB", 12);
    c.few_wide = env_int("GSC_FEW_WIDE", 1);
    c.quotient_eval = env_int("GSC_QUOTIENT_EVAL", 1);
    c.fuse_z_digits = env_int("GSC_FUSE_Z_DIGITS", 1);
    c.quotient_fold = env_int("GSC_QUOTIENT_FOLD", 1);
    if (c.quotient_fold < 0 || c.quotient_fold > 2) throw std::runtime_error("GSC_QUOTIENT_FOLD must be 0, 1 or 2");
    c.quotient_live_tiles = env_int("GSC_QUOTIENT_LIVE_TILES", 1) ? 1 : 0;
    c.small_witness = env_int("GSC_SMALL_WITNESS", 1);
    c.small_witness_few = env_int("GSC_SMALL_WITNESS_FEW", 1);
    c.ntt_plain = env_int("GSC_NTT_PLAIN", 1) ? 1 : 0;
    c.overlap_quotient = env_int("GSC_OVERLAP_QUOTIENT", 1);
    if (c.overlap_quotient < 0 || c.overlap_quotient > 2) throw std::runtime_error("GSC_OVERLAP_QUOTIENT must be 0, 1 or 2");
    c.stream_priorities = env_int("GSC_STREAM_PRIORITIES", 1);      // 0 plain; 1 = main normal, side high, third low; 3-digit codes (test hook): one digit per stream, 1 high 2 normal 3 low
    if (c.stream_priorities != 0 && c.stream_priorities != 1 && !(hooks && c.stream_priorities >= 111 && c.stream_priorities <= 333)) throw std::runtime_error("GSC_STREAM_PRIORITIES must be 0 or 1");
    if (test_hooks_enabled()) { c.win_slice = env_int("GSC_WIN_SLICE", 256); if (c.win_slice < 64 || c.win_slice > 4096 || c.win_slice % 8) throw std::runtime_error("GSC_WIN_SLICE must be a multiple of 8 in [64, 4096]"); }
    if (c.small_witness < 0 || c.small_witness > 2 || (c.small_witness == 2 && !test_hooks_enabled())) throw std::runtime_error("GSC_SMALL_WITNESS must be 0 or 1");
    if (c.few_workgroups < 0 || c.few_workgroups > 256) throw std::runtime_error("GSC_FEW_WGS must be in [0, 256]");
    c.trace_host = getenv("GSC_TRACE_HOST") != nullptr;
    c.prove_check = env_int("GSC_PROVE_CHECK", 0) != 0;
    if (const char* d = getenv("GSC_VK_DIR")) c.vk_dir = d;
    if (test_hooks_enabled()) { c.solver_trace = getenv("GSC_SOLVER_TRACE") != nullptr; c.few_test_abort = getenv("GSC_FEW_TEST_ABORT") != nullptr; c.keep_secrets = getenv("GSC_KEEP_SECRETS") != nullptr; c.wipe_full = env_int("GSC_WIPE", 1) != 0; c.fail_after_stage = env_int("GSC_FAIL_AFTER_STAGE", 0); c.wipe_grid = env_int("GSC_WIPE_GRID", 0); if (c.wipe_grid < 0 || c.wipe_grid > 65536) throw std::runtime_error("GSC_WIPE_GRID must be in [0, 65536]"); c.z_exp_entry_bits = env_int("GSC_Z_EXP_ENTRY_BITS", 0); }
    if (c.max_batch < 64) c.max_batch = 64;
    c.max_batch = (c.max_batch + 63) / 64 * 64;
    if ((c.window_z && (c.window_z < 4 || c.window_z > MSM_MAX_WINDOW)) || (c.window_w && (c.window_w < 4 || c.window_w > 16))) throw std::runtime_error("GSC_WINDOW_Z must be in [4,17], GSC_WINDOW_W in [4,16]");
    return c;
}

void debug_field_ops(int device, int field, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int chain) {
    use_device(device);
    DevBuf<fe> da(n), db(n), dout(n);
    HIP_CHECK(hipMemcpy(da.p, a, 32 * n, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(db.p, b, 32 * n, hipMemcpyHostToDevice));
    if (!launch_field_ops(field, op, da.p, db.p, dout.p, n, chain, nullptr)) throw std::runtime_error("gsc_debug_field_ops: field " + std::to_string(field) + " has no op " + std::to_string(op));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dout.p, 32 * n, hipMemcpyDeviceToHost));
}

void debug_limb_ops(int device, int field, int op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* out, size_t n) {
    const int operands = op == 0 ? 2 : op == 2 ? 4 : 1;      // mul: a, b; fmms: a, b, c, d; sqr / norm / freeze / freeze_near: a
    const int32_t* src[4] = {a, b, c, d};
    for (int j = 0; j < operands; j++) if (!src[j]) throw std::runtime_error("gsc_debug_limb_ops: operand missing");
    use_device(device);
    DevBuf<int32_t> din[4], dout(9 * n);
    for (int j = 0; j < 4; j++) {      // an operand the op does not read is a copy of a
        din[j].alloc(9 * n);
        HIP_CHECK(hipMemcpy(din[j].p, j < operands ? src[j] : a, 36 * n, hipMemcpyHostToDevice));
    }
    if (!launch_limb_ops(field, op, din[0].p, din[1].p, din[2].p, din[3].p, dout.p, n, nullptr)) throw std::runtime_error("gsc_debug_limb_ops: field " + std::to_string(field) + " has no op " + std::to_string(op));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dout.p, 36 * n, hipMemcpyDeviceToHost));
}

void debug_curve_ops(int device, int group, int op, const uint8_t* pts, const uint8_t* inf, const uint8_t* lam, size_t n, size_t k, uint8_t* out, uint8_t* flags) {
    // dbl, to_aff: one point; add: two; the accumulations: at least two (madd) / one (partial sums)
    const bool k_ok = op == 0 || op == 4 ? k == 1 : op == 3 ? k == 2 : op == 5 ? k >= 1 : k >= 2;
    if (group < 0 || group > 1 || op < 0 || op > 5 || !k_ok || k > 4096 || n > (1u << 20)) throw std::runtime_error("gsc_debug_curve_ops: no such group / op / point count");
    // an AFFINE operand cannot be the point at infinity: every point of madd but the first, every point of the partial sums
    if (op == 1 || op == 2 || op == 5)
        for (size_t i = 0; i < n; i++) for (size_t j = op == 5 ? 0 : 1; j < k; j++) if (inf[k * i + j]) throw std::runtime_error("gsc_debug_curve_ops: infinity as an affine operand");
    use_device(device);
    const size_t w = group == 0 ? 1 : 2;      // 32-byte values per coordinate
    DevBuf<fe> dpts(2 * w * k * n), dlam(2 * w * n), dout(2 * w * n);
    DevBuf<uint8_t> dinf(k * n), dflags(n);
    HIP_CHECK(hipMemcpy(dpts.p, pts, 32 * 2 * w * k * n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dlam.p, lam, 32 * 2 * w * n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dinf.p, inf, k * n, hipMemcpyHostToDevice));
    if (!launch_curve_ops(group, op, k, dpts.p, dinf.p, dlam.p, dout.p, dflags.p, n, nullptr)) throw std::runtime_error("gsc_debug_curve_ops: no such group / op");
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dout.p, 32 * 2 * w * n, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(flags, dflags.p, n, hipMemcpyDeviceToHost));
}

void debug_decode_points(int device, int group, const uint8_t* bytes, size_t len, size_t n, uint8_t* out_xy, uint8_t* status) {
    if (group < 0 || group > 1 || n > (1u << 20)) throw std::runtime_error("gsc_debug_decode_points: no such group / too many points");
    const size_t cb = group == 0 ? 32 : 64, w = cb / 32;
    KeyPoints pts;
    const size_t used = walk_points(bytes, len, n, cb, pts.x, pts.y, "points");      // the walk parse_pk makes over every slice
    if (used != len) throw std::runtime_error("points: trailing bytes");
    if (!n) return;
    use_device(device);
    DevBuf<fe> dpts(2 * w * n), dcanon(2 * w * n);
    const std::vector<uint8_t> st = group == 0 ? decode_g1_points(pts, reinterpret_cast<G1Aff*>(dpts.p), nullptr) : decode_g2_points(pts, reinterpret_cast<G2Aff*>(dpts.p), nullptr);
    launch_fp_from_mont(dpts.p, dcanon.p, 2 * w * n, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<uint8_t> le(64 * w * n);
    HIP_CHECK(hipMemcpy(le.data(), dcanon.p, le.size(), hipMemcpyDeviceToHost));
    // device order: G1 x, y; G2 x.a0, x.a1, y.a0, y.a1 (little-endian limbs) -> X | Y big-endian, in G2 A1 before A0 as in the encodings
    for (size_t i = 0; i < n; i++) {
        status[i] = st[i];
        for (size_t c = 0; c < 2 * w; c++) {
            const size_t src = w == 1 ? c : (c ^ 1);
            const uint8_t* v = le.data() + 32 * (2 * w * i + src);
            uint8_t* o = out_xy + 32 * (2 * w * i + c);
            for (int k = 0; k < 32; k++) o[k] = st[i] == 0 ? v[31 - k] : 0;
        }
    }
}

bool debug_tower_ops(int device, int path, int op, const int32_t* in, size_t n, int32_t* out, uint8_t* flags) {
    int iw, ow;
    if (!tower_ops_words(path, op, &iw, &ow)) return false;
    if (n > (1u << 16)) throw std::runtime_error("gsc_debug_tower_ops: too many elements");
    if (!n) return true;
    use_device(device);
    DevBuf<int32_t> din((size_t)iw * n), dout((size_t)(ow ? ow : 1) * n);
    DevBuf<uint8_t> dflags(n);
    HIP_CHECK(hipMemcpy(din.p, in, 4 * (size_t)iw * n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dout.p, 0, 4 * (size_t)(ow ? ow : 1) * n));
    HIP_CHECK(hipMemset(dflags.p, 0, n));
    if (!launch_tower_ops(path, op, din.p, dout.p, dflags.p, n, nullptr)) return false;
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (ow) HIP_CHECK(hipMemcpy(out, dout.p, 4 * (size_t)ow * n, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(flags, dflags.p, n, hipMemcpyDeviceToHost));
    return true;
}

void debug_quot_fold_dft(int device, int L, uint32_t m, const uint32_t* perm, const uint8_t* u_be, const uint8_t* u_inf, const uint8_t* v_be, const uint8_t* v_inf,
                         uint8_t* u2_be, uint8_t* u2_inf, uint8_t* v2_be, uint8_t* v2_inf) {
    const size_t n = (size_t)1 << L;
    std::vector<uint32_t> pm(n);
    {      // position -> coset index: a permutation, or the kernels' scatter would leave slots unwritten (or land outside the array)
        std::vector<uint8_t> seen(n, 0);
        for (size_t i = 0; i < n; i++) { pm[i] = perm ? perm[i] : (uint32_t)i; if (pm[i] >= n || seen[pm[i]]++) throw std::runtime_error("gsc_debug_quot_fold_dft: perm is not a permutation of 0 .. n - 1"); }
    }
    use_device(device);
    DevBuf<uint32_t> d_perm(n);
    DevBuf<uint8_t> d_be((m + n) * 64), d_inf(m + n), d_stU(m), d_stV(n), d_stU2(m), d_stV2(m - 1), d_out((2 * (size_t)m - 1) * 64), d_flags(2 * (size_t)m - 1), scratch(quot_fold_dft_scratch_bytes(L, m));
    DevBuf<G1Aff> d_U(m), d_V(n), d_U2(m), d_V2(m - 1);
    HIP_CHECK(hipMemcpy(d_perm.p, pm.data(), 4 * n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_be.p, u_be, 64 * (size_t)m, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(d_be.p + 64 * (size_t)m, v_be, 64 * n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_inf.p, u_inf, m, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(d_inf.p + m, v_inf, n, hipMemcpyHostToDevice));
    launch_g1_aff_from_be(d_be.p, d_inf.p, m, d_U.p, d_stU.p, nullptr);
    launch_g1_aff_from_be(d_be.p + 64 * (size_t)m, d_inf.p + m, n, d_V.p, d_stV.p, nullptr);
    launch_quot_fold_dft(L, m, d_perm.p, d_U.p, d_stU.p, d_V.p, d_stV.p, d_U2.p, d_stU2.p, d_V2.p, d_stV2.p, scratch.p, nullptr);
    launch_g1_aff_to_be(d_U2.p, d_stU2.p, m, d_out.p, d_flags.p, nullptr);
    launch_g1_aff_to_be(d_V2.p, d_stV2.p, m - 1, d_out.p + 64 * (size_t)m, d_flags.p + m, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(u2_be, d_out.p, 64 * (size_t)m, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(u2_inf, d_flags.p, m, hipMemcpyDeviceToHost));
    if (m > 1) { HIP_CHECK(hipMemcpy(v2_be, d_out.p + 64 * (size_t)m, 64 * (size_t)(m - 1), hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(v2_inf, d_flags.p + m, m - 1, hipMemcpyDeviceToHost)); }
}

float debug_wipe(int device, uint64_t bytes, int fill, const uint64_t* desc, size_t ndesc, const uint8_t* cls, size_t ncls, uint8_t* out, const uint64_t* win, size_t nwin, uint64_t* counts) {
    use_device(device);
    if (!bytes || bytes > ((uint64_t)1 << 36)) throw std::runtime_error("gsc_debug_wipe: buffer size out of range");
    // every descriptor inside the buffer (no overflow: each factor is bounded first), image descriptors only with a class array
    auto checked = [&](const uint64_t* d, uint8_t* base, const uint8_t* d_cls) {
        const uint64_t off = d[0], rows = d[1], pitch = d[2], width = d[3];
        if (off > bytes || rows > bytes || pitch > bytes || width > bytes) throw std::runtime_error("gsc_debug_wipe: descriptor outside the buffer");
        if (rows && width) {
            if (rows > 1 && pitch < width) throw std::runtime_error("gsc_debug_wipe: rows overlap");
            const unsigned __int128 end = (unsigned __int128)off + (unsigned __int128)(rows - 1) * pitch + width;
            if (end > bytes) throw std::runtime_error("gsc_debug_wipe: descriptor outside the buffer");
        }
        if (d[4] && (!d_cls || !ncls)) throw std::runtime_error("gsc_debug_wipe: plane image without row classes");
        return WipeDesc{base + off, rows, pitch, width, d[4] ? d_cls : nullptr, d[4] ? (uint64_t)ncls : 0};
    };
    DevBuf<uint8_t> buf(bytes), d_cls(ncls ? ncls : 1); DevBuf<unsigned long long> d_cnt(nwin ? nwin : 1);
    if (ncls) HIP_CHECK(hipMemcpy(d_cls.p, cls, ncls, hipMemcpyHostToDevice));
    std::vector<WipeDesc> ds, ws;
    for (size_t i = 0; i < ndesc; i++) ds.push_back(checked(desc + 5 * i, buf.p, d_cls.p));
    for (size_t i = 0; i < nwin; i++) ws.push_back(checked(win + 5 * i, buf.p, d_cls.p));
    HIP_CHECK(hipMemset(buf.p, fill, bytes));
    HIP_CHECK(hipMemset(d_cnt.p, 0, d_cnt.bytes()));
    HIP_CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1; HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
    struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
    HIP_CHECK(hipEventRecord(e0, nullptr));
    launch_wipe(ds.data(), ds.size(), 0, nullptr);
    HIP_CHECK(hipEventRecord(e1, nullptr));
    for (size_t i = 0; i < nwin; i++) launch_scan_idle(ws[i], d_cnt.p + i, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (out) HIP_CHECK(hipMemcpy(out, buf.p, bytes, hipMemcpyDeviceToHost));
    if (nwin) { std::vector<unsigned long long> h(nwin); HIP_CHECK(hipMemcpy(h.data(), d_cnt.p, nwin * 8, hipMemcpyDeviceToHost)); for (size_t i = 0; i < nwin; i++) counts[i] = h[i]; }
    return ms;
}

void debug_clock_trace(int device, uint32_t n, uint32_t interval_us, unsigned long long* out) {
    HIP_CHECK(hipSetDevice(device));
    hipStream_t st; HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DevBuf<unsigned long long> d(2 * (size_t)n);
    launch_clock_trace(d.p, n, interval_us * 100u, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d.p, 16 * (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    HIP_CHECK(e);
}

// ---- Algorithm: one replica of the engine per device (GSC_DEVICES), batches split over the replicas ----
Algorithm::Algorithm(Cipher cipher, const uint8_t* pk, size_t pk_len, const uint8_t* r1cs, size_t r1cs_len, const EngineConfig& cfg) {
    std::vector<int> devs = cfg.devices.empty() ? std::vector<int>{cfg.device} : cfg.devices;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device available: the GPU prover has no CPU fallback");
    for (int d : devs) if (d < 0 || d >= ndev) throw std::runtime_error("GSC_DEVICES / GSC_DEVICE: device " + std::to_string(d) + " does not exist (" + std::to_string(ndev) + " visible)");
    impls_.resize(devs.size());
    // every replica decodes the key and builds its own tables on its device; the builds run side by side
    std::exception_ptr err; std::mutex err_mu; std::vector<std::thread> th;
    auto make = [&](size_t i) {
        try { EngineConfig c = cfg; c.device = devs[i]; c.reclaim_bytes = i < cfg.outgoing_bytes.size() ? cfg.outgoing_bytes[i] : 0; impls_[i].reset(new AlgorithmImpl(cipher, pk, pk_len, r1cs, r1cs_len, c)); }
        catch (...) { std::lock_guard<std::mutex> g(err_mu); if (!err) err = std::current_exception(); }
    };
    for (size_t i = 1; i < devs.size(); i++) th.emplace_back(make, i);
    make(0);
    for (auto& t : th) t.join();
    if (err) { impls_.clear(); std::rethrow_exception(err); }
    for (auto& i : impls_) i->corrupt = &corrupt_;
    picker_.reset(new ReplicaPicker(impls_.size()));
}
bool Algorithm::prove_check_init(const uint8_t* vk, size_t len) {
    // every replica's context first (its device, its largest lane), then all of them in: a refused key changes nothing
    std::vector<std::shared_ptr<ProveCheckCtx>> ctx;
    for (auto& i : impls_) {
        ctx.push_back(prove_check_create((int)i->cipher, vk, len, i->cfg.device, i->cap));
        if (!ctx.back()) return false;
    }
    for (size_t k = 0; k < impls_.size(); k++) { std::lock_guard<std::mutex> l(impls_[k]->check_mu); impls_[k]->check = ctx[k]; }
    return true;
}
void Algorithm::prove_check_off() { for (auto& i : impls_) { std::lock_guard<std::mutex> l(i->check_mu); i->check.reset(); } }
void Algorithm::prove_check_stats(uint64_t out[4]) const {
    for (int k = 0; k < 4; k++) out[k] = 0;
    for (auto& i : impls_) if (auto c = i->check_now()) prove_check_add_stats(*c, out);
}
bool Algorithm::debug_prove_corrupt(uint32_t index, int which, int mode) {
    if (which < 0 || which > 4 || mode < 0 || mode > 1 || (which > 2 && !impls_[0]->has_commitment)) return false;
    corrupt_.store((uint64_t)1 << 63 | (uint64_t)mode << 40 | (uint64_t)which << 32 | index);
    return true;
}
Algorithm::~Algorithm() = default;
Cipher Algorithm::cipher() const { return impls_[0]->cipher; }
size_t Algorithm::max_batch() const { size_t c = 0; for (auto& i : impls_) c += i->cap; return c; }
size_t Algorithm::devices() const { return impls_.size(); }
size_t Algorithm::lanes() const { return impls_[0]->lanes.size(); }      // full + small: device batches that can be in flight per device
namespace { thread_local KernelStat t_call_stat; thread_local const Algorithm* t_call_owner = nullptr; }
KernelStat Algorithm::last_kernel_stat() const {
    if (t_call_owner == this) return t_call_stat;      // this thread's own last call
    AlgorithmImpl* a = impls_[last_replica_.load() < impls_.size() ? last_replica_.load() : 0].get();
    std::lock_guard<std::mutex> lk(a->stat_mu);
    return a->last_stat;
}
std::string Algorithm::describe() const {
    const AlgorithmImpl* impl_ = impls_[0].get();
    char buf[640];
    snprintf(buf, sizeof buf, "wires=%zu constraints=%zu domain=2^%d max_batch=%zu lanes=%zu small=%zux%zu devices=%zu window_z=%d window_w=%d tables=%.2f GiB bases A=%zu B=%zu K=%zu Z=%zu grouped A=%zu B=%zu K=%zu wide(windowed+expanded) A=%zu+%zu B=%zu+%zu K=%zu+%zu",
             impl_->n_wires, impl_->n_constraints, impl_->L, max_batch(), impl_->full_lanes, impl_->lanes.size() - impl_->full_lanes, impl_->lanes.size() > impl_->full_lanes ? impl_->lanes.back()->cap : (size_t)0, impls_.size(), impl_->cfg.window_z, impl_->cfg.window_w, impl_->table_bytes / 1073741824.0,
             impl_->mA.nbases, impl_->mB1.nbases, impl_->mK.nbases, impl_->mZ.digit_bases ? impl_->mZ.digit_bases : impl_->mZ.nbases, impl_->mA.nbit, impl_->mB1.nbit, impl_->mK.nbit,
             impl_->mA.nwide, impl_->mA.nexpanded, impl_->mB1.nwide, impl_->mB1.nexpanded, impl_->mK.nwide, impl_->mK.nexpanded);
    // per replica: calls and statements it has served (ReplicaPicker): shows that small calls reach every device
    std::string out = buf;
    if (impl_->quotient_eval) out += std::string(" quotient=evaluation-form") + (impl_->fuse_z_digits ? "+digits" : "") + (!impl_->fuse_z_digits || !impl_->cfg.overlap_quotient ? "" : impl_->cfg.overlap_quotient == 2 ? "+beside-wire-sets" : "+beside-wire-sets(<4096)") + "(c: " + std::to_string(impl_->mC.nbit) + " grouped + " + std::to_string(impl_->mC.nflat - impl_->mC.nbit) + " flat + " + std::to_string(impl_->mC.nwide) + " windowed)";
    else out += " quotient=coefficient-form";
    if (impl_->quotient_eval) out += impl_->mZ.digit_bases ? " Zlive=" + std::to_string(impl_->mZ.nwide) + " Zfold=dft" :" Zfold=off(" + impl_->fold_why + ")";
    if (impl_->quotient_eval) out += " Qtiles=" + std::to_string(quot_live_tiles(impl_->L, impl_->quot_live)) + "/" + std::to_string(1u << (impl_->L - (impl_->L + 1) / 2));      // tiles the last quotient kernel runs
    out += impl_->small.ok ? " witness=small-integer(" + std::to_string(impl_->small.n_levels) + " chained levels, fallbacks " + std::to_string(impl_->small_fallbacks.load()) + ")" : " witness=generic" + (impl_->small.why.empty() ? std::string() : "(" + impl_->small.why + ")");
    out += impl_->cfg.keep_secrets ? " wipe=off" : impl_->cfg.wipe_full ? " wipe=full" : " wipe=inputs";
    {   // the self-check: off, or on with the device memory its contexts take (all replicas)
        size_t bytes = 0; bool on = false;
        for (auto& i : impls_) if (auto c = i->check_now()) { on = true; bytes += prove_check_device_bytes(*c); }
        out += on ? " check=on(" + std::to_string(bytes) + ")" : " check=off";
    }
    out += " served(calls/statements)=";
    const auto sv = picker_->served();
    for (size_t i = 0; i < sv.size(); i++) out += (i ? "," : "") + std::to_string(sv[i].calls) + "/" + std::to_string(sv[i].statements);
    return out;
}
size_t Algorithm::domain_size() const { return impls_[0]->domain_n; }
// The set-up the quotient test hooks share: `mats` matrices [m][64] of canonical big-endian values into A, B (, C) of the first lane,
// `quot(plan, lane, columns)` on them, A back to the host (out != nullptr).  The plan is the one stage_quotient builds (the plain-integer tables included:
// they are read only where a launch passes byte planes with NttNarrow::plain).  m_max: the rows a hook admits.
template <class Quot>
static void debug_quotient(AlgorithmImpl& a, const char* who, const uint8_t* mats_be, size_t mats, size_t m, size_t m_max, uint8_t* out, Quot quot) {
    if (m > m_max) throw std::runtime_error(std::string(who) + (m_max == a.n_constraints ? ": more rows than constraints" : ": more rows than the domain has"));
    HIP_CHECK(hipSetDevice(a.cfg.device));
    struct Hold { AlgorithmImpl& a; size_t i; ~Hold() { a.release_lane(i); } } hold{a, a.acquire_lane(0)};
    AlgorithmImpl::Lane& ln = *a.lanes[0];
    const size_t B = 64, cnt = m * B;
    DevBuf<uint8_t> d_be(mats * cnt * 32 + 32, true);
    d_be.upload(mats_be, mats * cnt * 32, ln.stream);
    fe* const dst[3] = {ln.d_A.p, ln.d_B.p, ln.d_C.p};
    for (size_t k = 0; k < mats; k++) launch_fr_from_be(d_be.p + k * cnt * 32, dst[k], cnt, ln.stream);
    NttPlan plan{a.L, a.tw_fwd.p, a.tw_inv.p, a.scale_mid.p, a.scale_out.p, a.dom.p + 5, a.qr.p, nullptr, a.tw_inv_plain.p, a.scale_mid_plain.p};
    HIP_CHECK(quot(plan, ln, B));
    if (out) HIP_CHECK(hipMemcpyAsync(out, ln.d_A.p, a.domain_n * B * 32, hipMemcpyDeviceToHost, ln.stream));
    if (!a.cfg.keep_secrets && a.cfg.wipe_full) a.wipe_whole(ln, ln.stream);      // the hook's vectors are a caller's data like any other
    HIP_CHECK(hipStreamSynchronize(ln.stream));
}
void Algorithm::debug_compute_h(const uint8_t* abc_be, size_t m, uint8_t* h_out) {
    debug_quotient(*impls_[0], "debug_compute_h", abc_be, 3, m, impls_[0]->n_constraints, h_out, [m](const NttPlan& plan, AlgorithmImpl::Lane& ln, size_t B) { return launch_compute_h(plan, ln.d_A.p, ln.d_B.p, ln.d_C.p, m, B, ln.stream); });
}
void Algorithm::debug_compute_d(const uint8_t* ab_be, size_t m, uint8_t* d_out) {
    debug_quotient(*impls_[0], "debug_compute_d", ab_be, 2, m, impls_[0]->n_constraints, d_out, [m](const NttPlan& plan, AlgorithmImpl::Lane& ln, size_t B) { return launch_compute_d(plan, ln.d_A.p, ln.d_B.p, m, B, ln.stream); });
}
size_t Algorithm::debug_quotient_routes_bytes(int c) const {
    const size_t n = impls_[0]->domain_n;
    return c ? (size_t)msm_windows(c) * (n / 8) * 64 * msm_digit_words(c) * sizeof(uint4) : n * 64 * sizeof(fe);
}
void Algorithm::debug_quotient_routes(const uint8_t* ab_be, size_t m, const int8_t* planes, int plain, size_t ncols, size_t live, int c, uint8_t* out, size_t cap) {
    AlgorithmImpl& a = *impls_[0];
    const size_t n = a.domain_n, B = 64;
    const auto refuse = [](const char* why) { throw std::runtime_error(std::string("gsc_debug_quotient: ") + why); };
    if (!ab_be || !out) refuse("a missing buffer");
    if (plain != 0 && plain != 1) refuse("plain is 0 or 1");
    if (c != 0 && (c < 4 || c > MSM_MAX_WINDOW)) refuse("c is 0 or in [4, 17]");
    if (ncols > B || (c && ncols)) refuse("ncols above 64, or ncols with digits (whole batches only)");
    if (live > n) refuse("more live positions than the domain has");
    if (m > n) refuse("more rows than the domain has");
    if (cap < debug_quotient_routes_bytes(c)) refuse("too small an output buffer");
    if (planes) for (size_t k = 0; k < 2; k++) for (size_t i = 0; i < m * B; i++) { const int8_t t = planes[k * n * B + i]; if (t != 0 && t != 1 && t != -1 && t != WS_PLANE_WIDE) refuse("a plane entry below row m that is not 0, 1, -1 or -128"); }
    HIP_CHECK(hipSetDevice(a.cfg.device));
    DevBuf<int8_t> d_planes(planes ? 2 * n * B : 0, true);
    DevBuf<uint4> d_digits(c ? debug_quotient_routes_bytes(c) / sizeof(uint4) : 0, true);
    debug_quotient(a, "gsc_debug_quotient", ab_be, 2, m, n, c ? nullptr : out, [&](const NttPlan& plan, AlgorithmImpl::Lane& ln, size_t) {
        // rows m .. n - 1 of a and b are nobody's: the kernels must not read them
        for (fe* mat : {ln.d_A.p, ln.d_B.p}) if (m < n) HIP_CHECK(hipMemsetAsync(mat + m * B, 0xFF, (n - m) * B * sizeof(fe), ln.stream));
        if (planes) d_planes.upload(planes, 2 * n * B, ln.stream);
        // crows = n: one group of 64 columns.  Without planes the pointers are null and `plain` still travels as given: clearing it is launch_quotient's rule
        const NttNarrow nr{{d_planes.p, planes ? d_planes.p + n * B : nullptr, nullptr}, n, plain};
        const NttNarrow* narrow = &nr;
        if (!c) return launch_compute_d(plan, ln.d_A.p, ln.d_B.p, m, B, ln.stream, ncols, narrow, live);
        HIP_CHECK(hipMemsetAsync(d_digits.p, 0, d_digits.bytes(), ln.stream));      // (live: the words of the other positions are not written)
        HIP_CHECK(launch_compute_d_digits(plan, ln.d_A.p, ln.d_B.p, m, B, QuotDigits{d_digits.p, c, msm_windows(c)}, ln.stream, narrow, live));
        HIP_CHECK(hipMemcpyAsync(out, d_digits.p, d_digits.bytes(), hipMemcpyDeviceToHost, ln.stream));
        return hipGetLastError();
    });
}
void Algorithm::debug_z_sum(const uint8_t* abc_be, size_t m, uint8_t* out, uint8_t* flags) {
    AlgorithmImpl& a = *impls_[0];
    if (!a.quotient_eval) throw std::runtime_error("debug_z_sum: the engine holds the coefficient form");
    HIP_CHECK(hipSetDevice(a.cfg.device));
    DevBuf<uint8_t> d_out(64 * 64), d_flags(64);
    debug_quotient(a, "debug_z_sum", abc_be, 3, m, a.n_constraints, nullptr, [&](const NttPlan& plan, AlgorithmImpl::Lane& ln, size_t B) {
        AlgorithmImpl::Chunk ck{nullptr, B, B, nullptr, chunk_route(B, a.cfg, a.route_facts(), RouteCall{}), {}, {}, {}};
        ln.small_active = false;
        // rows m .. n - 1 of a, b, c (and the padding row of c) are zero in this call
        for (fe* mat : {ln.d_A.p, ln.d_B.p, ln.d_C.p}) HIP_CHECK(hipMemsetAsync(mat + m * B, 0, (a.domain_n - m) * B * sizeof(fe), ln.stream));
        HIP_CHECK(hipMemsetAsync(ln.d_C.p + a.domain_n * B, 0, B * sizeof(fe), ln.stream));
        if (ck.rt.z_digits_ready) HIP_CHECK(launch_compute_d_digits(plan, ln.d_A.p, ln.d_B.p, a.n_constraints, B, QuotDigits{ln.d_digits.p, a.mZ.c, a.mZ.nwin}, ln.stream, nullptr, a.quot_live));
        else HIP_CHECK(launch_compute_d(plan, ln.d_A.p, ln.d_B.p, a.n_constraints, B, ln.stream, 0, nullptr, a.quot_live));
        a.run_msm_g1(ln, ck, a.mC, ln.d_C.p, 1, ln.d_sumC.p);
        a.run_msm_g1(ln, ck, a.mZ, ln.d_A.p, 0, ln.d_sumZ.p, false, false, ck.rt.z_digits_ready);
        a.flush_horner<G1Aff>(ln.pending1, B, ln.stream);
        launch_g1_sum_be(ln.d_sumC.p, ln.d_sumZ.p, B, d_out.p, d_flags.p, ln.stream);
        HIP_CHECK(hipMemcpyAsync(out, d_out.p, 64 * 64, hipMemcpyDeviceToHost, ln.stream));
        HIP_CHECK(hipMemcpyAsync(flags, d_flags.p, 64, hipMemcpyDeviceToHost, ln.stream));
        return hipGetLastError();
    });
}
// one replica: cut the request list into chunks (multiples of 64 proofs, at most one lane's capacity) and let worker threads pull
// chunks, each on whichever lane is free.  A call that fits one lane stays whole: cutting a lone 1024-statement AES-128 call over
// the two lanes doubles the latency-bound level launches of the witness stage, and the lanes' streams share a hardware queue more
// often than not, so nothing hides (round 4, profiles/r04_aes128_lanes.txt: 3 255 proofs/s cut, 3 341 - 3 362 whole; round 2 had
// measured +4 % for cutting, on slower MSM kernels).  min_split > 0 (test hook) brings the cut back: the tests use it to cover
// chunked calls with small batches.
static void prove_on_replica(AlgorithmImpl& a, const ProofRequest* reqs, size_t n, ProofResult* results, DebugVectors* debug_first, KernelStat* stat, std::mutex* stat_mu) {
    if (!n) return;
    const size_t nl = a.full_lanes, lane_cap = a.lanes[0]->cap;      // only full lanes take the chunks of a big call
    size_t nchunks = (n + lane_cap - 1) / lane_cap;
    struct InFlight { std::atomic<int>& c; int seen; explicit InFlight(std::atomic<int>& x) : c(x), seen(x.fetch_add(1) + 1) {} ~InFlight() { c.fetch_sub(1); } } me(a.calls_in_flight);
    if (nl > 1 && a.cfg.min_split && me.seen == 1 && n >= 2 * a.cfg.min_split) { const size_t want = (nchunks + nl - 1) / nl * nl; nchunks = want; }
    size_t chunk = ((n + nchunks - 1) / nchunks + 63) / 64 * 64;
    if (chunk > lane_cap) chunk = lane_cap;
    nchunks = (n + chunk - 1) / chunk;
    std::atomic<size_t> next{0};
    std::exception_ptr err; std::mutex err_mu;
    auto work = [&]() {
        try {
            HIP_CHECK(hipSetDevice(a.cfg.device));
            for (;;) {
                const size_t c = next.fetch_add(1);
                if (c >= nchunks) break;
                const size_t off = c * chunk, take = n - off < chunk ? n - off : chunk;
                struct Hold { AlgorithmImpl& a; size_t i; ~Hold() { a.release_lane(i); } } hold{a, a.acquire_lane(-1, take)};
                a.prove_chunk(*a.lanes[hold.i], reqs + off, take, results + off, off == 0 ? debug_first : nullptr);
                if (stat) { std::lock_guard<std::mutex> g(*stat_mu); if (a.lanes[hold.i]->stat.ms >= stat->ms) *stat = a.lanes[hold.i]->stat; }      // the call's chunk with the longest dominant kernel
            }
        } catch (...) { std::lock_guard<std::mutex> g(err_mu); if (!err) err = std::current_exception(); }
    };
    const size_t nthreads = nchunks < nl ? nchunks : nl;
    std::vector<std::thread> th;
    for (size_t t = 1; t < nthreads; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}
size_t Algorithm::debug_secret_residue() { size_t n = 0; for (auto& i : impls_) n += i->secret_residue(); return n; }
size_t Algorithm::debug_secret_scan(std::string& report) {
    size_t n = 0, registered = 0, allocated = 0, lane_base = 0;
    for (auto& i : impls_) { n += i->secret_scan(lane_base, report, registered, allocated); lane_base += i->lanes.size(); }
    report += "registered=" + std::to_string(registered) + " allocated=" + std::to_string(allocated) + " public=";
    bool first = true;
    for (int r = 0; r < WR_COUNT; r++) if (wipe_region_public(r)) { report += (first ? "" : ",") + std::string(wipe_region_name(r)); first = false; }
    return n;
}
size_t Algorithm::scrub_before_free() {
    std::string report; size_t registered = 0, allocated = 0, lane_base = 0, n = 0;
    for (auto& i : impls_) { n += i->secret_scan(lane_base, report, registered, allocated); lane_base += i->lanes.size(); }
    if (!n) return 0;
    for (auto& i : impls_) {
        HIP_CHECK(hipSetDevice(i->cfg.device));
        for (auto& ln : i->lanes) { i->wipe_whole(*ln, ln->stream); HIP_CHECK(hipStreamSynchronize(ln->stream)); }
    }
    return n;
}
std::vector<std::pair<int, size_t>> Algorithm::replica_bytes() const {
    std::vector<std::pair<int, size_t>> out;
    for (auto& i : impls_) { size_t b = i->held_bytes(); if (auto c = i->check_now()) b += prove_check_device_bytes(*c); out.emplace_back(i->cfg.device, b); }
    return out;
}
bool device_memory_info(int device, uint64_t out[4]) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || device >= 64) return false;
    // (hipMemGetInfo answers for the calling thread's current device: set for the query, put back behind it)
    int was = 0; if (hipGetDevice(&was) != hipSuccess) return false;
    size_t free_b = 0, total_b = 0;
    const bool ok = hipSetDevice(device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    (void)hipSetDevice(was);
    if (!ok) return false;
    out[0] = free_b; out[1] = total_b; out[2] = prover_bytes_on(device).load(); out[3] = verifier_device_bytes(device);
    return true;
}
void Algorithm::forget_thread_stat() const { if (t_call_owner == this) t_call_owner = nullptr; }
void Algorithm::prove_batch(const ProofRequest* reqs, size_t n, ProofResult* results, DebugVectors* debug_first, bool whole) {
    if (!n) return;
    struct Held { ReplicaPicker& p; size_t i, n; std::atomic<size_t>& last; ~Held() { p.release(i, n); last.store(i); } };
    KernelStat call_stat; std::mutex call_stat_mu;
    struct Publish { const Algorithm* self; KernelStat& st; ~Publish() { t_call_stat = st; t_call_owner = self; } } publish{this, call_stat};
    const std::vector<CallShare> shares = plan_shares(n, impls_.size(), impls_[0]->cap, whole);
    if (shares.size() == 1 && shares[0].pick) {
        // not split: the call goes, whole, to the least-loaded replica (ReplicaPicker) — concurrent single-proof callers and the
        // micro-batcher's batches therefore use every GPU of the node, not only the first one.
        Held h{*picker_, picker_->acquire(n), n, last_replica_};
        return prove_on_replica(*impls_[h.i], reqs, n, results, debug_first, &call_stat, &call_stat_mu);
    }
    // Proofs are independent: contiguous shares (multiples of 64) go to the replicas, one host thread per device; nothing is
    // exchanged between devices (the "gather" is the results array the threads fill).
    std::exception_ptr err; std::mutex err_mu; std::vector<std::thread> th;
    auto work = [&](const CallShare& sh) {
        picker_->acquire_on(sh.replica, sh.n);
        Held h{*picker_, sh.replica, sh.n, last_replica_};
        try { prove_on_replica(*impls_[sh.replica], reqs + sh.off, sh.n, results + sh.off, sh.off == 0 ? debug_first : nullptr, &call_stat, &call_stat_mu); }
        catch (...) { std::lock_guard<std::mutex> g(err_mu); if (!err) err = std::current_exception(); }
    };
    for (size_t k = 1; k < shares.size(); k++) th.emplace_back(work, shares[k]);
    work(shares[0]);
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}

}  // namespace gsc
