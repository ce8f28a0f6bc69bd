// Per-batch half of the engine: witness -> quotient -> MSMs -> assembly for one chunk of statements on one lane (prove_chunk and its
// stage_* functions; which kernels a chunk takes is decided once, by chunk_route.hpp), the lane adapters of the MSM calls (msm_run, msm_set.hpp) and proof
// serialisation.  See engine_impl.hpp; reference: groth16.Prove + proof.WriteTo behind
// libraries/prover/impl/provers.go:148-157, :216-226.
#include "engine_impl.hpp"
#include "glv.hpp"
#include "prove_check_kernels.hpp"
#include <chrono>
#include <cstdio>
#include <cstring>

namespace gsc {

FewSolverChain& few_solver_chain(int device) { static FewSolverChain* chains = new FewSolverChain[64]; return chains[device & 63]; }

namespace {
// (p-1)/2, big-endian: a compressed point carries the "larger y" flag iff y > (p-1)/2
const uint8_t kHalfP[32] = {0x18, 0x32, 0x27, 0x39, 0x70, 0x98, 0xd0, 0x14, 0xdc, 0x28, 0x22, 0xdb, 0x40, 0xc0, 0xac, 0x2e,
                            0xcb, 0xc0, 0xb5, 0x48, 0xb4, 0x38, 0xe5, 0x46, 0x9e, 0x10, 0x46, 0x0b, 0x6c, 0x3e, 0x7e, 0xa3};

void le_limbs_to_be(const uint8_t* le, uint8_t* be) { for (int i = 0; i < 32; i++) be[i] = le[31 - i]; }
bool be_greater(const uint8_t* a, const uint8_t* b) { int c = memcmp(a, b, 32); return c > 0; }
bool be_is_zero(const uint8_t* a) { for (int i = 0; i < 32; i++) if (a[i]) return false; return true; }
}  // namespace

void AlgorithmImpl::run_msm_g1(Lane& ln, const Chunk& ck, const MsmSet<G1Aff>& set, const fe* scalars, int mont, G1Xyzz* sum, bool timed, bool side, bool digits_ready) {
    const int k = set_index(set);
    MsmRun<G1Xyzz> r{MsmCtx{ln.stream, ln.d_digits_w.p && &set != &mZ ? ln.d_digits_w.p : ln.d_digits.p, ln.d_gok.p}, scalars, mont != 0, ck.B, ck.n, ck.rt.latency,
                     ln.d_part1a.p, ln.d_part1b.p, ln.d_sj1[k].p, ln.d_flat1[k].p, sum};
    if (side) {
        if (!set.latency_flat() || ck.B != 64) throw std::runtime_error("internal: side-stream MSM on a set with a windowed part");
        r.ctx = MsmCtx{ln.side, ln.d_digits_s.p, ln.d_gok_s.p}; r.pa = ln.d_part1c.p; r.pb = ln.d_part1d.p;
    } else {
        r.digits_ready = digits_ready;
        if (timed) {      // the dominant kernel (Z): its events, and at full batches its clock stamps
            r.ev_begin = ln.ev[5]; r.ev_end = ln.ev[6];
            if (!ck.rt.latency) r.clk = ln.d_clk.p;
            if (cfg.z_exp_entry_bits > 0 && cfg.z_exp_entry_bits < 31) r.clk_mask = (1u << cfg.z_exp_entry_bits) - 1;
        }
    }
    r.ctx = with_plane(r.ctx, ln, scalars); r.opts = msm_opts;
    msm_run<G1Aff, G1Xyzz>(set, r, ln.pending1);
}

void AlgorithmImpl::run_msm_g2(Lane& ln, const Chunk& ck, const MsmSet<G2Aff>& set, const fe* scalars, int mont, G2Xyzz* sum, bool side) {
    if (side && (!set.latency_flat() || ck.B != 64)) throw std::runtime_error("internal: side-stream MSM on a set with a windowed part");
    MsmRun<G2Xyzz> r{with_plane(side ? MsmCtx{ln.side2, ln.d_digits_s2.p, ln.d_gok_s2.p} : MsmCtx{ln.stream, ln.d_digits_w.p ? ln.d_digits_w.p : ln.d_digits.p, ln.d_gok.p}, ln, scalars),
                     scalars, mont != 0, ck.B, ck.n, ck.rt.latency, ln.d_part2a.p, ln.d_part2b.p, ln.d_sj2.p, ln.d_flat2.p, sum};
    r.opts = msm_opts;
    msm_run<G2Aff, G2Xyzz>(set, r, ln.pending2);
}

void AlgorithmImpl::fetch_column(Lane& ln, const fe* mat, size_t rows, size_t B, size_t col, std::vector<uint8_t>& out) {
    out.resize(rows * 32);
    HIP_CHECK(hipMemcpy2DAsync(out.data(), 32, reinterpret_cast<const uint8_t*>(mat) + 32 * col, B * 32, 32, rows, hipMemcpyDeviceToHost, ln.stream));
    HIP_CHECK(hipStreamSynchronize(ln.stream));
}

void AlgorithmImpl::wipe_secrets(Lane& ln, size_t B, bool small_call) {
    if (cfg.keep_secrets) return;      // (test hook: shows that secret_residue() sees what the wipe removes)
    const size_t n_secret = n_inputs - n_public;
    HIP_CHECK(hipMemsetAsync(ln.d_inputs.p, 0, 176 * B, ln.stream));
    HIP_CHECK(hipMemsetAsync(ln.d_rs.p, 0, 64 * B, ln.stream));
    HIP_CHECK(hipMemsetAsync(ln.d_glv.p, 0, ln.d_glv.bytes(), ln.stream));
    if (has_commitment) { HIP_CHECK(hipMemsetAsync(ln.d_mask_in.p, 0, 32 * B, ln.stream)); HIP_CHECK(hipMemsetAsync(ln.d_mask.p, 0, B * sizeof(fe), ln.stream)); }
    HIP_CHECK(hipMemsetAsync(ln.d_W.p + n_public * B, 0, n_secret * B * sizeof(fe), ln.stream));      // the key wires
    HIP_CHECK(hipMemsetAsync(ln.d_W.p + n_wires * B, 0, 3 * B * sizeof(fe), ln.stream));               // r, s, -rs
    if (small_call) HIP_CHECK(hipMemset2DAsync(ln.d_W8.p + n_public * 64, (size_t)small.rows_per_group * 64, 0, n_secret * 64, B / 64, ln.stream));
}

WipePlan AlgorithmImpl::plan_wipe(const Lane& ln, const Chunk& ck) const {
    WipeSizes z;
    z.B = ck.B; z.n = ck.n; z.n_wires = n_wires; z.n_constraints = n_constraints; z.domain_n = domain_n; z.rows_per_group = small.ok ? small.rows_per_group : 0;
    z.fe_bytes = sizeof(fe); z.xyzz1_bytes = sizeof(G1Xyzz); z.xyzz2_bytes = sizeof(G2Xyzz);
    const Lane::ScratchNeed& nd = ln.need_at.at(ck.B / 64 - 1);
    z.part1a = nd.part1a; z.part1b = nd.part1b; z.part2a = nd.part2a; z.part2b = nd.part2b; z.digits = nd.digits; z.digits_w = nd.digits_w; z.gok = nd.gok; z.sj2 = nd.sj2;
    for (int k = 0; k < Lane::NSETS; k++) z.sj1[k] = nd.sj1[k];
    std::vector<WipeRegionInfo> table;
    for (const Lane::Region& r : ln.regions) table.push_back(WipeRegionInfo{r.region, r.bytes});
    return wipe_plan(ck.rt, route_facts(), z, table);
}

void AlgorithmImpl::run_wipe(Lane& ln, const std::vector<WipeItem>& items, hipStream_t s, unsigned max_blocks) {
    std::vector<WipeDesc> ds;
    for (const WipeItem& it : items) {
        const Lane::Region* reg = nullptr;
        for (const Lane::Region& r : ln.regions) if (r.region == it.region) reg = &r;
        if (!reg || wipe_region_public(it.region)) throw std::runtime_error("internal: wipe of a region the lane does not hold");
        // inside the allocation, whatever the plan said (a kernel that writes out of bounds is worse than a region left dirty, which the scan would show)
        if (!it.rows || !it.width) continue;
        if (it.offset > reg->bytes || it.width > reg->bytes || it.pitch > reg->bytes || it.rows > reg->bytes || it.offset + (it.rows - 1) * it.pitch + it.width > reg->bytes || (it.rows > 1 && it.pitch < it.width))
            throw std::runtime_error(std::string("internal: wipe descriptor outside region ") + wipe_region_name(it.region));
        const uint8_t* cls = nullptr;
        if (it.image) cls = it.region == WR_A8 ? ws_cls_a.p : it.region == WR_B8 ? ws_cls_b.p : it.region == WR_C8 ? ws_cls_c.p : nullptr;
        if (it.image && !cls) throw std::runtime_error("internal: plane image of a region that is no plane");
        ds.push_back(WipeDesc{reg->p + it.offset, it.rows, it.pitch, it.width, cls, it.image ? it.image_period : 0});
    }
    launch_wipe(ds.data(), ds.size(), max_blocks, s);
    HIP_CHECK(hipGetLastError());
}

// Phase A: from here on the call only reads the Z sum's digits and the tables (and, with a commitment, the committed wires once more: the plan keeps
// those back).  The Z kernel is VALU-bound and leaves HBM idle, so the fill goes beside it on the lane's low-priority stream with a
// bounded grid; phase B waits for it.
void AlgorithmImpl::wipe_phase_a(Lane& ln, const Chunk& ck) {
    ln.wipe_a_pending = false;
    if (cfg.keep_secrets || !cfg.wipe_full || ck.rt.latency) return;
    const WipePlan p = plan_wipe(ln, ck);
    if (p.a.empty()) return;
    HIP_CHECK(hipEventRecord(ln.ev_wa, ln.stream));
    HIP_CHECK(hipStreamWaitEvent(ln.side2, ln.ev_wa, 0));
    run_wipe(ln, p.a, ln.side2, cfg.wipe_grid ? (unsigned)cfg.wipe_grid : WIPE_GRID_BESIDE);
    HIP_CHECK(hipEventRecord(ln.ev_wa_done, ln.side2));
    ln.wipe_a_pending = true;
}

void AlgorithmImpl::wipe_phase_b(Lane& ln, const Chunk& ck) {
    if (cfg.keep_secrets) return;
    if (!cfg.wipe_full) return wipe_secrets(ln, ck.B, ck.rt.small);
    const WipePlan p = plan_wipe(ln, ck);
    if (ln.wipe_a_pending) { HIP_CHECK(hipStreamWaitEvent(ln.stream, ln.ev_wa_done, 0)); ln.wipe_a_pending = false; }
    else if (!p.a.empty()) throw std::runtime_error("internal: phase A of the wipe was not enqueued");
    run_wipe(ln, p.b, ln.stream, 0);
}

void AlgorithmImpl::wipe_whole(Lane& ln, hipStream_t s) {
    std::vector<WipeRegionInfo> table;
    for (const Lane::Region& r : ln.regions) table.push_back(WipeRegionInfo{r.region, r.bytes});
    run_wipe(ln, wipe_plan_whole(table, n_constraints), s, 0);
}

size_t AlgorithmImpl::secret_scan(size_t lane_base, std::string& report, size_t& registered, size_t& allocated) {
    HIP_CHECK(hipSetDevice(cfg.device));
    size_t total = 0;
    for (size_t li = 0; li < lanes.size(); li++) {
        Lane& ln = *lanes[li];
        HIP_CHECK(hipStreamSynchronize(ln.side)); HIP_CHECK(hipStreamSynchronize(ln.side2)); HIP_CHECK(hipStreamSynchronize(ln.stream));
        std::vector<WipeRegionInfo> table;
        for (const Lane::Region& r : ln.regions) { table.push_back(WipeRegionInfo{r.region, r.bytes}); registered += r.bytes; }
        allocated += ln.allocated;
        const std::vector<WipeItem> items = wipe_plan_whole(table, n_constraints);
        DevBuf<unsigned long long> d_cnt(items.size() + 1);
        HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, d_cnt.bytes(), ln.stream));
        for (size_t k = 0; k < items.size(); k++) {
            const WipeItem& it = items[k];
            const Lane::Region* reg = nullptr;
            for (const Lane::Region& r : ln.regions) if (r.region == it.region) reg = &r;
            const uint8_t* cls = !it.image ? nullptr : it.region == WR_A8 ? ws_cls_a.p : it.region == WR_B8 ? ws_cls_b.p : ws_cls_c.p;
            launch_scan_idle(WipeDesc{reg->p + it.offset, it.rows, it.pitch, it.width, cls, it.image ? it.image_period : 0}, d_cnt.p + k, ln.stream);
        }
        HIP_CHECK(hipGetLastError());
        std::vector<unsigned long long> h(items.size() + 1);
        HIP_CHECK(hipMemcpyAsync(h.data(), d_cnt.p, h.size() * 8, hipMemcpyDeviceToHost, ln.stream));
        HIP_CHECK(hipStreamSynchronize(ln.stream));
        for (size_t k = 0; k < items.size(); k++) if (h[k]) { total += h[k]; report += "lane" + std::to_string(lane_base + li) + "." + wipe_region_name(items[k].region) + "=" + std::to_string(h[k]) + " "; }
    }
    return total;
}

size_t AlgorithmImpl::secret_residue() {
    HIP_CHECK(hipSetDevice(cfg.device));
    size_t left = 0;
    auto count = [&](const void* p, size_t bytes) {
        std::vector<uint8_t> h(bytes);
        HIP_CHECK(hipMemcpy(h.data(), p, bytes, hipMemcpyDeviceToHost));
        for (uint8_t b : h) left += b != 0;
    };
    const size_t n_secret = n_inputs - n_public;
    for (auto& lp : lanes) {
        Lane& ln = *lp; const size_t B = ln.cap;
        HIP_CHECK(hipStreamSynchronize(ln.stream));
        count(ln.d_inputs.p, 176 * B); count(ln.d_rs.p, 64 * B); count(ln.d_glv.p, ln.d_glv.bytes());
        if (has_commitment) { count(ln.d_mask_in.p, 32 * B); count(ln.d_mask.p, B * sizeof(fe)); }
        // a chunk lays its rows out with ITS batch as the row stride (and wiped them in that layout): look where the lane's last chunk had them
        const size_t Bl = ln.last_batch;
        if (Bl) { count(ln.d_W.p + n_public * Bl, n_secret * Bl * sizeof(fe)); count(ln.d_W.p + n_wires * Bl, 3 * Bl * sizeof(fe)); }
        if (small.ok) for (size_t g = 0; g < B / 64; g++) count(ln.d_W8.p + (g * small.rows_per_group + n_public) * 64, n_secret * 64);
    }
    return left;
}

void AlgorithmImpl::stage_upload(Lane& ln, const Chunk& ck) {
    const size_t n = ck.n, B = ck.B;
    uint8_t* const h_in = ln.h_in.p; uint8_t* const h_rs = ln.h_rs.p; GlvSplit* const h_glv = ln.h_glv.p;
    pack_inputs(ck.reqs, n, B, h_in, h_rs);
    ln.d_inputs.upload(h_in, 176 * B, ln.stream);
    ln.d_rs.upload(h_rs, 64 * B, ln.stream);
    if (ck.rt.latency) {      // the two halves of s and r for k_fin_scalarmul_few
        for (size_t i = 0; i < n; i++) for (int role = 0; role < 2; role++) {
            uint32_t w[8]; memcpy(w, h_rs + 64 * i + (role == 0 ? 32 : 0), 32);
            if (!glv_split(w, h_glv[2 * i + role])) throw std::runtime_error("internal: scalar split out of range");
        }
        ln.d_glv.upload(h_glv, 2 * n, ln.stream);
    }
    HIP_CHECK(hipMemsetAsync(ln.d_flags.p, 0, ln.d_flags.bytes(), ln.stream));
    HIP_CHECK(hipEventRecord(ln.ev[0], ln.stream));
}

void AlgorithmImpl::run_levels(Lane& ln, const Chunk& ck, SolverArgs& sa, uint32_t from, uint32_t to) {
    SolverWalk walk;
    walk.n = ck.n; walk.resident = ck.rt.resident; walk.workgroups = cfg.few_workgroups > 0 ? (uint32_t)cfg.few_workgroups : 0u; walk.cu_count = cu_count; walk.device = cfg.device;
    walk.test_abort = cfg.few_test_abort != 0; walk.fsync = ln.d_fsync.p; walk.ev_few = ln.ev_few;
    solver_run_levels(*this, sa, walk, from, to, ln.stream);
}

// Circuits whose witness is small integers (ChaCha20-V3): the integer kernels on byte planes (wit_small.hpp) instead of the level launches
void AlgorithmImpl::solve_small(Lane& ln, const Chunk& ck) {
    solver_run_small(*this, SmallBuffers{ln.d_W.p, ln.d_A.p, ln.d_B.p, ln.d_C.p, ln.d_W8.p, ln.d_A8.p, ln.d_B8.p, ln.d_C8.p, ln.d_status.p, ln.d_wsflag.p}, ck.B, ck.dbg != nullptr, ln.stream);
}

void AlgorithmImpl::dump_solver_trace(Lane& ln, const unsigned long long* d_trace) {
    HIP_CHECK(hipStreamSynchronize(ln.stream));
    std::vector<unsigned long long> t(16 * ((size_t)n_levels + 1));
    HIP_CHECK(hipMemcpy(t.data(), d_trace, t.size() * 8, hipMemcpyDeviceToHost));
    { const unsigned long long* w = t.data() + 16 * (size_t)n_levels; if (w[2] > w[0]) fprintf(stderr, "last launch: %.1f us, shader clock %.0f MHz\n", (double)(w[2] - w[0]) / 100.0, (double)(w[3] - w[1]) / ((double)(w[2] - w[0]) / 100.0)); }
    fprintf(stderr, "solver trace: us after the level's first stamp (0 = not taken) | next level starts\n");
    for (uint32_t l = 0; l < n_levels; l++) {
        if (level_kind[l]) continue;
        fprintf(stderr, "level %3u w %4u long %3u |", l, level_width[l], level_long[l]);
        for (int k = 1; k < 13; k++) fprintf(stderr, " %6.2f", t[16 * l + k] ? (double)(t[16 * l + k] - t[16 * l]) / 100.0 : 0.0);
        if (l + 1 < n_levels && !level_kind[l + 1]) fprintf(stderr, " | %6.2f", (double)(t[16 * l + 16] - t[16 * l]) / 100.0);
        fprintf(stderr, "\n");
    }
}

void AlgorithmImpl::stage_witness(Lane& ln, const Chunk& ck) {
    const size_t n = ck.n, B = ck.B;
    if (cipher == CHACHA20) launch_assign_chacha(ln.d_inputs.p, ln.d_W.p, B, ln.stream);
    else launch_assign_aes(ln.d_inputs.p, cipher == AES_128 ? 16 : 32, ln.d_W.p, B, ln.stream);
    if (has_commitment) {
        for (size_t i = 0; i < B; i++) memcpy(ln.h_mask.p + 32 * i, ck.reqs[i < n ? i : n - 1].mask, 32);
        ln.d_mask_in.upload(ln.h_mask.p, 32 * B, ln.stream);
    }
    launch_prep_rs(ln.d_rs.p, ln.d_W.p, n_wires, B, has_commitment ? ln.d_mask_in.p : nullptr, ln.d_mask.p, ln.stream);
    HIP_CHECK(hipMemsetAsync(ln.d_status.p, 0xFF, B * 4, ln.stream));
    SolverArgs sa{prog.p, sched.p, 0, n_levels, coeff.p, coeff_inv.p, lookup_coeff.p, ln.d_W.p, ln.d_A.p, ln.d_B.p, ln.d_C.p, B, ln.d_status.p,
                  has_commitment ? ln.d_mask.p : nullptr, has_commitment ? ln.d_commit.p : nullptr, has_div, 0u, nullptr};
    DevBuf<unsigned long long> d_trace; d_trace.secret = true;      // (when a level ran says something about its values)
    if (cfg.solver_trace) {
        std::vector<unsigned long long> init(16 * ((size_t)n_levels + 1), 0ull);
        if (!ck.rt.resident_wanted) for (uint32_t l = 0; l < n_levels; l++) init[16 * l] = ~0ull;
        d_trace.alloc(init.size()); HIP_CHECK(hipMemcpy(d_trace.p, init.data(), init.size() * 8, hipMemcpyHostToDevice)); sa.trace = d_trace.p;
    }
    if (ck.rt.resident) HIP_CHECK(hipMemsetAsync(ln.d_fsync.p + 1, 0, 4, ln.stream));      // set by a resident launch that gave up at a barrier
    if (ck.rt.latency) HIP_CHECK(hipEventRecord(ln.ev[5], ln.stream));      // dominant kernel of a latency-path call: the witness solver
    if (has_commitment) {
        // Groth16 commitment (gnark "BSB22"): solve up to the commitment hint, D = sum w_j * Basis_j over the
        // committed wires (same MSM kernels as everything else), challenge = hash_to_field(D uncompressed) on the device, resume:
        // nothing leaves the stream.
        run_levels(ln, ck, sa, 0, commit_level);
        run_msm_g1(ln, ck, mPed, ln.d_W.p, 1, ln.d_sumD.p);
        flush_horner<G1Aff>(ln.pending1, B, ln.stream);
        launch_points_to_affine_be(ln.d_sumD.p, B, ln.d_cpts.p, ln.d_flags.p, 8, ln.stream);
        launch_challenge_from_point(ln.d_cpts.p, ln.d_commit.p, B, ln.stream);
        run_levels(ln, ck, sa, commit_level, n_levels);
    } else if (ck.rt.small) solve_small(ln, ck);
    else run_levels(ln, ck, sa, 0, n_levels);
    if (ck.rt.latency) HIP_CHECK(hipEventRecord(ln.ev[6], ln.stream));
    if (cfg.solver_trace) dump_solver_trace(ln, d_trace.p);
    HIP_CHECK(hipEventRecord(ln.ev[1], ln.stream));
    if (DebugVectors* dbg = ck.dbg) {
        dbg->n_wires = n_wires; dbg->n_constraints = n_constraints; dbg->n = domain_n;
        fetch_column(ln, ln.d_W.p, n_wires, B, 0, dbg->W); fetch_column(ln, ln.d_A.p, n_constraints, B, 0, dbg->A);
        fetch_column(ln, ln.d_B.p, n_constraints, B, 0, dbg->B); fetch_column(ln, ln.d_C.p, n_constraints, B, 0, dbg->C);
    }
}

// A latency-path call leaves the chip mostly idle, so its A and B1 sums and the two scalar multiplications that need them (s * Ar,
// r * Bs1: 254 serial doublings, 2 ms) start on the side stream right after the witness, beside the quotient and the other MSMs.
void AlgorithmImpl::stage_early_sums(Lane& ln, const Chunk& ck) {
    if (ck.rt.early_ab) {
        HIP_CHECK(hipEventRecord(ln.ev_ab, ln.stream));
        HIP_CHECK(hipStreamWaitEvent(ln.side, ln.ev_ab, 0));
        run_msm_g1(ln, ck, mA, ln.d_W.p, 1, ln.d_sumA.p, false, true);
        run_msm_g1(ln, ck, mB1, ln.d_W.p, 1, ln.d_sumB1.p, false, true);
        launch_fin_scalarmul_few(ln.d_sumA.p, ln.d_sumB1.p, ln.d_glv.p, ck.B, ck.n, ln.d_out.p, ln.d_flags.p, ln.d_tmp.p, ln.side);
    }
    if (ck.rt.early_b2) {         // the G2 sum too (it only reads the witness): a third stream
        HIP_CHECK(hipStreamWaitEvent(ln.side2, ln.ev_ab, 0));
        run_msm_g2(ln, ck, mB2, ln.d_W.p, 1, ln.d_sumB2.p, true);
        HIP_CHECK(hipEventRecord(ln.ev_s2, ln.side2));
    }
}

// Quotient polynomial.  Coefficient form: h overwrites A, canonical, bit-reversed order (six transforms).  Evaluation form (batch calls,
// k_quot_bases.hip): d = A B on the zeta-coset overwrites A, natural order (four transforms); c stays where the solver wrote it.
void AlgorithmImpl::stage_quotient(Lane& ln, const Chunk& ck) {
    const size_t B = ck.B; const ChunkRoute& rt = ck.rt; DebugVectors* const dbg = ck.dbg;
    NttPlan plan{L, tw_fwd.p, tw_inv.p, scale_mid.p, scale_out.p, dom.p + 5, qr.p, cfg.trace_host ? ln.d_clk.p + 32 : nullptr, tw_inv_plain.p, scale_mid_plain.p};
    const NttNarrow planes{{ln.d_A8.p, ln.d_B8.p, ln.d_C8.p}, n_constraints, cfg.ntt_plain};
    const NttNarrow* narrow = rt.small ? &planes : nullptr;      // a, b (and c) of this chunk are byte planes
    const size_t few_cols = rt.latency ? ck.n : 0;               // latency path: the statements' columns only
    HIP_CHECK(hipGetLastError());      // witness launches (launch-configuration errors are not sticky: check each group)
    // The evaluation-form quotient of a batch call reads a and b (rows or byte planes) and writes d over a and its digits into the Z set's own
    // digit buffer; the wire-set sums (A, B1, B2, K, and c over mC) read W and c and recode into d_digits_w.  Nothing is shared, so the
    // three quotient kernels go to the lane's third stream (rt.overlap_q) and the wire sets' thin tails (slice reductions, Horner chains, recoders: 5 ms of
    // a 1024-statement call's 54, none of it chip-filling) run under them; the Z sum waits for both.  Measured (profiles/r04k_overlap_quotient.txt):
    // 64 / 256 / 512 / 1024 statements per call +2 / +8 / +6 / +3.5 %, 8192 +0.1 %, AES-128 1024 / 256 per call +2.8 / +7 % — once the lanes'
    // streams stopped sharing hardware queues (alloc_lane); before that, calls on the small lanes lost 2 - 5 % to it.  Calls of 4096 statements
    // and more keep the one-stream order: nothing to gain (their tails are 1 % of the call), and the stage times stay those of the kernels.
    hipStream_t qs = rt.overlap_q ? ln.side2 : ln.stream;
    if (rt.eval) {
        if (dbg) {      // the debug vector is h itself: the coefficient-form kernels on copies (they overwrite their inputs)
            DevBuf<fe> ta(domain_n * B, true), tb(domain_n * B, true), tc(domain_n * B, true);
            HIP_CHECK(hipMemcpyAsync(ta.p, ln.d_A.p, n_constraints * B * sizeof(fe), hipMemcpyDeviceToDevice, ln.stream));
            HIP_CHECK(hipMemcpyAsync(tb.p, ln.d_B.p, n_constraints * B * sizeof(fe), hipMemcpyDeviceToDevice, ln.stream));
            HIP_CHECK(hipMemcpyAsync(tc.p, ln.d_C.p, n_constraints * B * sizeof(fe), hipMemcpyDeviceToDevice, ln.stream));
            HIP_CHECK(launch_compute_h(plan, ta.p, tb.p, tc.p, n_constraints, B, ln.stream, 0));
            fetch_column(ln, ta.p, domain_n, B, 0, dbg->H);
        }
        if (rt.overlap_q) HIP_CHECK(hipStreamWaitEvent(qs, ln.ev[1], 0));      // the end of the witness stage
        if (rt.z_digits_ready) HIP_CHECK(launch_compute_d_digits(plan, ln.d_A.p, ln.d_B.p, n_constraints, B, QuotDigits{ln.d_digits.p, mZ.c, mZ.nwin}, qs, narrow, quot_live));
        else HIP_CHECK(launch_compute_d(plan, ln.d_A.p, ln.d_B.p, n_constraints, B, ln.stream, few_cols, narrow, quot_live));      // (the recoding pass reads mZ's rows: live positions)
    } else HIP_CHECK(launch_compute_h(plan, ln.d_A.p, ln.d_B.p, ln.d_C.p, n_constraints, B, ln.stream, few_cols, narrow));
    HIP_CHECK(hipEventRecord(ln.ev[2], qs));
    if (dbg && !rt.eval) fetch_column(ln, ln.d_A.p, domain_n, B, 0, dbg->H);
}

// The MSMs.  (With fuse_z_digits the digits of d are already in the lane's Z digit buffer; every other set recodes into d_digits_w.)
// A and B1 first: the two scalar multiplications of the assembly only need those two sums and run on a side stream
// beside the remaining MSMs.
void AlgorithmImpl::stage_msms(Lane& ln, const Chunk& ck) {
    const size_t B = ck.B; const ChunkRoute& rt = ck.rt;
    if (!rt.early_ab) {
        run_msm_g1(ln, ck, mA, ln.d_W.p, 1, ln.d_sumA.p);
        run_msm_g1(ln, ck, mB1, ln.d_W.p, 1, ln.d_sumB1.p);
        flush_horner<G1Aff>(ln.pending1, B, ln.stream);                                       // (AES-V2: the wide wires of A and B1; nothing for ChaCha20-V3)
        HIP_CHECK(hipEventRecord(ln.ev_ab, ln.stream));
        HIP_CHECK(hipStreamWaitEvent(ln.side, ln.ev_ab, 0));
        launch_fin_scalarmul(ln.d_sumA.p, ln.d_sumB1.p, ln.d_rs.p, B, ln.d_out.p, ln.d_flags.p, ln.d_tmp.p, ln.side);
    }
    if (!rt.early_b2) run_msm_g2(ln, ck, mB2, ln.d_W.p, 1, ln.d_sumB2.p);
    if (ln.pending2.n) {                                                         // the G2 Horner chain (3x a G1 one) also goes beside the MSMs
        HIP_CHECK(hipEventRecord(ln.ev_b2, ln.stream));
        HIP_CHECK(hipStreamWaitEvent(ln.side, ln.ev_b2, 0));
        flush_horner<G2Aff>(ln.pending2, B, ln.side);
    }
    HIP_CHECK(hipEventRecord(ln.ev_fs, ln.side));
    run_msm_g1(ln, ck, mK, ln.d_W.p, 1, ln.d_sumK.p);
    if (rt.eval) {                                                               // sum c_i U_i: the solver's c rows, laid out like a wire set
        // the padding slots of mC read row n of c, which must be zero for THIS batch's row stride (an earlier, larger batch had other rows there)
        HIP_CHECK(hipMemsetAsync(ln.d_C.p + domain_n * B, 0, B * sizeof(fe), ln.stream));
        run_msm_g1(ln, ck, mC, ln.d_C.p, 1, ln.d_sumC.p);
    }
    if (rt.overlap_q) { HIP_CHECK(hipEventRecord(ln.ev_ws, ln.stream)); HIP_CHECK(hipStreamWaitEvent(ln.stream, ln.ev[2], 0)); }      // the wire sets are through; wait for d and its digits
    wipe_phase_a(ln, ck);      // the witness, a, b, c and the wire sets' digits have had their last reader
    run_msm_g1(ln, ck, rt.use_zfew ? mZfew : mZ, ln.d_A.p, 0, ln.d_sumZ.p, !rt.latency, false, rt.z_digits_ready);
    if (has_commitment) run_msm_g1(ln, ck, mPedSigma, ln.d_W.p, 1, ln.d_sumPok.p);      // proof of knowledge of the commitment: same scalars over sigma * Basis
    flush_horner<G1Aff>(ln.pending1, B, ln.stream);                                           // K, Z, PedSigma: one launch
    if (has_commitment) launch_points_to_affine_be(ln.d_sumPok.p, B, ln.d_cpts.p + 64 * B, ln.d_flags.p, 16, ln.stream);
    HIP_CHECK(hipGetLastError());      // MSM launches
    HIP_CHECK(hipEventRecord(ln.ev[3], ln.stream));
}

void AlgorithmImpl::stage_assembly(Lane& ln, Chunk& ck) {
    const size_t B = ck.B; const ChunkRoute& rt = ck.rt;
    HIP_CHECK(hipStreamWaitEvent(ln.stream, ln.ev_fs, 0));
    if (rt.early_b2) HIP_CHECK(hipStreamWaitEvent(ln.stream, ln.ev_s2, 0));
    launch_fin_combine(ln.d_sumB2.p, ln.d_sumK.p, ln.d_sumZ.p, rt.eval ? ln.d_sumC.p : nullptr, ln.d_tmp.p, B, ln.d_out.p, ln.d_flags.p, ln.stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ln.ev[4], ln.stream));
    if (ck.corrupt) {      // TEST HOOK: behind the last writer of the proof's points, in front of the check and the download
        launch_prove_corrupt(ln.d_out.p, ln.d_cpts.p, B, ck.n, (uint32_t)ck.corrupt, (int)((ck.corrupt >> 32) & 0xFF), (int)((ck.corrupt >> 40) & 0xFF), ln.stream);
        HIP_CHECK(hipGetLastError());
    }
    const std::unique_ptr<ProveCheckPass> pass = ck.check ? check_enqueue(ln, ck) : nullptr;
    HIP_CHECK(hipMemcpyAsync(ln.h_out.p, ln.d_out.p, 256 * B, hipMemcpyDeviceToHost, ln.stream));
    HIP_CHECK(hipMemcpyAsync(ln.h_flags.p, ln.d_flags.p, (B + 3) / 4 * 4, hipMemcpyDeviceToHost, ln.stream));
    HIP_CHECK(hipMemcpyAsync(ln.h_status.p, ln.d_status.p, B * 4, hipMemcpyDeviceToHost, ln.stream));
    if (has_commitment) HIP_CHECK(hipMemcpyAsync(ln.h_cpts.p, ln.d_cpts.p, 128 * B, hipMemcpyDeviceToHost, ln.stream));      // commitment | its proof of knowledge
    memset(ln.h_words.p, 0, ln.h_words.bytes());      // the small result words (Lane::h_fsync, h_wsflag, h_clk)
    if (rt.resident) HIP_CHECK(hipMemcpyAsync(ln.h_fsync(), ln.d_fsync.p, 8, hipMemcpyDeviceToHost, ln.stream));
    if (rt.small) HIP_CHECK(hipMemcpyAsync(&ln.h_wsflag(), ln.d_wsflag.p, 4, hipMemcpyDeviceToHost, ln.stream));
    wipe_phase_b(ln, ck);      // behind the last kernel of the chunk, inside the wait below
    if (!rt.latency) { HIP_CHECK(hipMemcpyAsync(ln.h_clk(), ln.d_clk.p, (cfg.trace_host ? 44 : 32) * 8, hipMemcpyDeviceToHost, ln.stream)); HIP_CHECK(hipMemsetAsync(ln.d_clk.p, 0, 32 * 8, ln.stream)); }
    ck.t_enqueued = std::chrono::steady_clock::now();
    HIP_CHECK(hipStreamSynchronize(ln.stream));
    if (pass) {
        ck.verdict = pass->finish(ln.h_status.p, ln.h_flags.p); ck.check_fell_back = pass->fell_back();
        // a chunk that is proved again (prove_chunk) is counted when it comes through here for the last time; what counts is what would have been released
        if (!ln.h_fsync()[1] && !ln.h_wsflag()) {
            size_t checked = 0, refused = 0;
            for (size_t i = 0; i < ck.n; i++) if (ln.h_status.p[i] == 0xFFFFFFFFu && !ln.h_flags.p[i]) { checked++; refused += !ck.verdict[i]; }
            pass->count(checked, refused);
        }
    }
    ck.t_done = std::chrono::steady_clock::now();
}

std::unique_ptr<ProveCheckPass> AlgorithmImpl::check_enqueue(Lane& ln, const Chunk& ck) {
    // the public signals as the caller's verifier builds them: the host's own ciphertext and the request, never the witness
    std::vector<uint8_t> sig(144 * ck.n);
    for (size_t i = 0; i < ck.n; i++) {
        const ProofRequest& q = ck.reqs[i]; uint8_t* o = sig.data() + 144 * i;
        memcpy(o, q.ciphertext, 64); memcpy(o + 64, q.nonce, 12);
        for (int b = 0; b < 4; b++) o[76 + b] = (uint8_t)(q.counter >> (8 * (cipher == CHACHA20 ? b : 3 - b)));      // little-endian for ChaCha20, big-endian for AES (verifiers.go)
        memcpy(o + 80, q.plaintext, 64);
    }
    return std::make_unique<ProveCheckPass>(ck.check, ProveCheckInput{ln.d_out.p, ln.d_cpts.p, ln.d_status.p, ln.d_flags.p, ck.B, ck.n, sig.data()}, ln.stream);
}

void AlgorithmImpl::stage_stat(Lane& ln, const Chunk& ck) {
    for (int k = 0; k < 4; k++) { float ms = 0; (void)hipEventElapsedTime(&ms, ln.ev[k], ln.ev[k + 1]); ln.stage_ms[k] = ms; }
    if (ck.rt.overlap_q) {
        // The quotient ran beside the wire-set MSMs: the stages stay a partition of the call's time, with the shared span charged to the MSMs —
        // msm = (witness end .. wire sets through) + (quotient end .. MSMs through), quotient = what it still ran alone after the wire sets
        float ws = 0, q = ln.stage_ms[1];
        (void)hipEventElapsedTime(&ws, ln.ev[1], ln.ev_ws);
        if (ws > q) ws = q;
        ln.stage_ms[1] = q - ws; ln.stage_ms[2] += ws;
    }
    (void)hipEventElapsedTime(&ln.msm_z_kernel_ms, ln.ev[5], ln.ev[6]); ln.last_batch = ck.B;
    KernelStat& st = ln.stat;
    st.name = ck.rt.kernel_name;
    st.ms = ln.msm_z_kernel_ms; st.statements = ck.n; st.columns = ck.B; st.nbases = mZ.digit_bases ? mZ.digit_bases : mZ.nwide; st.nwin = mZ.nwin;
    for (int k = 0; k < 4; k++) st.stage_ms[k] = ln.stage_ms[k];
    // shader clock of the Z launch: (shader-clock ticks) / (100 MHz ticks) over the lives of eight waves spread over the grid, one on each XCD
    // (the XCDs are clocked separately; a pair of stamps from two different waves is useless: the shader-clock counters are not chip-wide —
    // first-start-to-last-end read 1 772 ... 2 323 MHz on launches whose waves all saw 2 010 ... 2 069)
    double ticks = 0, shader = 0;
    if (!ck.rt.latency) for (int k = 0; k < 8; k++) { const unsigned long long* c = ln.h_clk() + 4 * k; if (c[2] > c[0] && c[3] > c[1]) { ticks += (double)(c[2] - c[0]); shader += (double)(c[3] - c[1]); } }
    st.clock_mhz = ticks > 0 ? (float)(100.0 * shader / ticks) : 0.f;
    std::lock_guard<std::mutex> lk(stat_mu);
    last_stat = st;
}

void AlgorithmImpl::trace_chunk(Lane& ln, const Chunk& ck) {
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "prove_chunk(%zu): enqueue %.2f ms, wait %.2f ms, serialise %.2f ms\n", ck.n, ms(ck.t_start, ck.t_enqueued), ms(ck.t_enqueued, ck.t_done), ms(ck.t_done, std::chrono::steady_clock::now()));
    auto mhz = [&](int k) { const unsigned long long* c = ln.h_clk() + 4 * k; return c[2] > c[0] && c[3] > c[1] ? 100.0 * (double)(c[3] - c[1]) / (double)(c[2] - c[0]) : 0.0; };
    if (!ck.rt.latency) fprintf(stderr, "prove_chunk(%zu): shader clock (one workgroup in the middle of each launch): transforms %.0f / %.0f / %.0f MHz, Z kernel %.0f MHz (eight waves, one per XCD: %.0f %.0f %.0f %.0f %.0f %.0f %.0f %.0f); stages %.2f / %.2f / %.2f / %.2f ms\n", ck.n, mhz(8), mhz(9), mhz(10), (double)ln.stat.clock_mhz, mhz(0), mhz(1), mhz(2), mhz(3), mhz(4), mhz(5), mhz(6), mhz(7),
                               ln.stage_ms[0], ln.stage_ms[1], ln.stage_ms[2], ln.stage_ms[3]);
}

void AlgorithmImpl::prove_chunk(Lane& ln, const ProofRequest* reqs, size_t n, ProofResult* results, DebugVectors* dbg, bool allow_few_solver, bool allow_small) {
    Chunk ck{reqs, n, (n + 63) / 64 * 64, dbg, {}, std::chrono::steady_clock::now(), {}, {}};
    const size_t B = ck.B;
    ln.n_real = n;
    // staging is the lane's pinned memory; what it holds of the statements' secrets (keys, randomness, masks) is cleared when the call leaves, however it leaves
    struct StagingWiper { Lane& l; size_t B; ~StagingWiper() { explicit_bzero(l.h_in.p, 176 * B); explicit_bzero(l.h_rs.p, 64 * B); explicit_bzero(l.h_glv.p, l.h_glv.bytes()); if (l.h_mask.p) explicit_bzero(l.h_mask.p, 32 * B); } } wipe_staging{ln, B};
    // a call that leaves by an exception must not leave work behind on the lane's other streams (the next call would share its buffers with it)
    // ... nor anything key-derived in its buffers: how far the call got is not tracked, so every secret region is cleared over its whole allocation
    struct Drain {
        AlgorithmImpl& a; Lane& l; int live = std::uncaught_exceptions();
        void sync() { (void)hipStreamSynchronize(l.side); (void)hipStreamSynchronize(l.side2); (void)hipStreamSynchronize(l.stream); }
        ~Drain() {
            if (std::uncaught_exceptions() <= live) return;
            sync();
            l.wipe_a_pending = false; l.pending1.n = 0; l.pending2.n = 0;
            if (a.cfg.keep_secrets || !a.cfg.wipe_full) return;
            try { a.wipe_whole(l, l.stream); } catch (const std::exception& e) { fprintf(stderr, "libprove: could not clear the lane after a failed call: %s\n", e.what()); }
            sync();
        }
    } drain{*this, ln};
    // the route, decided here and nowhere else (chunk_route.hpp)
    RouteCall call{dbg != nullptr, allow_few_solver, allow_small, false};
    ck.rt = chunk_route(n, cfg, route_facts(), call);
    if (ck.rt.resident) {      // a recent give-up on this replica: skip the resident kernel for a while (see few_skip)
        uint32_t k = few_skip.load();
        while (k && !few_skip.compare_exchange_weak(k, k - 1)) {}
        if (k) { call.skip_resident = true; ck.rt = chunk_route(n, cfg, route_facts(), call); }
    }
    ln.small_active = ck.rt.small;
    ck.check = check_now();      // the key loaded now checks this chunk, whatever is loaded while it runs
    if (corrupt) ck.corrupt = corrupt->exchange(0);
    stage_upload(ln, ck); fail_after(1);
    stage_witness(ln, ck); fail_after(2);
    stage_early_sums(ln, ck); fail_after(3);
    stage_quotient(ln, ck); fail_after(4);
    stage_msms(ln, ck); fail_after(5);
    stage_assembly(ln, ck);
    if (ln.h_fsync()[1]) {      // the resident solver gave up (its workgroups never became resident together: another process's kernel on this device)
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true)) fprintf(stderr, "libprove: the resident witness kernel could not hold the device (shared with another process?); solving level by level\n");
        const uint32_t pen = few_penalty.load();
        few_skip.store(pen); few_penalty.store(pen < 4096 ? pen * 2 : 4096);
        if (ck.corrupt) corrupt->store(ck.corrupt);      // (the chunk is proved again: the armed change is for the attempt that counts)
        return prove_chunk(ln, reqs, n, results, dbg, false, allow_small);
    }
    if (ln.h_wsflag()) {      // a value did not fit the byte plane it was predicted for: the whole chunk again with the generic solver (results never depend on predictions)
        small_fallbacks++;
        if (ck.corrupt) corrupt->store(ck.corrupt);
        return prove_chunk(ln, reqs, n, results, dbg, allow_few_solver, false);
    }
    if (ck.rt.resident) few_penalty.store(16);
    stage_stat(ln, ck);
    const uint8_t* const h_cpts = ln.h_cpts.p;
    for (size_t i = 0; i < n; i++)
        serialize(ln.h_out.p + 256 * i, ln.h_flags.p[i], ln.h_status.p[i], has_commitment ? h_cpts + 64 * i : nullptr, has_commitment ? h_cpts + 64 * B + 64 * i : nullptr, results[i], !ck.check || ck.verdict[i] != 0);
    if (cfg.trace_host) trace_chunk(ln, ck);
}

void AlgorithmImpl::serialize(const uint8_t* o, uint8_t flags, uint32_t status, const uint8_t* commitment_xy, const uint8_t* pok_xy, ProofResult& res, bool released) const {
    res.proof_len = 0; res.status = 0;
    if (status != 0xFFFFFFFFu) { res.status = 1; return; }
    if (flags) { res.status = 2; return; }
    if (!released) { res.status = 3; return; }
    uint8_t* p = res.proof;
    auto g1 = [&](const uint8_t* xy, uint8_t* dst) {
        uint8_t y[32]; le_limbs_to_be(xy, dst); le_limbs_to_be(xy + 32, y);
        dst[0] |= be_greater(y, kHalfP) ? 0xC0 : 0x80;
    };
    g1(o, p);
    {   // G2: X.A1 | X.A0, flag from y (A1 unless zero, then A0)
        uint8_t y0[32], y1[32];
        le_limbs_to_be(o + 96, p + 32); le_limbs_to_be(o + 64, p + 64);
        le_limbs_to_be(o + 128, y0); le_limbs_to_be(o + 160, y1);
        const bool large = be_is_zero(y1) ? be_greater(y0, kHalfP) : be_greater(y1, kHalfP);
        p[32] |= large ? 0xC0 : 0x80;
    }
    g1(o + 192, p + 96);
    if (!commitment_xy) {
        p[128] = p[129] = p[130] = p[131] = 0;          // no commitments (ChaCha20-V3)
        memset(p + 132, 0, 32); p[132] = 0x40;          // CommitmentPok = point at infinity
        res.proof_len = 164;
    } else {                                            // one commitment + its proof of knowledge (AES-V2)
        p[128] = p[129] = p[130] = 0; p[131] = 1;
        auto g1be = [&](const uint8_t* xy, uint8_t* dst) { memcpy(dst, xy, 32); dst[0] |= be_greater(xy + 32, kHalfP) ? 0xC0 : 0x80; };
        g1be(commitment_xy, p + 132); g1be(pok_xy, p + 164);
        res.proof_len = 196;
    }
}
}  // namespace gsc
