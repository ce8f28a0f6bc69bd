// See solver_tables.hpp: the witness solver's tables and launch sequences, one copy for the engine and for the test hook gsc_debug_solve.
#include "solver_tables.hpp"
#include <cstring>

namespace gsc {

namespace {
// Montgomery images of 0, 1, 2, -1, -2 in Fr: gnark puts these at coefficient ids 0..4 of every R1CS
// (SURVEY.md App. A); the solver kernel short-cuts them to additions.
const uint32_t kSmallCoeffs[5][8] = {
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u},
    {0x9ffffff6u, 0x592c6838u, 0x3ec19a53u, 0x6df8ed2bu, 0xf0f28c5cu, 0xccdd46deu, 0x340fbe5eu, 0x1c14ef83u},
    {0xa0000006u, 0x974bc177u, 0xda58a367u, 0xf13771b2u, 0x0908122eu, 0x51e1a247u, 0x4729c0fau, 0x2259d6b1u},
    {0x5000000bu, 0xeab58d5bu, 0x3af7d63du, 0xba3afb1du, 0x908ecc00u, 0xeb72fed7u, 0xad21e1cau, 0x144f5eefu},
};
}  // namespace

std::unique_ptr<SolverProgram> SolverTables::build_tables(const R1csFile& cs, hipStream_t stream) {
    n_wires = cs.n_wires(); n_public = cs.n_public; n_inputs = cs.n_public + cs.n_secret; n_constraints = cs.n_constraints; has_commitment = cs.has_commitment;
    if (cs.n_coeff() < 5 || memcmp(cs.coeff_limbs.data(), kSmallCoeffs, sizeof kSmallCoeffs)) throw std::runtime_error("r1cs: coefficient ids 0..4 are not 0,1,2,-1,-2");
    std::unique_ptr<SolverProgram> keep(new SolverProgram(build_solver_program(cs)));
    const SolverProgram& sp = *keep;
    n_levels = (uint32_t)sp.n_levels; commit_level = (uint32_t)sp.commit_level; has_div = sp.n_inversions ? 1 : 0;
    level_width.resize(n_levels); for (uint32_t l = 0; l < n_levels; l++) level_width[l] = sp.sched[2 + l] - sp.sched[1 + l];
    level_kind = sp.level_kind; level_long = sp.level_long;
    prog.alloc(sp.words.size()); prog.upload(sp.words.data(), sp.words.size(), stream);
    sched.alloc(sp.sched.size()); sched.upload(sp.sched.data(), sp.sched.size(), stream);
    {
        const FewProgram fp = build_few_program(sp);
        few_ops.alloc(fp.ops.size() ? fp.ops.size() : 8); few_terms.alloc(fp.terms.size()); few_lstart.alloc(fp.level_start.size());
        if (!fp.ops.empty()) few_ops.upload(fp.ops.data(), fp.ops.size(), stream);
        few_terms.upload(fp.terms.data(), fp.terms.size(), stream); few_lstart.upload(fp.level_start.data(), fp.level_start.size(), stream);
        few_count_first = fp.count_first;
        few_count_ops.alloc(fp.count_ops.size() + 4); few_count_qoff.alloc(fp.count_qoff.size() + 1);
        if (!fp.count_ops.empty()) { few_count_ops.upload(fp.count_ops.data(), fp.count_ops.size(), stream); few_count_qoff.upload(fp.count_qoff.data(), fp.count_qoff.size(), stream); }
    }
    lookup_coeff.alloc(sp.lookup_coeff.size() ? sp.lookup_coeff.size() : 1);
    if (!sp.lookup_coeff.empty()) lookup_coeff.upload(sp.lookup_coeff.data(), sp.lookup_coeff.size(), stream);
    coeff.alloc(cs.n_coeff()); coeff_inv.alloc(cs.n_coeff());
    HIP_CHECK(hipMemcpyAsync(coeff.p, cs.coeff_limbs.data(), cs.coeff_limbs.size() * 4, hipMemcpyHostToDevice, stream));
    launch_fr_inverse(coeff.p, coeff_inv.p, cs.n_coeff(), stream);
    if (!sp.count_ops.empty()) {      // lookup histograms rely on table row i carrying index i: verify once, on the device
        DevBuf<uint32_t> d_ops(sp.count_ops.size()), d_flag(1); uint32_t flag = 0;
        d_ops.upload(sp.count_ops.data(), sp.count_ops.size(), stream);
        HIP_CHECK(hipMemsetAsync(d_flag.p, 0, 4, stream));
        launch_check_count_tables(prog.p, coeff.p, d_ops.p, (uint32_t)sp.count_ops.size(), d_flag.p, stream);
        HIP_CHECK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        if (flag) throw std::runtime_error("r1cs: unsupported lookup table (index column is not 0..n-1)");
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    return keep;
}

// The small-integer witness program (wit_small.hpp), when the circuit qualifies: coefficients as integers (from the device: no field
// arithmetic on the host), the classes of wires and constraint rows, the item lists uploaded once.
void SolverTables::build_small_tables(const SolverProgram& sp, const std::vector<uint8_t>& class_w, const std::vector<uint8_t>& class_a, const std::vector<uint8_t>& class_b,
                                      const std::vector<uint8_t>& class_c, hipStream_t stream) {
    const size_t nc = coeff.n;
    DevBuf<long long> d_c(nc ? nc : 1); DevBuf<uint8_t> d_ok(nc ? nc : 1);
    std::vector<long long> hc(nc); std::vector<uint8_t> ok(nc);
    launch_coeff_small(coeff.p, nc, d_c.p, d_ok.p, stream);
    HIP_CHECK(hipGetLastError());
    if (nc) { HIP_CHECK(hipMemcpyAsync(hc.data(), d_c.p, nc * 8, hipMemcpyDeviceToHost, stream)); HIP_CHECK(hipMemcpyAsync(ok.data(), d_ok.p, nc, hipMemcpyDeviceToHost, stream)); }
    HIP_CHECK(hipStreamSynchronize(stream));
    std::vector<int64_t> ci(hc.begin(), hc.end());
    small = build_small_program(sp, n_wires, n_constraints, ci, ok, class_w, class_a, class_b, class_c);
    if (!small.ok) return;
    auto up32 = [&](DevBuf<uint32_t>& d, std::vector<uint32_t>& v, size_t pad) { v.resize(v.size() + pad, 0u); d.alloc(v.size()); d.upload(v.data(), v.size(), stream); };
    auto up64 = [&](DevBuf<long long>& d, std::vector<int64_t>& v, size_t pad) { v.resize(v.size() + pad, 0); d.alloc(v.size()); d.upload(reinterpret_cast<const long long*>(v.data()), v.size(), stream); };
    // (the kernels fetch descriptors and terms a whole wave at a time: 128 / 64 words beyond the last item may be read)
    up32(ws_tiny, small.tiny, 128); up32(ws_parts, small.parts, 4); up32(ws_bits, small.bits, 4); up32(ws_twire, small.twire, 64); up64(ws_tcoef, small.tcoef, 64); up32(ws_levels, small.levels, 6);
    up32(ws_rtiny, small.rtiny, 128); up32(ws_rgen, small.rgen, 8); up32(ws_rtwire, small.rtwire, 64); up64(ws_rtcoef, small.rtcoef, 64);
    ws_cls_a.alloc(n_constraints); ws_cls_b.alloc(n_constraints); ws_cls_c.alloc(n_constraints);
    ws_cls_a.upload(small.cls_a.data(), n_constraints, stream); ws_cls_b.upload(small.cls_b.data(), n_constraints, stream); ws_cls_c.upload(small.cls_c.data(), n_constraints, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
}

void solver_run_levels(const SolverTables& t, SolverArgs& sa, SolverWalk& w, uint32_t from, uint32_t to, hipStream_t stream) {
    SolverFewArgs fa{t.few_ops.p, t.few_terms.p, t.few_lstart.p, 0, 0, t.coeff.p, t.coeff_inv.p, t.lookup_coeff.p, sa.W, sa.A, sa.B, sa.C, sa.batch, (uint32_t)w.n,
                     sa.status, sa.mask, sa.commit, w.fsync, 1u << 21, 0u, t.n_levels, nullptr};
    if (w.test_abort) { fa.poll_limit = 256; fa.test_missing = 1; }      // test: the barrier never fills
    for (uint32_t l = from; l < to; l++) {
        sa.first_level = l; sa.n_long = t.level_long[l];
        if (t.level_kind[l]) {
            if (w.resident) launch_solver_count_few(sa, t.few_count_ops.p, t.few_count_qoff.p, t.few_count_first[l], t.level_width[l], w.n, stream);
            else launch_solver_count_level(sa, t.level_width[l], stream);
        } else if (w.resident) {                   // a run of generic levels: one launch, device-wide barriers in between
            uint32_t e = l + 1; while (e < to && !t.level_kind[e]) e++;
            fa.from = l; fa.to = e; fa.trace = sa.trace;
            HIP_CHECK(hipMemsetAsync(w.fsync, 0, 4, stream));
            {
                FewSolverChain& chain = few_solver_chain(w.device);
                std::lock_guard<std::mutex> lk(chain.m);
                if (chain.last && chain.last != w.ev_few) HIP_CHECK(hipStreamWaitEvent(stream, chain.last, 0));
                // measured: 128 workgroups best for 1-2 statements, 256 (one per CU) beyond; never more than the device has CUs
                // (every workgroup must be resident: one per CU by construction) — the kernel works with any grid
                uint32_t wgs = w.workgroups ? w.workgroups : (w.n <= 2 ? 128u : 256u);
                if (wgs > (uint32_t)w.cu_count) wgs = (uint32_t)w.cu_count;
                launch_solver_few(fa, t.has_div, wgs, stream);
                HIP_CHECK(hipEventRecord(w.ev_few, stream));
                chain.last = w.ev_few;
                w.launches++; w.workgroups_used = wgs;
            }
            l = e - 1;
        } else launch_solver_level(sa, t.level_width[l], stream);
    }
}

void solver_run_small(const SolverTables& t, const SmallBuffers& b, size_t B, bool expand, hipStream_t stream) {
    const SmallProgram& small = t.small;
    HIP_CHECK(hipMemsetAsync(b.flag, 0, 4, stream));
    launch_wit_narrow(b.W, B, t.n_inputs, b.W8, small.rows_per_group, b.flag, stream);
    launch_wit_chain(WitChainArgs{t.ws_tiny.p, t.ws_parts.p, t.ws_bits.p, t.ws_twire.p, t.ws_tcoef.p, t.ws_levels.p, small.n_levels, b.W8, small.rows_per_group, b.flag}, B / 64, 512 * (size_t)small.max_slots, stream);
    const uint32_t per_chunk = 4 * WS_IB;
    launch_wit_rows(WitRowsArgs{t.ws_rtiny.p, small.n_rtiny, per_chunk, (small.n_rtiny + per_chunk - 1) / per_chunk, t.ws_rgen.p, small.n_rgen, t.ws_rtwire.p, t.ws_rtcoef.p, b.W8, small.rows_per_group,
                                b.A8, b.B8, b.C8, t.n_constraints, b.A, b.B, b.C, B, b.status, b.flag}, B / 64, stream);
    // The consumers (first transform kernel, flat recoders) read the byte planes; the 32-byte matrices only hold the rows predicted wide.
    if (expand) {      // debug dumps want every row as a 32-byte element
        launch_wit_expand(b.W8, small.rows_per_group, t.n_wires, nullptr, b.W, B, stream);
        launch_wit_expand(b.A8, t.n_constraints, t.n_constraints, t.ws_cls_a.p, b.A, B, stream);
        launch_wit_expand(b.B8, t.n_constraints, t.n_constraints, t.ws_cls_b.p, b.B, B, stream);
        launch_wit_expand(b.C8, t.n_constraints, t.n_constraints, t.ws_cls_c.p, b.C, B, stream);
    }
}

}  // namespace gsc
