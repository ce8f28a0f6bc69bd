// TEST HOOK gsc_debug_solve (include/libprove.h): the witness solver kernels on a caller's constraint system, without a key or an algorithm.
// The R1csFile is put together from the caller's fields as parse_r1cs would have; everything after that is the engine's own code: SolverTables'
// build_tables / build_small_tables (solver_tables.hip) for the tables, solver_run_levels / solver_run_small for the launches — the resident ones in the
// device's few_solver_chain.  No kernel is changed or copied for it.  tests/test_gpu_solver.py is the caller.
#include "solver_debug.hpp"
#include "engine_impl.hpp"
#include <cstdio>

namespace gsc {

namespace {

[[noreturn]] void refuse(const std::string& why) { throw std::runtime_error("gsc_debug_solve: " + why); }
struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };

R1csFile describe(const gsc_debug_solve_args& a) {
    if (a.batch == 0 || a.batch % 64 || a.batch > 4096) refuse("the batch is a multiple of 64 up to 4096");
    if (a.nproofs > MSM_FEW_PROOFS) refuse("nproofs beyond the resident kernels' 32");
    if (a.nproofs && a.batch != 64) refuse("the resident path takes a batch of 64");
    if (a.mode != 0 && a.mode != 1) refuse("no such mode");
    if (a.mode == 1 && (a.nproofs || !a.class_w || !a.class_a || !a.class_b || !a.class_c)) refuse("the small-integer path takes whole batches and the four class predictions");
    if (a.workgroups > 256) refuse("more than 256 workgroups");
    if (!a.n_public || (size_t)a.n_public + a.n_secret + a.n_internal > (1u << 20) || a.n_constraints > (1u << 20)) refuse("no constant wire, or more than 2^20 wires / constraints");
    if (!a.calldata || !a.blueprint || !a.constraint_off || !a.wire_off || !a.bp_kind || !a.bp_entries_len || !a.coeff || !a.in_W) refuse("a part of the description is missing");
    if (!a.W || !a.A || !a.B || !a.C || !a.status || !a.flag || !a.info || !a.why) refuse("no room for the results");
    R1csFile cs;
    cs.n_public = a.n_public; cs.n_secret = a.n_secret; cs.n_internal = a.n_internal; cs.n_constraints = a.n_constraints;
    cs.calldata.assign(a.calldata, a.calldata + a.n_calldata);
    for (size_t q = 0; q < a.n_calldata;) {      // instruction i's first word is its own length (parse_r1cs)
        const uint32_t l = cs.calldata[q];
        if (l == 0 || q + l > a.n_calldata) refuse("corrupt instruction length");
        cs.instr_start.push_back(q); q += l;
    }
    cs.instr_start.push_back(a.n_calldata);
    if (cs.instr_start.size() - 1 != a.n_instr) refuse("instruction table size mismatch");
    cs.blueprint.assign(a.blueprint, a.blueprint + a.n_instr); cs.constraint_off.assign(a.constraint_off, a.constraint_off + a.n_instr); cs.wire_off.assign(a.wire_off, a.wire_off + a.n_instr);
    size_t at = 0;
    for (uint32_t b = 0; b < a.n_blueprints; b++) {
        if (a.bp_kind[b] > BP_LOOKUP) refuse("no such blueprint kind");
        cs.bp_kind.push_back((BlueprintKind)a.bp_kind[b]);
        if (a.bp_entries_len[b] > 4096 || (a.bp_entries_len[b] && !a.bp_entries)) refuse("blueprint entries missing or too long");
        cs.bp_entries.emplace_back(a.bp_entries + at, a.bp_entries + at + a.bp_entries_len[b]);
        at += a.bp_entries_len[b];
    }
    for (uint32_t b : cs.blueprint) if (b >= cs.bp_kind.size()) refuse("blueprint id out of range");
    if (a.n_coeff > (1u << 20)) refuse("more than 2^20 coefficients");
    cs.coeff_limbs.assign(a.coeff, a.coeff + 8 * (size_t)a.n_coeff);
    cs.has_commitment = a.has_commitment != 0; cs.commit_wire = a.commit_wire;
    if (a.n_commit_private && !a.commit_private) refuse("committed wires missing");
    if (a.n_commit_private) cs.commit_private.assign(a.commit_private, a.commit_private + a.n_commit_private);
    const size_t col = (size_t)a.batch * sizeof(fe);
    if (a.W_cap < cs.n_wires() * col || a.A_cap < a.n_constraints * col || a.B_cap < a.n_constraints * col || a.C_cap < a.n_constraints * col) refuse("an output buffer is too small");
    return cs;
}

int run(int device, const gsc_debug_solve_args& a, const R1csFile& cs) {
    uint32_t* info = a.info;
    for (int i = 0; i < 32; i++) info[i] = 0;
    memset(a.why, 0, 128); *a.flag = 0;
    int cus = 256;
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0) cus = v; }
    hipStream_t s = stream_take(device, STREAM_PLAIN, STREAM_ROLE_INIT);
    struct StreamGuard { hipStream_t s; int device; ~StreamGuard() { stream_give(device, STREAM_PLAIN, STREAM_ROLE_INIT, s); } } stream_guard{s, device};
    SolverTables t;
    std::unique_ptr<SolverProgram> sp;
    try { sp = t.build_tables(cs, s); }
    catch (const std::runtime_error& e) {      // the builders' refusals are the caller's; a HIP error is the device's
        snprintf(a.why, 128, "%s", e.what());
        if (!strncmp(e.what(), "HIP error", 9)) throw DeviceError(e.what());
        throw;
    }
    info[0] = t.n_levels; info[1] = t.commit_level; info[2] = (uint32_t)t.has_div; info[3] = (uint32_t)sp->n_ops;
    for (uint32_t l = 0; l < t.n_levels; l++) {
        if (t.level_long[l]) { info[9]++; if (t.level_long[l] > info[11]) info[11] = t.level_long[l]; }
        if (t.level_kind[l]) info[10]++;
        if (l < 18) info[14 + l] = (uint32_t)t.level_kind[l] | (t.level_long[l] << 1) | (t.level_width[l] << 12);
    }
    if (a.mode == 1) {
        t.build_small_tables(*sp, std::vector<uint8_t>(a.class_w, a.class_w + t.n_wires), std::vector<uint8_t>(a.class_a, a.class_a + t.n_constraints),
                             std::vector<uint8_t>(a.class_b, a.class_b + t.n_constraints), std::vector<uint8_t>(a.class_c, a.class_c + t.n_constraints), s);
        info[8] = t.small.ok ? 1u : 0u;
        snprintf(a.why, 128, "%s", t.small.why.c_str());
        if (!t.small.ok) return -2;
        info[12] = t.small.n_levels;
        for (uint32_t l = 0; l < t.small.n_levels; l++) { const uint32_t b = (t.small.levels[6 * l + 1] - t.small.levels[6 * l]) / WS_IB; if (b > info[13]) info[13] = b; }
    }
    const size_t B = a.batch, nw = t.n_wires, nc = t.n_constraints;
    DevBuf<fe> d_W(nw * B), d_A(nc ? nc * B : 1), d_B(nc ? nc * B : 1), d_C(nc ? nc * B : 1), d_mask(B), d_commit(B);
    DevBuf<uint32_t> d_status(B), d_fsync(2), d_flag(1);
    const int fill = (int)(a.fill & 0xFF);
    HIP_CHECK(hipMemsetAsync(d_W.p, fill, d_W.bytes(), s)); HIP_CHECK(hipMemsetAsync(d_A.p, fill, d_A.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_B.p, fill, d_B.bytes(), s)); HIP_CHECK(hipMemsetAsync(d_C.p, fill, d_C.bytes(), s));
    HIP_CHECK(hipMemcpyAsync(d_W.p, a.in_W, t.n_inputs * B * sizeof(fe), hipMemcpyHostToDevice, s));
    if (a.mask) HIP_CHECK(hipMemcpyAsync(d_mask.p, a.mask, B * sizeof(fe), hipMemcpyHostToDevice, s));
    if (a.commit) HIP_CHECK(hipMemcpyAsync(d_commit.p, a.commit, B * sizeof(fe), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_status.p, 0xFF, B * 4, s));
    HIP_CHECK(hipMemsetAsync(d_fsync.p, 0, 8, s)); HIP_CHECK(hipMemsetAsync(d_flag.p, 0, 4, s));
    if (a.mode == 1) {
        // byte planes as a lane holds them: zero, the rows predicted wide marked for good (alloc_lane)
        DevBuf<int8_t> d_W8((size_t)t.small.rows_per_group * B), d_A8(nc ? nc * B : 1), d_B8(nc ? nc * B : 1), d_C8(nc ? nc * B : 1);
        HIP_CHECK(hipMemsetAsync(d_W8.p, 0, d_W8.bytes(), s)); HIP_CHECK(hipMemsetAsync(d_A8.p, 0, d_A8.bytes(), s));
        HIP_CHECK(hipMemsetAsync(d_B8.p, 0, d_B8.bytes(), s)); HIP_CHECK(hipMemsetAsync(d_C8.p, 0, d_C8.bytes(), s));
        launch_wit_mark_wide(d_A8.p, nc, nc, t.ws_cls_a.p, B, s); launch_wit_mark_wide(d_B8.p, nc, nc, t.ws_cls_b.p, B, s); launch_wit_mark_wide(d_C8.p, nc, nc, t.ws_cls_c.p, B, s);
        solver_run_small(t, SmallBuffers{d_W.p, d_A.p, d_B.p, d_C.p, d_W8.p, d_A8.p, d_B8.p, d_C8.p, d_status.p, d_flag.p}, B, true, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    } else {
        SolverArgs sa{t.prog.p, t.sched.p, 0, t.n_levels, t.coeff.p, t.coeff_inv.p, t.lookup_coeff.p, d_W.p, d_A.p, d_B.p, d_C.p, B, d_status.p,
                      a.mask ? d_mask.p : nullptr, a.commit ? d_commit.p : nullptr, t.has_div, 0u, nullptr};
        SolverWalk walk;
        walk.n = a.nproofs ? a.nproofs : B; walk.resident = a.nproofs != 0; walk.workgroups = a.workgroups; walk.cu_count = cus; walk.device = device; walk.fsync = d_fsync.p;
        struct EventGuard {      // the completion event leaves the device's chain before it is destroyed (Lane's destructor does the same)
            hipEvent_t ev = nullptr; int device;
            ~EventGuard() { if (!ev) return; (void)hipEventSynchronize(ev); FewSolverChain& c = few_solver_chain(device); { std::lock_guard<std::mutex> lk(c.m); if (c.last == ev) c.last = nullptr; } (void)hipEventDestroy(ev); }
        } evg{nullptr, device};
        HIP_CHECK(hipEventCreateWithFlags(&evg.ev, hipEventDisableTiming));
        walk.ev_few = evg.ev;
        // a circuit with a commitment is solved in two walks around the commitment's level, as stage_witness does (the challenge is the caller's here)
        if (t.has_commitment) { solver_run_levels(t, sa, walk, 0, t.commit_level, s); solver_run_levels(t, sa, walk, t.commit_level, t.n_levels, s); }
        else solver_run_levels(t, sa, walk, 0, t.n_levels, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        if (!walk.resident) info[4] = solver_level_wpb(B);
        info[5] = walk.workgroups_used; info[6] = walk.launches;
        uint32_t fs[2] = {0, 0};
        HIP_CHECK(hipMemcpy(fs, d_fsync.p, 8, hipMemcpyDeviceToHost));
        info[7] = fs[1] ? 1u : 0u;
    }
    HIP_CHECK(hipMemcpy(a.W, d_W.p, nw * B * sizeof(fe), hipMemcpyDeviceToHost));
    if (nc) { HIP_CHECK(hipMemcpy(a.A, d_A.p, nc * B * sizeof(fe), hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(a.B, d_B.p, nc * B * sizeof(fe), hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(a.C, d_C.p, nc * B * sizeof(fe), hipMemcpyDeviceToHost)); }
    HIP_CHECK(hipMemcpy(a.status, d_status.p, B * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(a.flag, d_flag.p, 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

int debug_solve(int device, const gsc_debug_solve_args& a) {
    const R1csFile cs = describe(a);      // every refusal the host can decide without the builders comes before a device is asked for
    try {
        use_device(device);
        return run(device, a, cs);
    } catch (const DeviceError& e) { printf("gsc_debug_solve: %s\n", e.what()); return -3; }
    catch (const std::runtime_error& e) {
        if (!strncmp(e.what(), "HIP error", 9)) { printf("gsc_debug_solve: %s\n", e.what()); return -3; }
        throw;
    }
}

}  // namespace gsc
