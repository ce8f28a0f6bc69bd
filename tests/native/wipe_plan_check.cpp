// The wipe plan of the prover (csrc/wipe_plan.hpp) on the CPU, for every route chunk_route can return: what a chunk wrote and which stage reads what
// are written out here by hand from the stage functions of engine_prove.hip, never by asking the plan.  Built and run by tests/test_wipe_plan_host.py;
// prints WIPE-PLAN-OK when every case holds.
#include "../../gnark-symmetric-crypto_amd/csrc/wipe_plan.hpp"
#include <cstdio>
#include <set>
#include <string>
#include <vector>

using namespace gsc;

namespace {
// a made-up circuit and lane: 256 columns of capacity
const uint64_t NW = 1000, NC = 300, DOM = 512, RPG = 1100, CAP = 256, X1 = 128, X2 = 256;
int bad = 0;
std::string what;
void fail(const std::string& msg) { printf("FAIL %s: %s\n", what.c_str(), msg.c_str()); bad++; }

WipeSizes sizes(uint64_t B, uint64_t n) {
    WipeSizes z; z.B = B; z.n = n; z.n_wires = NW; z.n_constraints = NC; z.domain_n = DOM; z.rows_per_group = RPG; z.fe_bytes = 32; z.xyzz1_bytes = X1; z.xyzz2_bytes = X2;
    z.part1a = 700 * B * X1; z.part1b = 40 * B * X1; z.part2a = 90 * B * X2; z.part2b = 8 * B * X2; z.digits = 4111 * B * 16; z.digits_w = 333 * B * 16 + 16; z.gok = 3 * B + 7; z.sj2 = 17 * B * X2;
    for (int k = 0; k < 8; k++) z.sj1[k] = (k % 3 ? 17 : 0) * B * X1 + X1;
    return z;
}
std::vector<WipeRegionInfo> lane_table(const RouteFacts& f) {
    const WipeSizes z = sizes(CAP, CAP);
    std::vector<WipeRegionInfo> t;
    auto add = [&](int r, uint64_t bytes) { t.push_back(WipeRegionInfo{r, bytes}); };
    add(WR_INPUTS, 176 * CAP); add(WR_RS, 64 * CAP); add(WR_GLV, 2 * 32 * 44);
    add(WR_W, (NW + 4) * CAP * 32); add(WR_A, DOM * CAP * 32); add(WR_B, DOM * CAP * 32); add(WR_C, (DOM + 1) * CAP * 32);
    if (f.small_ok) { add(WR_W8, RPG * CAP); add(WR_A8, NC * CAP); add(WR_B8, NC * CAP); add(WR_C8, NC * CAP); add(WR_WSFLAG, 4); }
    if (f.has_commitment) { add(WR_MASK_IN, 32 * CAP); add(WR_MASK, 32 * CAP); add(WR_COMMIT, 32 * CAP); add(WR_SUM_D, CAP * X1); add(WR_SUM_POK, CAP * X1); add(WR_CPTS, 128 * CAP); }
    add(WR_PART1A, z.part1a); add(WR_PART1B, z.part1b); add(WR_PART2A, z.part2a); add(WR_PART2B, z.part2b); add(WR_PART1C, 9 * 64 * X1); add(WR_PART1D, 2 * 64 * X1);
    add(WR_DIGITS, z.digits); if (f.fuse_z_digits) add(WR_DIGITS_W, z.digits_w);
    add(WR_DIGITS_S, 5000); add(WR_DIGITS_S2, 6001); add(WR_GOK, z.gok); add(WR_GOK_S, 77); add(WR_GOK_S2, 78);
    for (int k = 0; k < 8; k++) { add(WR_SJ1 + k, z.sj1[k]); add(WR_FLAT1 + k, k % 2 ? CAP * X1 : X1); }
    add(WR_SJ2, z.sj2); add(WR_FLAT2, CAP * X2);
    for (int r : {WR_SUM_A, WR_SUM_B1, WR_SUM_K, WR_SUM_Z, WR_SUM_C}) add(r, CAP * X1);
    add(WR_SUM_B2, CAP * X2); add(WR_TMP, 2 * CAP * X1);
    add(WR_OUT, 256 * CAP); add(WR_FLAGS, CAP); add(WR_STATUS, 4 * CAP); add(WR_CLK, 48 * 8); add(WR_FSYNC, 8);
    return t;
}
uint64_t alloc_bytes(const std::vector<WipeRegionInfo>& t, int r) { for (auto& e : t) if (e.region == r) return e.bytes; return 0; }

bool covered(const WipePlan& p, int region, uint64_t off) {
    for (const auto* v : {&p.a, &p.b}) for (const WipeItem& it : *v) {
        if (it.region != region || off < it.offset || !it.rows || !it.width) continue;
        const uint64_t rel = off - it.offset, row = it.pitch ? rel / it.pitch : 0, col = it.pitch ? rel % it.pitch : rel;
        if (row < it.rows && col < it.width) return true;
    }
    return false;
}
// every sampled byte of rows x width (rows `pitch` apart, from 0) lies in some descriptor of either phase
void want_rows(const WipePlan& p, const std::vector<WipeRegionInfo>& t, int region, uint64_t rows, uint64_t pitch, uint64_t width) {
    if (!alloc_bytes(t, region) || !rows || !width) return;
    for (uint64_t row : {(uint64_t)0, rows / 2, rows - 1}) for (uint64_t col : {(uint64_t)0, width / 2, width - 1}) {
        const uint64_t off = row * pitch + col;
        if (off >= alloc_bytes(t, region)) continue;      // (a need clamped by the allocation)
        if (!covered(p, region, off)) fail(std::string(wipe_region_name(region)) + ": written byte " + std::to_string(off) + " is in no phase");
    }
}
void want_prefix(const WipePlan& p, const std::vector<WipeRegionInfo>& t, int region, uint64_t bytes) { want_rows(p, t, region, 1, bytes, bytes); }

void check(const EngineConfig& cfg, const RouteFacts& f, const RouteCall& call, uint64_t B, uint64_t n) {
    const ChunkRoute rt = chunk_route(n, cfg, f, call);
    const std::vector<WipeRegionInfo> t = lane_table(f);
    const WipeSizes z = sizes(B, n);
    const WipePlan p = wipe_plan(rt, f, z, t);
    // 1. the union of the phases covers what the stages of this route write (engine_prove.hip)
    want_prefix(p, t, WR_INPUTS, 176 * B); want_prefix(p, t, WR_RS, 64 * B);                      // stage_upload
    want_prefix(p, t, WR_W, (NW + 4) * B * 32);                                                   // k_assign_*, k_prep_rs and every solver: whole rows (the padding columns too)
    const bool own_columns = rt.latency && rt.resident;      // k_solver_few writes a, b, c for the statements' columns, the latency transforms touch no others
    for (int r : {WR_A, WR_B, WR_C}) {
        const uint64_t rows = r == WR_C ? DOM + 1 : DOM;
        if (own_columns) want_rows(p, t, r, rows, B * 32, n * 32); else want_prefix(p, t, r, rows * B * 32);
    }
    if (rt.small) { want_prefix(p, t, WR_W8, RPG * B); for (int r : {WR_A8, WR_B8, WR_C8}) want_prefix(p, t, r, NC * B); }      // solve_small
    // run_msm: recoders, verdicts.  Every set but the batch layout of Z recodes into digits_w where it exists (run_msm_g1), and a latency call over the latency layout of Z walks no other
    if (!(rt.latency && rt.use_zfew && f.fuse_z_digits)) want_prefix(p, t, WR_DIGITS, z.digits);
    want_prefix(p, t, WR_DIGITS_W, z.digits_w); want_prefix(p, t, WR_GOK, z.gok);
    want_prefix(p, t, WR_PART1A, z.part1a); want_prefix(p, t, WR_PART1B, z.part1b); want_prefix(p, t, WR_PART2A, z.part2a); want_prefix(p, t, WR_PART2B, z.part2b);
    for (int k = 0; k < 8; k++) { want_prefix(p, t, WR_SJ1 + k, z.sj1[k]); want_prefix(p, t, WR_FLAT1 + k, B * X1); }
    want_prefix(p, t, WR_SJ2, z.sj2); want_prefix(p, t, WR_FLAT2, B * X2);
    for (int r : {WR_SUM_A, WR_SUM_B1, WR_SUM_K, WR_SUM_Z, WR_SUM_C}) want_prefix(p, t, r, B * X1);
    want_prefix(p, t, WR_SUM_B2, B * X2); want_prefix(p, t, WR_TMP, 2 * B * X1);
    if (f.has_commitment) { want_prefix(p, t, WR_MASK_IN, 32 * B); want_prefix(p, t, WR_MASK, 32 * B); want_prefix(p, t, WR_COMMIT, 32 * B); want_prefix(p, t, WR_SUM_D, B * X1); want_prefix(p, t, WR_SUM_POK, B * X1); }
    if (rt.latency) for (int r : {WR_GLV, WR_PART1C, WR_PART1D, WR_DIGITS_S, WR_DIGITS_S2, WR_GOK_S, WR_GOK_S2}) want_prefix(p, t, r, alloc_bytes(t, r));      // stage_upload's split, the side streams' MSMs
    // 2. nothing in phase A that a stage behind its trigger still reads or writes.  Behind the trigger (stage_msms from the Z sum on, stage_assembly):
    //    the Z sum reads its digits — or, unless the last quotient kernel wrote them, d / h in A, recoding into WR_DIGITS — and writes partial sums, per-window sums;
    //    with a commitment the sigma sum reads W once more and recodes into the wire sets' digit buffer; the Horner passes read per-window and flat sums;
    //    the scalar multiplications and k_fin_combine read the sums, rs, tmp.
    std::set<int> late = {WR_DIGITS, WR_GOK, WR_PART1A, WR_PART1B, WR_PART2A, WR_PART2B, WR_SJ2, WR_FLAT2, WR_SUM_A, WR_SUM_B1, WR_SUM_K, WR_SUM_Z, WR_SUM_C, WR_SUM_B2, WR_TMP, WR_RS, WR_SUM_POK};
    for (int k = 0; k < 8; k++) { late.insert(WR_SJ1 + k); late.insert(WR_FLAT1 + k); }
    if (!rt.z_digits_ready) late.insert(WR_A);
    if (f.has_commitment) { late.insert(WR_W); late.insert(WR_W8); late.insert(WR_DIGITS_W); }
    for (const WipeItem& it : p.a) if (late.count(it.region)) fail(std::string("phase A holds ") + wipe_region_name(it.region) + ", which a later stage touches");
    if (rt.latency && !p.a.empty()) fail("a latency call has a phase A");
    // ... and the big ones ARE there when nothing holds them back (or the schedule hides nothing)
    if (!rt.latency) {
        std::set<int> in_a; for (const WipeItem& it : p.a) in_a.insert(it.region);
        for (int r : {WR_B, WR_C}) if (!in_a.count(r)) fail(std::string(wipe_region_name(r)) + " is not in phase A of a batch call");
        if (in_a.count(WR_A) != (rt.z_digits_ready ? 1u : 0u)) fail("A is in phase A exactly when the quotient wrote the Z digits itself");
        if (in_a.count(WR_W) != (f.has_commitment ? 0u : 1u)) fail("W is in phase A exactly when there is no commitment");
    }
    // 3. planes only as images by row class; 4. no public region; and everything inside its allocation
    for (const auto* v : {&p.a, &p.b}) for (const WipeItem& it : *v) {
        if (wipe_region_public(it.region)) fail(std::string("public region ") + wipe_region_name(it.region) + " in the plan");
        if (it.region == WR_A8 || it.region == WR_B8 || it.region == WR_C8) { if (!it.image || it.image_period != NC || it.pitch != 64 || it.width != 64 || it.offset) fail("a marked plane is wiped with zeros, not with its image"); }
        else if (it.image) fail(std::string("image wipe of ") + wipe_region_name(it.region));
        if (!it.rows || !it.width || (it.rows > 1 && it.pitch < it.width) || it.offset + (it.rows - 1) * it.pitch + it.width > alloc_bytes(t, it.region)) fail(std::string(wipe_region_name(it.region)) + ": descriptor outside the allocation");
    }
}
}  // namespace

int main() {
    // the closed public list, and names for all
    {
        what = "region list";
        std::string pub;
        for (int r = 0; r < WR_COUNT; r++) { if (wipe_region_public(r)) pub += std::string(wipe_region_name(r)) + ","; if (std::string(wipe_region_name(r)) == "?") fail("a region without a name"); }
        if (pub != "out,flags,status,cpts,clk,fsync,wsflag,") fail("public regions are " + pub);
    }
    size_t cases = 0; std::set<std::string> routes;
    for (int circuit = 0; circuit < 2; circuit++)            // ChaCha20-V3 (small-integer witness, no commitment) / AES-V2 (generic, one commitment)
    for (int form = 0; form < 3; form++)                     // coefficient form / evaluation form, digits recoded / evaluation form, digits fused
    for (int zfew = 0; zfew < 2; zfew++)
    for (int flat = 0; flat < 2; flat++)                     // the wire sets' latency layouts
    for (int few_path = 0; few_path < 2; few_path++)
    for (int few_solver = 0; few_solver < 2; few_solver++)
    for (int swf = 0; swf < 2; swf++)
    for (int overlap = 0; overlap < 3; overlap++)
    for (int callkind = 0; callkind < 4; callkind++)         // first attempt / after a failed prediction / after the resident solver gave up / debug vectors
    for (uint64_t B : {64, 128, 256}) for (uint64_t n : {(uint64_t)1, (uint64_t)5, (uint64_t)64, B - 3}) {
        if (n > B) continue;
        EngineConfig cfg; cfg.few_max = circuit ? 20 : 32; cfg.few_path = few_path; cfg.few_solver = few_solver; cfg.small_witness_few = swf; cfg.overlap_quotient = overlap;
        RouteFacts f; f.small_ok = circuit == 0; f.has_commitment = circuit == 1; f.quotient_eval = form > 0; f.fuse_z_digits = form == 2; f.zfew_flat = zfew; f.a_flat = f.b1_flat = f.b2_flat = flat;
        RouteCall call; call.allow_small = callkind != 1; call.allow_few_solver = callkind != 2; call.dbg = callkind == 3;
        const ChunkRoute rt = chunk_route(n, cfg, f, call);
        char key[64]; snprintf(key, sizeof key, "%d%d%d%d%d%d%d%d%d%d c%d", rt.latency, rt.resident_wanted, rt.small, rt.resident, rt.early_ab, rt.early_b2, rt.use_zfew, rt.eval, rt.z_digits_ready, rt.overlap_q, circuit);
        routes.insert(key);
        what = std::string(key) + " B=" + std::to_string(B) + " n=" + std::to_string(n);
        check(cfg, f, call, B, n); cases++;
    }
    // the whole-allocation plan: every secret region of the table once, whole; planes as images; nothing public
    {
        what = "whole";
        RouteFacts f; f.small_ok = true; f.quotient_eval = f.fuse_z_digits = true;
        const std::vector<WipeRegionInfo> t = lane_table(f);
        const std::vector<WipeItem> w = wipe_plan_whole(t, NC);
        size_t secret = 0; for (auto& e : t) secret += !wipe_region_public(e.region);
        if (w.size() != secret) fail("not one descriptor per secret region");
        for (const WipeItem& it : w) {
            if (wipe_region_public(it.region)) fail("public region in the whole plan");
            if (it.offset || it.rows * it.pitch != alloc_bytes(t, it.region) || it.width != it.pitch) fail(std::string(wipe_region_name(it.region)) + " is not covered whole");
            if (it.image != (it.region == WR_A8 || it.region == WR_B8 || it.region == WR_C8)) fail("image flag of the whole plan");
        }
    }
    if (bad) { printf("WIPE-PLAN-FAILED: %d\n", bad); return 1; }
    printf("WIPE-PLAN-OK %zu cases, %zu distinct routes\n", cases, routes.size());
    return 0;
}
