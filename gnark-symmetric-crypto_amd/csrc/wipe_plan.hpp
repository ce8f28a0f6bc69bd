// What a chunk leaves in a lane's device buffers, and when each of them can be cleared: the regions of a lane (every device allocation
// alloc_lane makes, by name and class), which stage touches which region last on which route, and the descriptors of the wipe phases of
// one chunk.  A pure function of the route (chunk_route.hpp), a few sizes and the lane's region table: no HIP, no state
// (tests/native/wipe_plan_check.cpp checks every route on the CPU).  The kernels that execute the descriptors: k_wipe.hip.
//
// The idle image of a secret region is zero, except the rows of the byte planes A8 / B8 / C8 that launch_wit_mark_wide marked wide: they
// hold WS_PLANE_WIDE (0x80) for good, nothing rewrites them, and a wipe of a plane writes the image by row class instead of zeros.
#pragma once
#include "chunk_route.hpp"
#include <cstdint>
#include <vector>

namespace gsc {

// Every device allocation of a lane.  PUBLIC_REGIONS is closed: results, verdicts and timing words, nothing key-derived that is not published
// anyway.  Everything else is secret: key-derived after a call, back to its idle image when the call leaves.
enum WipeRegion : int {
    WR_INPUTS, WR_RS, WR_GLV, WR_MASK_IN, WR_MASK, WR_COMMIT, WR_SUM_D, WR_SUM_POK,
    WR_W, WR_A, WR_B, WR_C, WR_W8, WR_A8, WR_B8, WR_C8,
    WR_PART1A, WR_PART1B, WR_PART2A, WR_PART2B, WR_PART1C, WR_PART1D,
    WR_DIGITS, WR_DIGITS_W, WR_DIGITS_S, WR_DIGITS_S2, WR_GOK, WR_GOK_S, WR_GOK_S2,
    WR_SJ1, WR_SJ1_LAST = WR_SJ1 + 7, WR_FLAT1, WR_FLAT1_LAST = WR_FLAT1 + 7, WR_SJ2, WR_FLAT2,
    WR_SUM_A, WR_SUM_B1, WR_SUM_K, WR_SUM_Z, WR_SUM_C, WR_SUM_B2, WR_TMP,
    WR_OUT, WR_FLAGS, WR_STATUS, WR_CPTS, WR_CLK, WR_FSYNC, WR_WSFLAG,
    WR_COUNT
};
constexpr int WR_FIRST_PUBLIC = WR_OUT;
inline bool wipe_region_public(int r) { return r >= WR_FIRST_PUBLIC; }
inline const char* wipe_region_name(int r) {
    static const char* const names[WR_COUNT] = {
        "inputs", "rs", "glv", "mask_in", "mask", "commit", "sumD", "sumPok",
        "W", "A", "B", "C", "W8", "A8", "B8", "C8",
        "part1a", "part1b", "part2a", "part2b", "part1c", "part1d",
        "digits", "digits_w", "digits_s", "digits_s2", "gok", "gok_s", "gok_s2",
        "sj1.A", "sj1.B1", "sj1.K", "sj1.Z", "sj1.Ped", "sj1.PedSigma", "sj1.Zfew", "sj1.C",
        "flat1.A", "flat1.B1", "flat1.K", "flat1.Z", "flat1.Ped", "flat1.PedSigma", "flat1.Zfew", "flat1.C", "sj2", "flat2",
        "sumA", "sumB1", "sumK", "sumZ", "sumC", "sumB2", "tmp",
        "out", "flags", "status", "cpts", "clk", "fsync", "wsflag"};
    return r >= 0 && r < WR_COUNT ? names[r] : "?";
}

// The stages of a batch call in the order the lane's main stream runs them.  WS_WIRE_SUMS ends where the wire-set sums (A, B1, B2, K) and
// sum c_i U_i are through and the last quotient kernel has finished: the trigger of phase A.  Behind it only the Z sum, the sum over the
// commitment's sigma bases, the deferred Horner passes and the assembly remain.
enum WipeStage : int { WS_UPLOAD, WS_WITNESS, WS_QUOTIENT, WS_WIRE_SUMS, WS_Z_SUM, WS_POK_SUM, WS_HORNER, WS_ASSEMBLY };
constexpr int WIPE_PHASE_A_TRIGGER = WS_WIRE_SUMS;

// The last stage that reads or writes region r in a batch call on this route (what runs on the side streams is charged to the stage that
// waits for it).  Regions the route does not touch at all answer WS_UPLOAD.
inline int wipe_last_touch(int r, const ChunkRoute& rt, const RouteFacts& f) {
    switch (r) {
    case WR_INPUTS: return WS_WITNESS;                                  // k_assign_*
    case WR_MASK_IN: case WR_MASK: case WR_COMMIT: case WR_SUM_D: return f.has_commitment ? WS_WITNESS : WS_UPLOAD;
    case WR_W: case WR_W8: return f.has_commitment ? WS_POK_SUM : WS_WIRE_SUMS;      // the sigma sum reads the committed wires once more
    case WR_A: return rt.z_digits_ready ? WS_QUOTIENT : WS_Z_SUM;       // d (or h) is the Z sum's scalar vector unless the quotient wrote its digits
    case WR_B: case WR_A8: case WR_B8: return WS_QUOTIENT;
    case WR_C: case WR_C8: return rt.eval ? WS_WIRE_SUMS : WS_QUOTIENT;  // evaluation form: the scalars of sum c_i U_i
    case WR_DIGITS_W: return f.has_commitment ? WS_POK_SUM : WS_WIRE_SUMS;           // (exists with fused digits only: the Z sum then reads WR_DIGITS)
    case WR_DIGITS: case WR_PART1A: case WR_PART1B: case WR_GOK: return f.has_commitment ? WS_POK_SUM : WS_Z_SUM;
    case WR_PART2A: case WR_PART2B: case WR_SJ2: case WR_FLAT2: return WS_ASSEMBLY;     // the G2 Horner pass runs on the side stream, joined by the assembly
    case WR_SUM_POK: return f.has_commitment ? WS_HORNER : WS_UPLOAD;
    case WR_GLV: case WR_PART1C: case WR_PART1D: case WR_DIGITS_S: case WR_DIGITS_S2: case WR_GOK_S: case WR_GOK_S2: return WS_UPLOAD;      // latency path only
    default: break;
    }
    if (r >= WR_SJ1 && r <= WR_FLAT1_LAST) return WS_HORNER;
    return WS_ASSEMBLY;      // rs (the scalar multiplications), the sums, tmp
}

struct WipeRegionInfo { int region; uint64_t bytes; };      // one row of a lane's region table: what alloc_lane allocated

// per-chunk sizes.  The scratch needs are those alloc_lane sized the buffers by, for THIS chunk's batch: a chunk writes no further than that
struct WipeSizes {
    uint64_t B = 0, n = 0;                    // columns (the chunk's row stride) and statements
    uint64_t n_wires = 0, n_constraints = 0, domain_n = 0, rows_per_group = 0;
    uint64_t fe_bytes = 32, xyzz1_bytes = 0, xyzz2_bytes = 0;
    uint64_t part1a = 0, part1b = 0, part2a = 0, part2b = 0, digits = 0, digits_w = 0, gok = 0, sj1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sj2 = 0;      // bytes
};

// rows x width bytes at `offset` into the region, rows `pitch` apart.  image: a byte plane — row i holds 0x80 where the plane's row class
// says wide (class index i mod image_period), else 0.
struct WipeItem { int region; uint64_t offset, rows, pitch, width; bool image; uint64_t image_period; };
struct WipePlan { std::vector<WipeItem> a, b; };      // phase A (beside the Z sum), phase B (behind the assembly); a latency call: everything in b

namespace wipe_detail {
inline uint64_t alloc_of(const std::vector<WipeRegionInfo>& table, int r) { for (const auto& t : table) if (t.region == r) return t.bytes; return 0; }
inline void prefix(std::vector<WipeItem>& out, const std::vector<WipeRegionInfo>& table, int r, uint64_t bytes) {
    const uint64_t have = alloc_of(table, r);
    if (bytes > have) bytes = have;
    if (bytes) out.push_back(WipeItem{r, 0, 1, bytes, bytes, false, 0});
}
inline void plane(std::vector<WipeItem>& out, const std::vector<WipeRegionInfo>& table, int r, uint64_t rows_per_group, uint64_t groups, bool image) {
    uint64_t rows = rows_per_group * groups; const uint64_t have = alloc_of(table, r) / 64;
    if (rows > have) rows = have;
    if (!rows) return;
    if (image) out.push_back(WipeItem{r, 0, rows, 64, 64, true, rows_per_group});
    else out.push_back(WipeItem{r, 0, 1, rows * 64, rows * 64, false, 0});
}
}  // namespace wipe_detail

// The wipe of one chunk: every secret region over the extent this route wrote, in this chunk's row stride.
inline WipePlan wipe_plan(const ChunkRoute& rt, const RouteFacts& f, const WipeSizes& z, const std::vector<WipeRegionInfo>& table) {
    using namespace wipe_detail;
    WipePlan p;
    const uint64_t B = z.B, fe = z.fe_bytes, x1 = z.xyzz1_bytes, x2 = z.xyzz2_bytes;
    // a region goes to phase A when the call is a batch call and nothing touches it behind the trigger
    auto phase = [&](int r) -> std::vector<WipeItem>& { return !rt.latency && wipe_last_touch(r, rt, f) <= WIPE_PHASE_A_TRIGGER ? p.a : p.b; };
    // -- the matrices.  W always whole rows: k_assign_* and k_prep_rs write all B columns (the padding columns repeat the last statement)
    prefix(phase(WR_W), table, WR_W, (z.n_wires + 4) * B * fe);
    // a, b, c: a latency call whose witness came from the resident solver wrote (and transformed) the statements' columns only
    const bool cols = rt.latency && rt.resident && z.n < B;
    auto matrix = [&](int r, uint64_t rows) {
        if (!alloc_of(table, r)) return;
        if (cols) phase(r).push_back(WipeItem{r, 0, rows, B * fe, z.n * fe, false, 0});
        else prefix(phase(r), table, r, rows * B * fe);
    };
    matrix(WR_A, z.domain_n); matrix(WR_B, z.domain_n); matrix(WR_C, z.domain_n + 1);
    if (rt.small) {
        plane(phase(WR_W8), table, WR_W8, z.rows_per_group, B / 64, false);
        for (int r : {WR_A8, WR_B8, WR_C8}) plane(phase(r), table, r, z.n_constraints, B / 64, true);
    }
    prefix(phase(WR_DIGITS_W), table, WR_DIGITS_W, z.digits_w);
    // -- phase B: the Z sum's digits, the partial sums, the per-window and flat sums, the sum points, what the assembly read
    // (a latency call over the Z set's latency layout recodes into the wire sets' digit buffer where there is one: run_msm_g1 — the Z digits stay untouched)
    if (!(rt.latency && rt.use_zfew && alloc_of(table, WR_DIGITS_W))) prefix(p.b, table, WR_DIGITS, z.digits);
    prefix(p.b, table, WR_GOK, z.gok);
    prefix(p.b, table, WR_PART1A, z.part1a); prefix(p.b, table, WR_PART1B, z.part1b); prefix(p.b, table, WR_PART2A, z.part2a); prefix(p.b, table, WR_PART2B, z.part2b);
    for (int k = 0; k < 8; k++) { prefix(p.b, table, WR_SJ1 + k, z.sj1[k]); prefix(p.b, table, WR_FLAT1 + k, B * x1); }
    prefix(p.b, table, WR_SJ2, z.sj2); prefix(p.b, table, WR_FLAT2, B * x2);
    for (int r : {WR_SUM_A, WR_SUM_B1, WR_SUM_K, WR_SUM_Z, WR_SUM_C}) prefix(p.b, table, r, B * x1);
    prefix(p.b, table, WR_SUM_B2, B * x2); prefix(p.b, table, WR_TMP, 2 * B * x1);
    prefix(p.b, table, WR_INPUTS, 176 * B); prefix(p.b, table, WR_RS, 64 * B);
    if (f.has_commitment) {
        prefix(p.b, table, WR_MASK_IN, 32 * B); prefix(p.b, table, WR_MASK, B * fe); prefix(p.b, table, WR_COMMIT, B * fe);
        prefix(p.b, table, WR_SUM_D, B * x1); prefix(p.b, table, WR_SUM_POK, B * x1);
    }
    if (rt.latency)      // the scalar split and the side streams' scratch: sized for one 64-column batch, written by latency calls only
        for (int r : {WR_GLV, WR_PART1C, WR_PART1D, WR_DIGITS_S, WR_DIGITS_S2, WR_GOK_S, WR_GOK_S2}) prefix(p.b, table, r, alloc_of(table, r));
    return p;
}

// Every secret region over its whole allocation (alloc_lane; a call that leaves by an exception): `cap` = the lane's capacity in columns
inline std::vector<WipeItem> wipe_plan_whole(const std::vector<WipeRegionInfo>& table, uint64_t n_constraints) {
    std::vector<WipeItem> out;
    for (const auto& t : table) {
        if (wipe_region_public(t.region) || !t.bytes) continue;
        if (t.region == WR_A8 || t.region == WR_B8 || t.region == WR_C8) out.push_back(WipeItem{t.region, 0, t.bytes / 64, 64, 64, true, n_constraints});
        else out.push_back(WipeItem{t.region, 0, 1, t.bytes, t.bytes, false, 0});
    }
    return out;
}

}  // namespace gsc
