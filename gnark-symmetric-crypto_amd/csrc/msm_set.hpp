// One fixed-base MSM set on the device, shared by the engine (AlgorithmImpl::build_set, run_msm_g1 / run_msm_g2) and the test hook gsc_debug_msm
// (msm_debug.hip): the tables of a planned layout (msm_build_tables) and the launch sequence of one call over them (msm_run) — recoding,
// gather-accumulate of the flat and the windowed part, slice reductions, the Horner job.  The layout and the slices of a call are decided by
// msm_layout.hpp (msm_plan_flat, msm_geometry).  Implementation: msm_set.hip.
#pragma once
#include "kernels.hpp"
#include "solver_tables.hpp"
#include <memory>
#include <utility>
#include <vector>

namespace gsc {

template <class AffT>
struct MsmSet {                     // one fixed-base MSM of the proving key (kernels.hpp, "multi-scalar multiplication")
    size_t nbases = 0;              // bases of the key in this set
    // windowed part (uniform rows of 2^(c-1) multiples): every base of Z; the wide wires of a wire set when there are many
    DevBuf<AffT> wtable; DevBuf<uint32_t> wrows; size_t nwide = 0; int c = 0, nwin = 0;
    // the folded Z set (init_key): the last quotient kernel lays the digits out for this many bases, of which the kernel walks the first nwide (0: nwide)
    size_t digit_bases = 0;
    // flat part: [bit groups of eight][narrow wires, own row lengths][window octets of a few wide wires (cv-bit digits)]
    DevBuf<AffT> ftable; DevBuf<uint64_t> rowoff; DevBuf<uint32_t> rowlen; DevBuf<uint32_t> frows; DevBuf<int32_t> octwin;
    size_t nflat = 0, nbit = 0, nexpanded = 0; int cv = 0; DevBuf<AffT> sub; DevBuf<uint8_t> group_ok;
    // latency path: the windowed part once more as a flat set of (base, window) rows of 8-bit digits (no Horner pass behind it)
    std::unique_ptr<MsmSet<AffT>> few_wide;
    bool latency_flat() const { return !nwide || few_wide; }       // calls with a handful of statements need no windowed kernel for this set
    MsmShape shape() const { return MsmShape{nflat, nbit, nwide, c, nwin, digit_bases, few_wide ? few_wide->nflat : 0}; }
};

// The tables of `plan` over the decoded bases on the device (the key's order): the flat part's shifted bases, row offsets, rows of multiples and
// bit-group subset sums, the windowed part's uniform rows of 2^(c-1) multiples and scalar rows.  rows: the scalar row of every base.  Fills every
// field of `set` but nbases, digit_bases and few_wide; adds the tables' bytes to *table_bytes; `stream` is synchronised before returning.
template <class AffT, class XyzzT>
void msm_build_tables(MsmSet<AffT>& set, const AffT* bases, const MsmFlatPlan& plan, const std::vector<uint32_t>& rows, int c, hipStream_t stream, size_t* table_bytes);

// the reduction levels a call ran, per part: the slices entering every level and whether it took the by-proof kernel (the test hook)
struct MsmLevels { std::vector<std::pair<size_t, bool>> flat, win; };

// where a call runs: its stream, the digit and bit-group verdict buffers, and the scalars' byte plane (small-integer witness path; none: the matrix holds every row)
struct MsmCtx { hipStream_t stream; uint4* digits; uint8_t* gok; const int8_t* plane = nullptr; size_t plane_rows = 0, plane_stride = 0; };

// One call.  scalars: the wire matrix W (Montgomery: wires = true) or h (canonical; Z), [row][B].  latency: the latency kernels, which work on the
// first n_real columns only.  pa / pb: the slice partials and the reduction's ping-pong (msm_geometry's pa and pb points); sj: per-window sums
// [window][B]; flat: the flat part's sum [B] of a set with both parts; sum: the result [B].
template <class XyzzT>
struct MsmRun {
    MsmCtx ctx;
    const fe* scalars; bool wires;
    size_t B, n_real; bool latency;
    XyzzT *pa, *pb, *sj, *flat, *sum;
    bool digits_ready = false;      // the windowed part's digits are already in the digit buffer, laid out for set.digit_bases bases: no recoding pass
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;      // recorded around the dominant kernel (null: not stamped)
    unsigned long long* clk = nullptr; uint32_t clk_mask = 0;      // MsmWinArgs::clk and exp_entry_mask
    MsmLaunchOpts opts;
    uint4* win_digits = nullptr;    // the windowed part's digits apart from the flat part's (null: both in ctx.digits, one after the other)
    MsmLevels* levels = nullptr;
};
// The Horner pass of the windowed part is NOT launched here: it is queued in `pending` and flushed together with those of other sets
// (launch_msm_horner), because each is a serial chain of 254 doublings whose duration does not depend on the batch.
template <class AffT, class XyzzT>
void msm_run(const MsmSet<AffT>& set, const MsmRun<XyzzT>& run, MsmHornerJobs& pending);

}  // namespace gsc
