// See msm_set.hpp: the tables and the launch sequence of an MSM set, one copy for the engine and for the test hook gsc_debug_msm.
#include "msm_set.hpp"

namespace gsc {

namespace {

// rows of multiples (row i: len[i] entries at off[i]); work is cut into segments of at most 256 multiples, the projective scratch stays below 4 GiB
template <class AffT, class XyzzT>
void build_rows(const AffT* bases, const std::vector<uint64_t>& off, const std::vector<uint32_t>& len, AffT* table, hipStream_t stream) {
    const uint32_t cap = 256;
    const std::vector<MsmRowSeg> segs = msm_row_segments(off, len, cap);
    if (segs.empty()) return;
    size_t chunk = ((size_t)4 << 30) / (cap * sizeof(XyzzT)); if (chunk > segs.size()) chunk = segs.size();
    DevBuf<XyzzT> scratch(chunk * cap); DevBuf<MsmRowSeg> d_segs(segs.size());
    d_segs.upload(segs.data(), segs.size(), stream);
    for (size_t t0 = 0; t0 < segs.size(); t0 += chunk) launch_build_rows(bases, d_segs.p + t0, segs.size() - t0 < chunk ? segs.size() - t0 : chunk, cap, table, scratch.p, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
}

// group tables are built in chunks so that the projective scratch stays below ~2 GiB
template <class AffT, class XyzzT>
void build_subset(const AffT* b, size_t ng, AffT* t, uint8_t* ok, hipStream_t stream) {
    size_t chunk = ((size_t)2 << 30) / (MSM_GROUP_ENTRIES * sizeof(XyzzT)); if (chunk > ng) chunk = ng;
    DevBuf<XyzzT> sc(chunk * MSM_GROUP_ENTRIES);
    for (size_t g0 = 0; g0 < ng; g0 += chunk) launch_build_subset(b + 8 * g0, ng - g0 < chunk ? ng - g0 : chunk, t + g0 * MSM_GROUP_ENTRIES, sc.p, ok + g0, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
}

// Slice partials -> one sum per column: reduction levels over the call's ping-pong buffers pa (the partials) and pb until one group is left, which
// goes to `out`.  A latency call: the first n_real columns of every row of B only (nobody reads the padding proofs' columns), 64 slices per group.
// levels (optional): the slices entering every level and whether it took the by-proof kernel.
template <class XyzzT>
void reduce_slices(const MsmRun<XyzzT>& r, size_t nslices, size_t cols, XyzzT* out, std::vector<std::pair<size_t, bool>>* levels) {
    XyzzT* src = r.pa; XyzzT* alt = r.pb; size_t ns = nslices;
    for (;;) {
        const size_t groups = r.latency ? (ns + 63) / 64 : msm_reduce_groups(ns, cols);
        XyzzT* dst = groups == 1 ? out : alt;
        if (levels) levels->emplace_back(ns, !r.latency && msm_reduce_by_proof(ns, cols));
        if (r.latency) launch_msm_reduce_few(src, ns, cols, r.B, r.n_real, dst, r.ctx.stream);
        else launch_msm_reduce(src, ns, cols, dst, r.ctx.stream);
        if (groups == 1) break;
        XyzzT* t = src; src = dst; alt = t; ns = groups;
    }
}

}  // namespace

template <class AffT, class XyzzT>
void msm_build_tables(MsmSet<AffT>& set, const AffT* bases, const MsmFlatPlan& plan, const std::vector<uint32_t>& rows, int c, hipStream_t stream, size_t* table_bytes) {
    const std::vector<uint32_t>&src = plan.src, &shift = plan.shift, &frows = plan.frows, &len = plan.len, &wide = plan.wide; const std::vector<int32_t>& octwin = plan.octwin;
    const size_t D = (size_t)1 << (c - 1);
    set.c = c; set.nwin = msm_windows(c);
    if (plan.nexpanded) { set.cv = plan.cv; set.nexpanded = plan.nexpanded; }
    set.nflat = src.size(); set.nbit = plan.nbit;
    if (set.nflat) {
        DevBuf<AffT> fb(set.nflat); DevBuf<uint32_t> d_src(set.nflat), d_shift(set.nflat);
        d_src.upload(src.data(), src.size(), stream); d_shift.upload(shift.data(), shift.size(), stream);
        launch_shift_bases(bases, d_src.p, d_shift.p, set.nflat, fb.p, stream);
        std::vector<uint64_t> off; const size_t entries = msm_row_offsets(len, off);
        set.ftable.alloc(entries); *table_bytes += set.ftable.bytes();
        set.rowoff.alloc(set.nflat); set.rowlen.alloc(set.nflat); set.frows.alloc(set.nflat); set.octwin.alloc(octwin.size());
        set.rowoff.upload(off.data(), set.nflat, stream); set.rowlen.upload(len.data(), set.nflat, stream);
        set.frows.upload(frows.data(), set.nflat, stream); set.octwin.upload(octwin.data(), octwin.size(), stream);
        build_rows<AffT, XyzzT>(fb.p, off, len, set.ftable.p, stream);
        if (set.nbit) {
            const size_t ng = set.nbit / 8;
            set.sub.alloc(ng * MSM_GROUP_ENTRIES); set.group_ok.alloc(ng);
            *table_bytes += set.sub.bytes();
            build_subset<AffT, XyzzT>(fb.p, ng, set.sub.p, set.group_ok.p, stream);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));      // fb, d_src, d_shift go out of scope
    }
    set.nwide = wide.size();
    if (set.nwide) {      // windowed part: uniform rows
        DevBuf<AffT> wb(set.nwide); DevBuf<uint32_t> d_src(set.nwide), d_shift(set.nwide);
        std::vector<uint32_t> zero(set.nwide, 0u), wrows(set.nwide);
        for (size_t i = 0; i < set.nwide; i++) wrows[i] = rows[wide[i]];
        d_src.upload(wide.data(), set.nwide, stream); d_shift.upload(zero.data(), set.nwide, stream);
        launch_shift_bases(bases, d_src.p, d_shift.p, set.nwide, wb.p, stream);
        set.wrows.alloc(set.nwide); set.wrows.upload(wrows.data(), set.nwide, stream);
        set.wtable.alloc(set.nwide * D); *table_bytes += set.wtable.bytes();
        std::vector<uint64_t> off(set.nwide); std::vector<uint32_t> wlen(set.nwide, (uint32_t)D);
        for (size_t i = 0; i < set.nwide; i++) off[i] = i * D;
        build_rows<AffT, XyzzT>(wb.p, off, wlen, set.wtable.p, stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));
    }
}

template <class AffT, class XyzzT>
void msm_run(const MsmSet<AffT>& set, const MsmRun<XyzzT>& r, MsmHornerJobs& pending) {
    const MsmCtx& ctx = r.ctx;
    const size_t B = r.B;
    const MsmGeometry g = msm_geometry(set.shape(), B, r.latency, r.opts);
    std::vector<std::pair<size_t, bool>>* const flat_levels = r.levels ? &r.levels->flat : nullptr;
    // `nslices` slices of the flat rows of `m` for a call with a handful of statements: lanes = octets of bases, partial sums to `out`
    auto flat_few = [&](const MsmSet<AffT>& m, size_t nslices, XyzzT* out, bool stamp) {
        if (!m.nflat) return;
        MsmFlatRecodeArgs ra{r.scalars, m.frows.p, m.octwin.p, m.nflat, B, m.cv, ctx.digits, m.nbit, m.group_ok.p, ctx.gok, r.wires ? 1 : 0, ctx.plane, ctx.plane_rows, ctx.plane_stride};
        launch_msm_recode_flat_few(ra, r.n_real, ctx.stream);
        MsmFlatArgs a{m.ftable.p, m.rowoff.p, m.rowlen.p, m.nflat, ctx.digits, B, nslices, g.flat_per, out, m.nbit, m.sub.p, ctx.gok, r.scalars, m.frows.p};
        if (stamp && r.ev_begin) HIP_CHECK(hipEventRecord(r.ev_begin, ctx.stream));
        launch_msm_flat_few<AffT>(a, r.n_real, ctx.stream);
        if (stamp && r.ev_end) HIP_CHECK(hipEventRecord(r.ev_end, ctx.stream));
    };
    if (r.latency && set.few_wide) {
        // every part of the set as flat rows: the partial sums of both parts side by side, one reduction, no Horner pass
        const size_t own = g.flat_slices - g.few_wide_slices;
        flat_few(set, own, r.pa, true);
        flat_few(*set.few_wide, g.few_wide_slices, r.pa + own * B, false);
        reduce_slices(r, g.flat_slices, B, r.sum, flat_levels);
        return;
    }
    if (set.nflat) {
        if (r.latency) flat_few(set, g.flat_slices, r.pa, true);
        else {
            MsmFlatRecodeArgs ra{r.scalars, set.frows.p, set.octwin.p, set.nflat, B, set.cv, ctx.digits, set.nbit, set.group_ok.p, ctx.gok, r.wires ? 1 : 0, ctx.plane, ctx.plane_rows, ctx.plane_stride};
            launch_msm_recode_flat(ra, ctx.stream);
            MsmFlatArgs a{set.ftable.p, set.rowoff.p, set.rowlen.p, set.nflat, ctx.digits, B, g.flat_slices, g.flat_per, r.pa, set.nbit, set.sub.p, ctx.gok, r.scalars, set.frows.p};
            launch_msm_flat<AffT>(a, ctx.stream);
        }
        reduce_slices(r, g.flat_slices, B, set.nwide ? r.flat : r.sum, flat_levels);
    }
    if (set.nwide) {      // (a latency call comes here for a set whose windowed part has no latency layout: GSC_FEW_WIDE=0, Z without mZfew)
        uint4* const digits = r.win_digits ? r.win_digits : ctx.digits;
        MsmRecodeArgs ra{r.scalars, set.wrows.p, r.wires ? 1 : 0, set.nwide, B, set.c, set.nwin, digits};
        if (!r.digits_ready) launch_msm_recode(ra, ctx.stream);
        MsmWinArgs a{set.wtable.p, set.c, set.nwin, set.nwide, digits, B, g.win_slices, g.win_per, r.pa, r.clk, r.clk_mask,
                     r.digits_ready ? set.digit_bases : 0};      // (digits recoded here are laid out for the bases walked)
        if (r.ev_begin) HIP_CHECK(hipEventRecord(r.ev_begin, ctx.stream));
        if (r.latency) launch_msm_win_few<AffT>(a, r.n_real, ctx.stream);
        else launch_msm_win<AffT>(a, ctx.stream);
        if (r.ev_end) HIP_CHECK(hipEventRecord(r.ev_end, ctx.stream));
        reduce_slices(r, g.win_slices, g.sj, r.sj, r.levels ? &r.levels->win : nullptr);      // slices -> one sum per (window, proof)
        if (pending.n >= MSM_HORNER_JOBS) throw std::runtime_error("internal: too many pending Horner passes");
        pending.job[pending.n++] = MsmHornerJob{r.sj, set.nflat ? r.flat : (XyzzT*)nullptr, r.sum, set.nwin, set.c};
    }
    if (!set.nflat && !set.nwide) HIP_CHECK(hipMemsetAsync(r.sum, 0, B * sizeof(XyzzT), ctx.stream));      // empty set: the point at infinity
}

template void msm_build_tables<G1Aff, G1Xyzz>(MsmSet<G1Aff>&, const G1Aff*, const MsmFlatPlan&, const std::vector<uint32_t>&, int, hipStream_t, size_t*);
template void msm_build_tables<G2Aff, G2Xyzz>(MsmSet<G2Aff>&, const G2Aff*, const MsmFlatPlan&, const std::vector<uint32_t>&, int, hipStream_t, size_t*);
template void msm_run<G1Aff, G1Xyzz>(const MsmSet<G1Aff>&, const MsmRun<G1Xyzz>&, MsmHornerJobs&);
template void msm_run<G2Aff, G2Xyzz>(const MsmSet<G2Aff>&, const MsmRun<G2Xyzz>&, MsmHornerJobs&);

}  // namespace gsc
