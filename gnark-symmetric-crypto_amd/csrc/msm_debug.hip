// TEST HOOK gsc_debug_msm (include/libprove.h): the MSM kernels on a caller's bases and scalars, without a key, a circuit or a witness.
// The layout comes from the planner build_set uses (msm_layout.hpp), the tables from the same builders, and the sums run through run_msm's launch
// sequence: launch_shift_bases, launch_build_rows, launch_build_subset; launch_msm_recode / launch_msm_recode_flat(_few); launch_msm_flat(_few) /
// launch_msm_win(_few); the reduction loops of reduce_slices(_few); launch_msm_horner with the flat sum as addend.  No production kernel is changed
// or copied for it: the one kernel here turns the XYZZ sums into canonical affine coordinates.  tests/test_gpu_msm.py is the caller.
#include "msm_debug.hpp"
#include "engine_impl.hpp"
#include "msm_dev.hpp"

namespace gsc {
using namespace bn254;

namespace {

// out[i] = sums[i] as canonical little-endian coordinates (G1 x, y; G2 x.a0, x.a1, y.a0, y.a1); inf[i] = 1 and zeros for the point at infinity
template <class F>
__global__ __launch_bounds__(64) void k_debug_msm_out(const fe* sums, size_t n, fe* out, uint8_t* inf) {
    using C = Curve9<F>;
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Xyzz9<F> v = C::load_xyzz(sums + i * (4 * F::WORDS));
    fe* o = out + i * (2 * F::WORDS);
    if (v.inf) { inf[i] = 1; for (int q = 0; q < 2 * F::WORDS; q++) store_fe(o + q, fe{}); return; }
    inf[i] = 0;
    const Aff9<F> a = C::to_aff(v);
    if constexpr (F::WORDS == 1) { store_fe(o, Fp29::pack(Fp29::from_mont(a.x))); store_fe(o + 1, Fp29::pack(Fp29::from_mont(a.y))); }
    else {
        store_fe(o, Fp29::pack(Fp29::from_mont(a.x.a0))); store_fe(o + 1, Fp29::pack(Fp29::from_mont(a.x.a1)));
        store_fe(o + 2, Fp29::pack(Fp29::from_mont(a.y.a0))); store_fe(o + 3, Fp29::pack(Fp29::from_mont(a.y.a1)));
    }
}

const uint8_t kFrModBE[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                              0x28, 0x33, 0xe8, 0x48, 0x79, 0xb9, 0x70, 0x91, 0x43, 0xe1, 0xf5, 0x93, 0xf0, 0x00, 0x00, 0x01};

[[noreturn]] void refuse(const std::string& why) { throw std::runtime_error("gsc_debug_msm: " + why); }

// what the host can decide: everything but "the point is on the curve / in the subgroup"
struct Checked { MsmFlatPlan plan; int nwin = 0; size_t ncols = 0, flat_entries = 0, D = 0, noct_w = 0; std::vector<uint64_t> off; };
Checked check(const gsc_debug_msm_args& a) {
    Checked ck;
    if (a.group < 0 || a.group > 1) refuse("no such group");
    if (a.c < 4 || a.c > MSM_MAX_WINDOW) refuse("c outside [4, 17]");
    if (a.cv != 0 && (a.cv < 4 || a.cv > 15)) refuse("cv outside [4, 15]");
    if (a.batch != 64 && a.batch != 128) refuse("the batch is 64 or 128");
    if (a.nproofs > MSM_FEW_PROOFS || a.nproofs > a.batch) refuse("nproofs beyond the latency kernels' 32 / the batch");
    if (a.per_flat % 8 || a.per_win % 8) refuse("bases per slice must be a multiple of 8");
    if (a.per_flat > 512) refuse("a flat slice holds at most 512 bases");
    if (a.nbases > (1u << 16) || a.digit_bases > (1u << 16) || a.n_rows > (1u << 17)) refuse("more than 2^16 bases / 2^17 scalar rows");
    if (!a.info || !a.out || !a.out_inf) refuse("no room for the results");
    if (a.nbases && (!a.points || !a.kind || !a.rows)) refuse("bases without points, kinds or rows");
    if (!a.n_rows || !a.scalars_be || a.zero_row >= a.n_rows) refuse("no scalar rows / no zero row among them");
    const size_t W = a.group == 0 ? 64 : 128;
    MsmSorted sorted;
    for (uint32_t k = 0; k < a.nbases; k++) {
        if (a.rows[k] >= a.n_rows) refuse("a scalar row out of range");
        if (a.kind[k] == 0) sorted.bits.push_back(k);
        else if (a.kind[k] == 1) {
            if (!a.rowlen || a.rowlen[k] < 1 || a.rowlen[k] > 32768) refuse("a narrow row of no length, or longer than 2^15");
            sorted.narrow.push_back(k); sorted.narrow_len.push_back(a.rowlen[k]);
        } else if (a.kind[k] == 2) sorted.wide.push_back(k);
        else refuse("no such kind of base");
        const uint8_t* pt = a.points + W * k;
        bool zero = true; for (size_t i = 0; i < W; i++) zero = zero && !pt[i];
        if ((pt[0] & 0xC0) || zero) refuse("a point that is not raw and finite");
    }
    if (!a.mont && (!sorted.bits.empty() || !sorted.narrow.empty())) refuse("canonical scalars (mont = 0) with bit or narrow bases: the flat kernels read Montgomery images outside window octets");
    for (size_t i = 0; i < (size_t)a.n_rows * a.batch; i++) if (memcmp(a.scalars_be + 32 * i, kFrModBE, 32) >= 0) refuse("a scalar that is not below r");
    for (size_t i = 0; i < a.batch; i++) for (int q = 0; q < 32; q++) if (a.scalars_be[32 * ((size_t)a.zero_row * a.batch + i) + q]) refuse("the zero row is not zero");
    if (a.plane && (a.plane_rows > a.plane_stride || a.plane_rows > a.n_rows)) refuse("plane_rows beyond plane_stride / the scalar rows");
    if (a.plane) for (size_t i = 0; i < (size_t)(a.batch / 64) * a.plane_stride * 64; i++) { const int8_t t = a.plane[i]; if (t != 0 && t != 1 && t != -1 && t != WS_PLANE_WIDE) refuse("a plane entry that is not 0, 1, -1 or -128"); }
    std::vector<uint32_t> rows(a.rows, a.rows + a.nbases);
    // cv > 0: every wide base is expanded (build_set's expand_cv); cv == 0: none is (EXPAND_MAX = 0), they take the windowed kernel
    ck.plan = msm_plan_flat(std::move(sorted), rows, a.zero_row, false, a.cv, 0, 0, msm_windows);
    ck.nwin = msm_windows(a.c); ck.D = (size_t)1 << (a.c - 1);
    ck.ncols = a.nproofs ? a.nproofs : a.batch;
    ck.flat_entries = msm_row_offsets(ck.plan.len, ck.off);
    const size_t nwide = ck.plan.wide.size();
    if (ck.flat_entries + nwide * ck.D + (ck.plan.nbit / 8) * (size_t)MSM_GROUP_ENTRIES > ((size_t)1 << 28)) refuse("more than 2^28 table entries");
    if (a.digit_bases) {
        if (a.digit_bases <= nwide || !a.digit_rows) refuse("digit_bases must exceed the wide bases and come with digit_rows");
        for (uint32_t i = 0; i < a.digit_bases; i++) if (a.digit_rows[i] >= a.n_rows || (i < nwide && a.digit_rows[i] != rows[ck.plan.wide[i]])) refuse("digit_rows out of range, or not the wide bases' rows in front");
    }
    ck.noct_w = ((a.digit_bases ? a.digit_bases : nwide) + 7) / 8;
    return ck;
}

template <class AffT, class XyzzT>
void build_rows(const AffT* bases, const std::vector<uint64_t>& off, const std::vector<uint32_t>& len, AffT* table, hipStream_t s) {
    const uint32_t cap = 256;
    const std::vector<MsmRowSeg> segs = msm_row_segments(off, len, cap);
    if (segs.empty()) return;
    size_t chunk = ((size_t)1 << 30) / (cap * sizeof(XyzzT)); if (chunk > segs.size()) chunk = segs.size();
    DevBuf<XyzzT> scratch(chunk * cap); DevBuf<MsmRowSeg> d_segs(segs.size());
    d_segs.upload(segs.data(), segs.size(), s);
    for (size_t t0 = 0; t0 < segs.size(); t0 += chunk) launch_build_rows(bases, d_segs.p + t0, segs.size() - t0 < chunk ? segs.size() - t0 : chunk, cap, table, scratch.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
}

void copy_out(uint8_t* dst, size_t cap, const void* src, size_t bytes, uint32_t& written, const char* what, hipStream_t s) {
    written = 0;
    if (!dst && !cap) return;
    if (!dst || cap < bytes) refuse(std::string("too small a buffer for ") + what);
    if (bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    written = (uint32_t)bytes;
}

template <class AffT, class XyzzT>
void run(const gsc_debug_msm_args& a, const Checked& ck) {
    using F = typename GroupOf<AffT>::F;
    const MsmFlatPlan& pl = ck.plan;
    const size_t B = a.batch, n = a.nbases, nflat = pl.src.size(), nwide = pl.wide.size(), nwin = (size_t)ck.nwin, npr = a.nproofs;
    const bool few = npr != 0;
    hipStream_t s = nullptr;
    uint32_t* info = a.info; memset(info, 0, 64 * sizeof(uint32_t));
    info[0] = (uint32_t)nflat; info[1] = (uint32_t)pl.nbit; info[2] = (uint32_t)pl.nexpanded; info[3] = (uint32_t)nwide; info[4] = (uint32_t)nwin;
    info[44] = (uint32_t)ck.ncols; info[45] = (uint32_t)(nflat / 8); info[46] = (uint32_t)ck.noct_w; info[47] = (uint32_t)pl.cv;

    // the bases, decoded like a key's points
    const size_t cb = sizeof(AffT) / 2;
    DevBuf<AffT> bases(n ? n : 1);
    if (n) {
        KeyPoints raw; raw.x.resize(n * cb); raw.y.resize(n * cb);
        for (size_t k = 0; k < n; k++) { memcpy(&raw.x[k * cb], a.points + 2 * cb * k, cb); memcpy(&raw.y[k * cb], a.points + 2 * cb * k + cb, cb); }
        std::vector<uint8_t> st;
        if constexpr (sizeof(AffT) == sizeof(G1Aff)) st = decode_g1_points(raw, bases.p, s); else st = decode_g2_points(raw, bases.p, s);
        for (size_t k = 0; k < n; k++) if (st[k] != 0) refuse("a point that is not on the curve / in the group");
    }
    // the scalars: [row][column], Montgomery images or canonical limbs
    const size_t nsc = (size_t)a.n_rows * B;
    DevBuf<fe> scalars(nsc);
    if (a.mont) {
        DevBuf<uint8_t> be(32 * nsc); be.upload(a.scalars_be, 32 * nsc, s);
        launch_fr_from_be(be.p, scalars.p, nsc, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    } else {
        std::vector<uint8_t> le(32 * nsc);
        for (size_t i = 0; i < nsc; i++) for (int q = 0; q < 32; q++) le[32 * i + q] = a.scalars_be[32 * i + 31 - q];
        HIP_CHECK(hipMemcpy(scalars.p, le.data(), le.size(), hipMemcpyHostToDevice));
    }
    DevBuf<int8_t> plane;
    if (a.plane) { const size_t pb = (B / 64) * (size_t)a.plane_stride * 64; plane.alloc(pb ? pb : 1); if (pb) HIP_CHECK(hipMemcpy(plane.p, a.plane, pb, hipMemcpyHostToDevice)); }

    DevBuf<XyzzT> sum(B), flat(B);
    HIP_CHECK(hipMemsetAsync(sum.p, 0, sum.bytes(), s)); HIP_CHECK(hipMemsetAsync(flat.p, 0, flat.bytes(), s));
    std::vector<std::pair<size_t, bool>> levels;
    auto put_levels = [&](uint32_t at) {
        if (levels.size() > 8) refuse("more than eight reduction levels");
        info[at] = (uint32_t)levels.size();
        for (size_t i = 0; i < levels.size(); i++) { info[at + 1 + 2 * i] = (uint32_t)levels[i].first; info[at + 2 + 2 * i] = levels[i].second ? 1u : 0u; }
        levels.clear();
    };

    // ---- flat part ----
    DevBuf<AffT> ftable, sub; DevBuf<uint64_t> rowoff; DevBuf<uint32_t> rowlen, frows; DevBuf<int32_t> octwin; DevBuf<uint8_t> group_ok, gok; DevBuf<uint4> fdigits;
    DevBuf<XyzzT> fpa, fpb;
    if (nflat) {
        {
            DevBuf<AffT> fb(nflat); DevBuf<uint32_t> d_src(nflat), d_shift(nflat);
            d_src.upload(pl.src.data(), nflat, s); d_shift.upload(pl.shift.data(), nflat, s);
            launch_shift_bases(bases.p, d_src.p, d_shift.p, nflat, fb.p, s);
            ftable.alloc(ck.flat_entries); rowoff.alloc(nflat); rowlen.alloc(nflat); frows.alloc(nflat); octwin.alloc(pl.octwin.size());
            rowoff.upload(ck.off.data(), nflat, s); rowlen.upload(pl.len.data(), nflat, s); frows.upload(pl.frows.data(), nflat, s); octwin.upload(pl.octwin.data(), pl.octwin.size(), s);
            build_rows<AffT, XyzzT>(fb.p, ck.off, pl.len, ftable.p, s);
            const size_t ng = pl.nbit / 8;
            if (ng) {
                sub.alloc(ng * MSM_GROUP_ENTRIES); group_ok.alloc(ng);
                DevBuf<XyzzT> sc(ng * MSM_GROUP_ENTRIES);
                launch_build_subset(fb.p, ng, sub.p, sc.p, group_ok.p, s);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipStreamSynchronize(s));
            }
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));
        }
        const size_t noct = nflat / 8, ng = pl.nbit / 8, gok_n = ng * (few ? MSM_FEW_PROOFS : B / 64);
        fdigits.alloc(noct * B); gok.alloc(gok_n ? gok_n : 1);
        HIP_CHECK(hipMemsetAsync(fdigits.p, 0, fdigits.bytes(), s)); HIP_CHECK(hipMemsetAsync(gok.p, 0, gok.bytes(), s));
        MsmFlatRecodeArgs ra{scalars.p, frows.p, octwin.p, nflat, B, pl.cv, fdigits.p, pl.nbit, group_ok.p, gok.p, a.mont ? 1 : 0, a.plane ? plane.p : nullptr, a.plane ? a.plane_rows : 0, a.plane ? a.plane_stride : 0};
        size_t per = 512, nslices;
        if (few) nslices = msm_flat_few_slices(nflat);
        else if (a.per_flat) { per = a.per_flat; nslices = (nflat + per - 1) / per; }
        else nslices = msm_slices(nflat, 1, 256, B, per);
        if (per % 8 || per > 512 || nslices * per < nflat) refuse("internal: flat slices do not cover the bases");
        info[5] = (uint32_t)nslices; info[6] = (uint32_t)per;
        fpa.alloc(nslices * B); fpb.alloc(nslices * B);
        HIP_CHECK(hipMemsetAsync(fpa.p, 0, fpa.bytes(), s)); HIP_CHECK(hipMemsetAsync(fpb.p, 0, fpb.bytes(), s));
        MsmFlatArgs fa{ftable.p, rowoff.p, rowlen.p, nflat, fdigits.p, B, nslices, per, fpa.p, pl.nbit, sub.p, gok.p, scalars.p, frows.p};
        XyzzT* dst = nwide ? flat.p : sum.p;
        if (few) {
            launch_msm_recode_flat_few(ra, npr, s);
            launch_msm_flat_few<AffT>(fa, npr, s);
            msm_reduce_slices_few(s, fpa.p, fpb.p, nslices, B, B, npr, dst, &levels);
        } else {
            launch_msm_recode_flat(ra, s);
            launch_msm_flat<AffT>(fa, s);
            msm_reduce_slices(s, fpa.p, fpb.p, nslices, B, dst, &levels);
        }
        HIP_CHECK(hipGetLastError());
        put_levels(9);
    }
    // ---- windowed part ----
    DevBuf<AffT> wtable; DevBuf<uint32_t> wrows; DevBuf<uint4> wdigits; DevBuf<XyzzT> wpa, wpb, sj;
    if (nwide) {
        const size_t nrec = a.digit_bases ? a.digit_bases : nwide;
        {
            DevBuf<AffT> wb(nwide); DevBuf<uint32_t> d_src(nwide), d_shift(nwide);
            std::vector<uint32_t> zero(nwide, 0u), wr(nrec);
            for (size_t i = 0; i < nrec; i++) wr[i] = a.digit_bases ? a.digit_rows[i] : a.rows[pl.wide[i]];
            d_src.upload(pl.wide.data(), nwide, s); d_shift.upload(zero.data(), nwide, s);
            launch_shift_bases(bases.p, d_src.p, d_shift.p, nwide, wb.p, s);
            wrows.alloc(nrec); wrows.upload(wr.data(), nrec, s);
            wtable.alloc(nwide * ck.D);
            std::vector<uint64_t> off(nwide); std::vector<uint32_t> len(nwide, (uint32_t)ck.D);
            for (size_t i = 0; i < nwide; i++) off[i] = i * ck.D;
            build_rows<AffT, XyzzT>(wb.p, off, len, wtable.p, s);
        }
        size_t per = 0, nslices;
        if (a.per_win) { per = a.per_win; nslices = (nwide + per - 1) / per; }
        else { nslices = msm_slices(nwide, nwin, 256, B, per); if (few) msm_slices_latency(nwide, nslices, per); }
        if (!per || per % 8 || nslices * per < nwide) refuse("internal: windowed slices do not cover the bases");
        info[7] = (uint32_t)nslices; info[8] = (uint32_t)per;
        const size_t Bw = B * nwin;
        wdigits.alloc(nwin * ck.noct_w * B * msm_digit_words(a.c));
        wpa.alloc(nslices * Bw); wpb.alloc(nslices * Bw); sj.alloc(Bw);
        HIP_CHECK(hipMemsetAsync(wdigits.p, 0, wdigits.bytes(), s)); HIP_CHECK(hipMemsetAsync(wpa.p, 0, wpa.bytes(), s)); HIP_CHECK(hipMemsetAsync(wpb.p, 0, wpb.bytes(), s)); HIP_CHECK(hipMemsetAsync(sj.p, 0, sj.bytes(), s));
        MsmRecodeArgs ra{scalars.p, wrows.p, a.mont ? 1 : 0, nrec, B, a.c, (int)nwin, wdigits.p};
        launch_msm_recode(ra, s);
        MsmWinArgs wa{wtable.p, a.c, (int)nwin, nwide, wdigits.p, B, nslices, per, wpa.p, nullptr, 0u, a.digit_bases ? (size_t)a.digit_bases : 0};
        if (few) { launch_msm_win_few<AffT>(wa, npr, s); msm_reduce_slices_few(s, wpa.p, wpb.p, nslices, Bw, B, npr, sj.p, &levels); }
        else { launch_msm_win<AffT>(wa, s); msm_reduce_slices(s, wpa.p, wpb.p, nslices, Bw, sj.p, &levels); }
        MsmHornerJobs jobs{}; jobs.n = 1;
        jobs.job[0] = MsmHornerJob{sj.p, nflat ? flat.p : (XyzzT*)nullptr, sum.p, (int)nwin, a.c};
        launch_msm_horner<AffT>(jobs, B, s);
        HIP_CHECK(hipGetLastError());
        put_levels(26);
        info[43] = nflat ? 1u : 0u;
    }
    // ---- results ----
    DevBuf<fe> d_out(2 * F::WORDS * ck.ncols); DevBuf<uint8_t> d_inf(ck.ncols);
    hipLaunchKernelGGL(k_debug_msm_out<F>, dim3((unsigned)((ck.ncols + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const fe*>(sum.p), ck.ncols, d_out.p, d_inf.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(a.out, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(a.out_inf, d_inf.p, ck.ncols, hipMemcpyDeviceToHost, s));
    copy_out(a.flat_digits, a.flat_digits_cap, fdigits.p, fdigits.bytes(), info[48], "the flat digits", s);
    copy_out(a.win_digits, a.win_digits_cap, wdigits.p, wdigits.bytes(), info[49], "the windowed digits", s);
    copy_out(a.gok, a.gok_cap, gok.p, pl.nbit / 8 * (few ? MSM_FEW_PROOFS : B / 64), info[50], "gok", s);
    copy_out(a.group_ok, a.group_ok_cap, group_ok.p, pl.nbit / 8, info[51], "group_ok", s);
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace

void debug_msm(int device, const gsc_debug_msm_args& a) {
    const Checked ck = check(a);      // every refusal the host can decide comes before a device is asked for
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device available");
    HIP_CHECK(hipSetDevice(device));
    if (a.group == 0) run<G1Aff, G1Xyzz>(a, ck); else run<G2Aff, G2Xyzz>(a, ck);
}

}  // namespace gsc
