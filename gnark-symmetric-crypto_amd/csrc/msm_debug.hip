// TEST HOOK gsc_debug_msm (include/libprove.h): the MSM kernels on a caller's bases and scalars, without a key, a circuit or a witness.
// What is the hook's own: the refusals (check), decoding the caller's points and scalars, scratch for one call (sized by msm_geometry), the info
// block and the copies back.  Everything between is the engine's own code: the planner build_set uses (msm_plan_flat, msm_layout.hpp), its table
// builder (msm_build_tables, msm_set.hpp) and the launch sequence of a prover's MSM (msm_run), then launch_msm_horner on the job that left.  With
// digit_bases the hook recodes digit_rows into the digit buffer itself (launch_msm_recode), as the last quotient kernel does for the folded Z set.
// No production kernel is changed or copied for it: the one kernel here turns the XYZZ sums into canonical affine coordinates (debug_ops.hpp's sum_out).
// tests/test_gpu_msm.py is the caller.
#include "msm_debug.hpp"
#include "engine_impl.hpp"
#include "msm_dev.hpp"
#include "debug_ops.hpp"

namespace gsc {
using namespace bn254;

namespace {

// out[i] = sums[i] as canonical little-endian coordinates; inf[i] = 1 and zeros for the point at infinity
template <class F>
__global__ __launch_bounds__(64) void k_debug_msm_out(const fe* sums, size_t n, fe* out, uint8_t* inf) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) dbg::sum_out<F>(sums, i, out, inf);
}

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
    const size_t B = a.batch, n = a.nbases, nflat = pl.src.size(), nwide = pl.wide.size(), npr = a.nproofs;
    const bool few = npr != 0;
    hipStream_t s = nullptr;
    uint32_t* info = a.info; memset(info, 0, 64 * sizeof(uint32_t));
    info[0] = (uint32_t)nflat; info[1] = (uint32_t)pl.nbit; info[2] = (uint32_t)pl.nexpanded; info[3] = (uint32_t)nwide; info[4] = (uint32_t)ck.nwin;
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

    // the tables: the engine's builder on the plan
    MsmSet<AffT> set; size_t table_bytes = 0;
    msm_build_tables<AffT, XyzzT>(set, bases.p, pl, std::vector<uint32_t>(a.rows, a.rows + n), a.c, s, &table_bytes);
    if (nwide) set.digit_bases = a.digit_bases;
    // scratch for this one call
    MsmLaunchOpts opts; opts.per_flat = a.per_flat; opts.per_win = a.per_win;
    const MsmGeometry g = msm_geometry(set.shape(), B, few, opts);
    info[5] = (uint32_t)g.flat_slices; info[6] = (uint32_t)g.flat_per; info[7] = (uint32_t)g.win_slices; info[8] = (uint32_t)g.win_per;
    DevBuf<XyzzT> sum(B), flat(B), pa(g.pa + 1), pb(g.pb + 1), sj(g.sj + 1);
    DevBuf<uint4> fdigits(g.digit_words + 1), wdigits(g.digit_words + 1); DevBuf<uint8_t> gok(g.gok_bytes + 1);
    HIP_CHECK(hipMemsetAsync(sum.p, 0, sum.bytes(), s)); HIP_CHECK(hipMemsetAsync(flat.p, 0, flat.bytes(), s));
    HIP_CHECK(hipMemsetAsync(pa.p, 0, pa.bytes(), s)); HIP_CHECK(hipMemsetAsync(pb.p, 0, pb.bytes(), s)); HIP_CHECK(hipMemsetAsync(sj.p, 0, sj.bytes(), s));
    HIP_CHECK(hipMemsetAsync(fdigits.p, 0, fdigits.bytes(), s)); HIP_CHECK(hipMemsetAsync(wdigits.p, 0, wdigits.bytes(), s)); HIP_CHECK(hipMemsetAsync(gok.p, 0, gok.bytes(), s));
    DevBuf<uint32_t> drows;
    if (set.digit_bases) {      // in the last quotient kernel's place: the digits of digit_rows, laid out for digit_bases bases
        drows.alloc(a.digit_bases); drows.upload(a.digit_rows, a.digit_bases, s);
        launch_msm_recode(MsmRecodeArgs{scalars.p, drows.p, a.mont ? 1 : 0, a.digit_bases, B, a.c, set.nwin, wdigits.p}, s);
    }
    // the call: the engine's launch sequence, then the Horner job it left
    MsmLevels levels; MsmHornerJobs jobs{};
    MsmRun<XyzzT> r{MsmCtx{s, fdigits.p, gok.p, a.plane ? plane.p : nullptr, a.plane ? a.plane_rows : 0u, a.plane ? a.plane_stride : 0u}, scalars.p, a.mont != 0, B, npr, few, pa.p, pb.p, sj.p, flat.p, sum.p};
    r.digits_ready = set.digit_bases != 0; r.opts = opts; r.win_digits = wdigits.p; r.levels = &levels;
    msm_run<AffT, XyzzT>(set, r, jobs);
    if (jobs.n) launch_msm_horner<AffT>(jobs, B, s);
    HIP_CHECK(hipGetLastError());
    auto put_levels = [&](uint32_t at, const std::vector<std::pair<size_t, bool>>& lv) {
        if (lv.size() > 8) refuse("more than eight reduction levels");
        info[at] = (uint32_t)lv.size();
        for (size_t i = 0; i < lv.size(); i++) { info[at + 1 + 2 * i] = (uint32_t)lv[i].first; info[at + 2 + 2 * i] = lv[i].second ? 1u : 0u; }
    };
    put_levels(9, levels.flat); put_levels(26, levels.win);
    info[43] = jobs.n && jobs.job[0].addend ? 1u : 0u;
    // ---- results ----
    DevBuf<fe> d_out(2 * F::WORDS * ck.ncols); DevBuf<uint8_t> d_inf(ck.ncols);
    hipLaunchKernelGGL(k_debug_msm_out<F>, dim3((unsigned)((ck.ncols + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const fe*>(sum.p), ck.ncols, d_out.p, d_inf.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(a.out, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(a.out_inf, d_inf.p, ck.ncols, hipMemcpyDeviceToHost, s));
    const size_t win_words = nwide ? (size_t)set.nwin * ck.noct_w * B * msm_digit_words(a.c) : 0;
    copy_out(a.flat_digits, a.flat_digits_cap, fdigits.p, nflat / 8 * B * sizeof(uint4), info[48], "the flat digits", s);
    copy_out(a.win_digits, a.win_digits_cap, wdigits.p, win_words * sizeof(uint4), info[49], "the windowed digits", s);
    copy_out(a.gok, a.gok_cap, gok.p, pl.nbit / 8 * (few ? MSM_FEW_PROOFS : B / 64), info[50], "gok", s);
    copy_out(a.group_ok, a.group_ok_cap, set.group_ok.p, pl.nbit / 8, info[51], "group_ok", s);
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace

void debug_msm(int device, const gsc_debug_msm_args& a) {
    const Checked ck = check(a);      // every refusal the host can decide comes before a device is asked for
    use_device(device);
    if (a.group == 0) run<G1Aff, G1Xyzz>(a, ck); else run<G2Aff, G2Xyzz>(a, ck);
}

}  // namespace gsc
