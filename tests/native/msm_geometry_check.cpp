// Host build of the MSM's geometry helpers: xcd_slice and slice_bounds (csrc/msm_dev.hpp), msm_slices and the layout planner
// (csrc/msm_layout.hpp), msm_reduce_groups / msm_reduce_by_proof (csrc/kernels.hpp).  tests/test_msm_layout_host.py runs it.
//   no argument: the self-check below; prints the first violated property and returns 1
//   "layout"   : the planner on a description from stdin, its plan to stdout
//     stdin : n, uniform, bit_groups, margin, max_bits, expand_cv, expand_max, expand_c, zero_row, ncls (int32 LE) | status: n bytes | rows: n u32 | cls: ncls bytes
//     stdout: nbit, nexpanded, cv, nflat, noct, nwide, nsegs (u32) | src, shift, frows, len: nflat u32 each | octwin: noct i32 | wide: nwide u32 |
//             off: nflat u64 | entries u64
//   "geometry" : msm_geometry (csrc/msm_layout.hpp) on the calls of stdin, one per line, its answer to stdout, one line each
//     stdin : nflat nbit nwide c nwin digit_bases few_wide_nflat B latency win_slice per_flat per_win
//     stdout: flat_slices flat_per win_slices win_per few_wide_slices pa pb sj digit_words gok_bytes
#include "msm_dev.hpp"
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include <vector>
using namespace gsc;

#define REQUIRE(cond, ...) do { if (!(cond)) { printf("violated: %s: ", #cond); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static int self_check() {
    // xcd_slice: a bijection from [0, nslices * per_slice) onto (slice, rem); below the last multiple of eight slices every workgroup of a slice has the
    // same id mod 8 (one XCD), the tail slices are taken in order
    for (size_t ns = 1; ns <= 40; ns++) for (size_t ps = 1; ps <= 130; ps++) {
        std::vector<uint8_t> seen(ns * ps, 0); std::vector<int> xcd(ns, -1);
        const size_t S8 = ns & ~(size_t)7;
        for (size_t L = 0; L < ns * ps; L++) {
            const SliceRem sr = xcd_slice(L, ns, ps);
            REQUIRE(sr.slice < ns && sr.rem < ps, "ns %zu ps %zu L %zu -> (%zu, %zu)", ns, ps, L, sr.slice, sr.rem);
            REQUIRE(!seen[sr.slice * ps + sr.rem], "ns %zu ps %zu L %zu: (%zu, %zu) twice", ns, ps, L, sr.slice, sr.rem);
            seen[sr.slice * ps + sr.rem] = 1;
            if (sr.slice < S8) {
                REQUIRE(xcd[sr.slice] < 0 || xcd[sr.slice] == (int)(L & 7), "ns %zu ps %zu: slice %zu on two XCDs", ns, ps, sr.slice);
                xcd[sr.slice] = (int)(L & 7);
            } else REQUIRE(L >= S8 * ps && sr.slice == L / ps && sr.rem == L % ps, "ns %zu ps %zu L %zu: the tail is not in order", ns, ps, L);
        }
        if (ns >= 8) for (size_t sl = 0; sl < S8; sl++) REQUIRE(xcd[sl] == (int)(sl & 7), "ns %zu ps %zu: slice %zu on XCD %d", ns, ps, sl, xcd[sl]);
    }
    // slice_bounds: consecutive slices of `per` partition [0, nbases); slices past the end are empty
    for (size_t per : {8, 16, 64, 256, 512}) for (size_t nb = 0; nb <= 1100; nb++) {
        size_t next = 0;
        const size_t ns = (nb + per - 1) / per;
        for (size_t sl = 0; sl < ns + 2; sl++) {
            const BaseRange b = slice_bounds(sl, per, nb);
            REQUIRE(b.k0 == next && b.k1 >= b.k0 && b.k1 <= nb && b.k1 - b.k0 <= per, "per %zu nbases %zu slice %zu: [%zu, %zu)", per, nb, sl, b.k0, b.k1);
            REQUIRE(sl >= ns || b.k1 > b.k0, "per %zu nbases %zu: slice %zu is empty", per, nb, sl);
            REQUIRE(b.k0 % 8 == 0 || b.k0 == nb, "per %zu nbases %zu slice %zu starts inside an octet", per, nb, sl);
            next = b.k1;
        }
        REQUIRE(next == nb, "per %zu nbases %zu: covered %zu", per, nb, next);
    }
    // msm_slices: per a multiple of 8, the slices cover the bases and none is empty
    for (size_t nwin : {1, 16, 17, 32, 43, 64}) for (size_t most : {64, 256, 512}) for (size_t B : {64, 128, 1024, 8192}) {
        std::vector<size_t> sizes;
        for (size_t nb = 0; nb <= 1200; nb++) sizes.push_back(nb);
        for (size_t nb : {4095, 4096, 4097, 32767, 32768, 65535, 131071, 131072}) sizes.push_back(nb);
        for (size_t nb : sizes) {
            size_t per = 0; const size_t n = msm_slices(nb, nwin, most, B, per);
            REQUIRE(per >= 8 && per % 8 == 0 && n >= 1, "nbases %zu nwin %zu most %zu B %zu: per %zu n %zu", nb, nwin, most, B, per, n);
            REQUIRE(n * per >= nb && (nb == 0 ? n == 1 : (n - 1) * per < nb), "nbases %zu nwin %zu most %zu B %zu: %zu slices of %zu", nb, nwin, most, B, n, per);
            size_t nl = n, pl = per; msm_slices_latency(nb, nl, pl);
            REQUIRE(pl % 8 == 0 && nl * pl >= nb && nl <= n && (nb == 0 || (nl - 1) * pl < nb), "latency: nbases %zu: %zu slices of %zu", nb, nl, pl);
        }
    }
    for (size_t nf = 0; nf <= 9000; nf += 8) REQUIRE(msm_flat_few_slices(nf) * 512 >= nf && (nf == 0 || (msm_flat_few_slices(nf) - 1) * 512 < nf), "flat latency slices of %zu bases", nf);
    // the reduction levels iterate to one group; the by-proof kernel only where its grid has a whole wave per group of proofs
    for (size_t batch : {64, 128, 64 * 43, 128 * 17, 8192, 8192 * 17}) for (size_t ns = 1; ns <= 5000; ns++) {
        size_t cur = ns; int levels = 0;
        for (;;) {
            const size_t g = msm_reduce_groups(cur, batch), f = msm_reduce_by_proof(cur, batch) ? MSM_REDUCE_FANIN : 64;
            REQUIRE(g >= 1 && g * f >= cur && (g - 1) * f < cur, "nslices %zu batch %zu: %zu groups of %zu", cur, batch, g, f);
            REQUIRE(g * batch <= ((cur + MSM_REDUCE_FANIN - 1) / MSM_REDUCE_FANIN) * batch, "nslices %zu batch %zu: more groups than the output holds", cur, batch);
            levels++;
            if (g == 1) break;
            REQUIRE(g < cur && levels < 8, "nslices %zu batch %zu: no progress", ns, batch);
            cur = g;
        }
    }
    // the row-building work items tile every row
    {
        const std::vector<uint32_t> len = {1, 2, 255, 256, 257, 512, 16384, 1, 700};
        std::vector<uint64_t> off; const size_t entries = msm_row_offsets(len, off);
        std::vector<uint8_t> hit(entries, 0);
        for (const MsmRowSeg& sg : msm_row_segments(off, len, 256)) {
            REQUIRE(sg.count >= 1 && sg.count <= 256 && sg.base < len.size() && sg.first >= 1 && sg.first + sg.count - 1 <= len[sg.base], "segment of base %u: %u from %u", sg.base, sg.count, sg.first);
            REQUIRE(sg.entry == off[sg.base] + sg.first - 1, "segment of base %u at entry %llu", sg.base, (unsigned long long)sg.entry);
            for (uint32_t d = 0; d < sg.count; d++) { REQUIRE(!hit[sg.entry + d], "entry %llu twice", (unsigned long long)(sg.entry + d)); hit[sg.entry + d] = 1; }
        }
        for (size_t e = 0; e < entries; e++) REQUIRE(hit[e], "entry %zu not built", e);
    }
    printf("ok\n");
    return 0;
}

static int layout() {
    int32_t h[10];
    if (fread(h, 4, 10, stdin) != 10 || h[0] < 0 || h[9] < 0) return 2;
    const size_t n = (size_t)h[0], ncls = (size_t)h[9];
    std::vector<uint8_t> status(n), cls(ncls); std::vector<uint32_t> rows(n);
    if ((n && (fread(status.data(), 1, n, stdin) != n || fread(rows.data(), 4, n, stdin) != n)) || (ncls && fread(cls.data(), 1, ncls, stdin) != ncls)) return 2;
    const bool uniform = h[1] != 0;
    const MsmFlatPlan p = msm_plan_flat(msm_sort_bases(status, rows, cls, uniform, h[2], h[3], h[4]), rows, (uint32_t)h[8], uniform, h[5], (size_t)h[6], h[7], msm_windows);
    std::vector<uint64_t> off; const uint64_t entries = msm_row_offsets(p.len, off);
    const uint32_t head[7] = {(uint32_t)p.nbit, (uint32_t)p.nexpanded, (uint32_t)p.cv, (uint32_t)p.src.size(), (uint32_t)p.octwin.size(), (uint32_t)p.wide.size(),
                              (uint32_t)msm_row_segments(off, p.len, 256).size()};
    fwrite(head, 4, 7, stdout);
    auto put = [](const void* v, size_t size, size_t count) { if (count) fwrite(v, size, count, stdout); };      // (an empty vector's data() may be null)
    for (const std::vector<uint32_t>* v : {&p.src, &p.shift, &p.frows, &p.len}) put(v->data(), 4, v->size());
    put(p.octwin.data(), 4, p.octwin.size()); put(p.wide.data(), 4, p.wide.size());
    put(off.data(), 8, off.size()); put(&entries, 8, 1);
    return 0;
}

static int geometry() {
    unsigned long long v[12];
    for (;;) {
        int got = 0;
        while (got < 12 && scanf("%llu", &v[got]) == 1) got++;
        if (!got) return 0;
        if (got != 12) return 2;
        MsmShape m; m.nflat = v[0]; m.nbit = v[1]; m.nwide = v[2]; m.c = (int)v[3]; m.nwin = (int)v[4]; m.digit_bases = v[5]; m.few_wide_nflat = v[6];
        MsmLaunchOpts o; o.win_slice = v[9]; o.per_flat = v[10]; o.per_win = v[11];
        const MsmGeometry g = msm_geometry(m, v[7], v[8] != 0, o);
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", g.flat_slices, g.flat_per, g.win_slices, g.win_per, g.few_wide_slices, g.pa, g.pb, g.sj, g.digit_words, g.gok_bytes);
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "layout")) return layout();
    if (argc > 1 && !strcmp(argv[1], "geometry")) return geometry();
    return self_check();
}
