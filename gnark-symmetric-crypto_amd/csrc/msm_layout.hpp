// Host-side planning of an MSM set (no HIP: builds with a plain compiler): which bases become bit groups, narrow rows, window octets or the
// windowed part, the flat part's order and row geometry, the row-building work items, and msm_geometry: the slice counts of a launch with the
// scratch a call can write.  ONE definition: the planner is called by AlgorithmImpl::build_set (engine_tables.hip) and by the test hook
// gsc_debug_msm (msm_debug.hip); msm_geometry by msm_run (msm_set.hip, the launch sequence of both), by alloc_lane for the lanes' scratch and by the
// hook for its own.  tests/test_msm_layout_host.py holds both against a Python statement of the same rules.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gsc {

// What calibration predicts of the bases of a set, in the key's order.  bits: scalars in {-1, 0, 1}; narrow: rows of narrow_len entries;
// wide: full-width scalars.
struct MsmSorted { std::vector<uint32_t> bits, narrow, narrow_len, wide; };

// status[i] == 2: the point at infinity contributes nothing and is dropped.  cls[row]: 0 / 1 a bit wire, 2 .. 254 the bit length seen, 255 (or a
// row beyond cls) unknown.  A class whose length with the margin exceeds max_bits is wide; so is everything when uniform or without bit groups.
inline MsmSorted msm_sort_bases(const std::vector<uint8_t>& status, const std::vector<uint32_t>& rows, const std::vector<uint8_t>& cls, bool uniform, int bit_groups,
                                int row_margin_bits, int max_bits) {
    MsmSorted s;
    for (size_t i = 0; i < status.size(); i++) {
        if (status[i] == 2) continue;
        const int k = uniform || rows[i] >= cls.size() ? 255 : cls[rows[i]];
        if (uniform || bit_groups <= 0 || k == 255 || k + row_margin_bits > max_bits) s.wide.push_back((uint32_t)i);
        else if (k <= 1) s.bits.push_back((uint32_t)i);
        else { s.narrow.push_back((uint32_t)i); const int lb = k + row_margin_bits; s.narrow_len.push_back(1u << (lb < 0 ? 0 : lb)); }
    }
    return s;
}

// The flat part: [bit groups][narrow rows][padding to an octet][window octets of the expanded wide wires].  Flat base i is 2^shift[i] times the
// key's base src[i], takes scalar row frows[i] and has a table row of len[i] multiples; octwin[o] is the first window of a window octet, else -1.
struct MsmFlatPlan {
    std::vector<uint32_t> src, shift, frows, len; std::vector<int32_t> octwin;
    size_t nbit = 0, nexpanded = 0; int cv = 0;
    std::vector<uint32_t> wide;      // what is left for the windowed kernel
};
// Bits that do not fill an octet are demoted to narrow rows of length 2 (in front of the narrow ones).  Padding slots repeat the first base with the
// always-zero scalar row `zero_row`.  The wide wires are expanded into ceil(nwv / 8) window octets each (digit width cv = expand_cv, or expand_c when
// expand_cv == 0 and there are at most expand_max of them); slots past the nwv windows get shift 0, length 1 and, from the recoder, the digit 0.
// uniform: the set was sorted as all-wide; it has a flat part only when expand_cv > 0 (EVERY base as window octets: the latency-path layout of the
// quotient bases, no Horner pass).  nwv = msm_windows(cv) comes from the caller (kernels.hpp), so that this header needs nothing of the device.
template <class Windows>
inline MsmFlatPlan msm_plan_flat(MsmSorted s, const std::vector<uint32_t>& rows, uint32_t zero_row, bool uniform, int expand_cv, size_t expand_max, int expand_c, Windows windows_of) {
    MsmFlatPlan f;
    if (uniform && expand_cv <= 0) { f.wide = s.wide; return f; }      // uniform full-width scalars (Z): no flat part, every base to the windowed kernel
    while (s.bits.size() % 8) { s.narrow.insert(s.narrow.begin(), s.bits.back()); s.narrow_len.insert(s.narrow_len.begin(), 2u); s.bits.pop_back(); }
    f.src = s.bits;
    f.src.insert(f.src.end(), s.narrow.begin(), s.narrow.end());
    for (uint32_t i : f.src) f.frows.push_back(rows[i]);
    f.len.assign(s.bits.size(), 1u); f.len.insert(f.len.end(), s.narrow_len.begin(), s.narrow_len.end());
    while (f.src.size() % 8) { f.src.push_back(f.src[0]); f.frows.push_back(zero_row); f.len.push_back(1u); }
    f.shift.assign(f.src.size(), 0u); f.octwin.assign(f.src.size() / 8, -1);
    f.wide = s.wide;
    if (!s.wide.empty() && (expand_cv > 0 || s.wide.size() <= expand_max)) {
        f.cv = expand_cv > 0 ? expand_cv : expand_c;
        const int nwv = windows_of(f.cv), octs = (nwv + 7) / 8;
        for (uint32_t w : s.wide) for (int q = 0; q < 8 * octs; q++) {
            f.src.push_back(w); f.frows.push_back(rows[w]); f.shift.push_back(q < nwv ? (uint32_t)(f.cv * q) : 0u); f.len.push_back(q < nwv ? 1u << (f.cv - 1) : 1u);
            if (q % 8 == 0) f.octwin.push_back(q);
        }
        f.nexpanded = s.wide.size(); f.wide.clear();
    }
    f.nbit = s.bits.size();
    return f;
}

// Table entry of every row when they follow each other; returns the entries in all
inline size_t msm_row_offsets(const std::vector<uint32_t>& len, std::vector<uint64_t>& off) {
    off.resize(len.size()); size_t entries = 0;
    for (size_t i = 0; i < len.size(); i++) { off[i] = entries; entries += len[i]; }
    return entries;
}

// Row-building work items (launch_build_rows): `count` <= cap consecutive multiples of base `base` from the `first`-th, written at table entry `entry`
struct MsmRowSeg { uint32_t base, first, count, pad; uint64_t entry; };
inline std::vector<MsmRowSeg> msm_row_segments(const std::vector<uint64_t>& off, const std::vector<uint32_t>& len, uint32_t cap) {
    std::vector<MsmRowSeg> segs;
    for (size_t i = 0; i < len.size(); i++) for (uint32_t f = 0; f < len[i]; f += cap) segs.push_back(MsmRowSeg{(uint32_t)i, f + 1, len[i] - f < cap ? len[i] - f : cap, 0u, off[i] + f});
    return segs;
}

// Waves of an MSM launch = slices x windows x groups of 64 proofs (windows = 1 for the flat kernel).  Slices of up to `most`
// bases (256: few partial sums to reduce, a tail of < 2 % at full batches; measured 64 .. 512: kernel time within 1 %, reductions -3 ms); shorter ones when that would leave fewer than ~8k waves,
// so that a small batch still spreads over the whole chip.  per: a multiple of 8; the slices returned cover the bases and none is empty.
inline size_t msm_slices(size_t nbases, size_t nwin, size_t most, size_t B, size_t& per) {
    const size_t gw = (B / 64) * nwin, want = (8192 + gw - 1) / gw;
    size_t n = (nbases + most - 1) / most; if (n < want) n = want;
    n = (n + 7) & ~(size_t)7;
    per = ((nbases + n - 1) / n + 7) & ~(size_t)7; if (!per) per = 8;
    n = (nbases + per - 1) / per;
    return n ? n : 1;
}
// a single Prove call (lanes = bases): slices of 512 bases — 8 gathers + 6 butterfly additions per wave, and at most 64 partial
// sums per column, which one reduction launch folds
inline void msm_slices_latency(size_t nbases, size_t& nslices, size_t& per) {
    if (nslices > (nbases + 511) / 512) { per = 512; nslices = (nbases + 511) / 512; }
}
// slices of a flat set's latency kernel: lanes = octets, 64 octets per wave
inline size_t msm_flat_few_slices(size_t nflat) { return ((nflat + 7) / 8 + 63) / 64; }

constexpr size_t MSM_REDUCE_FANIN = 32;   // slices per group of a reduction level by proof (launch_msm_reduce, kernels.hpp); a level's output holds ceil(slices / 32) groups
constexpr size_t MSM_FEW_PROOFS = 32;     // layout bound of the latency kernels; the engine's threshold is EngineConfig::few_max
inline size_t msm_digit_words(int c) { return c > 16 ? 2 : 1; }      // 16-byte words per (window, octet, proof) of the windowed digits

// The geometry of one MSM call over a set: the slices the launches take, and what the call can write of its scratch.
// few_wide_nflat: the flat bases of the latency layout of the windowed part (MsmSet::few_wide), 0 = none.
struct MsmShape { size_t nflat = 0, nbit = 0, nwide = 0; int c = 0, nwin = 0; size_t digit_bases = 0, few_wide_nflat = 0; };
// win_slice: bases per slice of the windowed kernel at full batches (measured 64 .. 512: kernel time within 1 %); per_flat / per_win: bases per slice
// whatever the batch (the test hook; per_flat is not read by a latency call), 0 = the choice of msm_slices
struct MsmLaunchOpts { size_t win_slice = 256, per_flat = 0, per_win = 0; };
struct MsmGeometry {
    size_t flat_slices = 0, flat_per = 0, win_slices = 0, win_per = 0;      // what the launches take
    size_t few_wide_slices = 0;      // latency call: the last of flat_slices belong to the latency layout of the windowed part, side by side in the same partial buffer
    size_t pa = 0, pb = 0, sj = 0;   // points: slice partials, the first reduction level's output, the per-window sums
    size_t digit_words = 0, gok_bytes = 0;      // 16-byte digit words, bit-group verdicts
};
inline MsmGeometry msm_geometry(const MsmShape& m, size_t B, bool latency, const MsmLaunchOpts& o = MsmLaunchOpts()) {
    MsmGeometry g;
    auto raise = [](size_t& v, size_t to) { if (to > v) v = to; };
    if (m.nflat) {
        if (latency) { g.flat_per = 512; g.flat_slices = msm_flat_few_slices(m.nflat); }
        else if (o.per_flat) { g.flat_per = o.per_flat; g.flat_slices = (m.nflat + o.per_flat - 1) / o.per_flat; }
        else g.flat_slices = msm_slices(m.nflat, 1, 256, B, g.flat_per);
        g.digit_words = m.nflat / 8 * B;
        g.gok_bytes = m.nbit / 8 * (B / 64); raise(g.gok_bytes, m.nbit / 8 * MSM_FEW_PROOFS);
    }
    if (latency && m.few_wide_nflat) {
        g.flat_per = 512; g.few_wide_slices = msm_flat_few_slices(m.few_wide_nflat); g.flat_slices += g.few_wide_slices;
        raise(g.digit_words, (m.few_wide_nflat + 7) / 8 * B);
    }
    if (m.nwide) {
        if (o.per_win) { g.win_per = o.per_win; g.win_slices = (m.nwide + o.per_win - 1) / o.per_win; }
        else { g.win_slices = msm_slices(m.nwide, (size_t)m.nwin, o.win_slice, B, g.win_per); if (latency) msm_slices_latency(m.nwide, g.win_slices, g.win_per); }
        g.sj = B * (size_t)m.nwin;
        raise(g.digit_words, (size_t)m.nwin * (((m.digit_bases ? m.digit_bases : m.nwide) + 7) / 8) * B * msm_digit_words(m.c));
    }
    g.pa = g.flat_slices * B; raise(g.pa, g.win_slices * g.sj);
    g.pb = (g.flat_slices + MSM_REDUCE_FANIN - 1) / MSM_REDUCE_FANIN * B; raise(g.pb, (g.win_slices + MSM_REDUCE_FANIN - 1) / MSM_REDUCE_FANIN * g.sj);
    return g;
}

}  // namespace gsc
