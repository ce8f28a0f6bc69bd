// Clearing key-derived buffers (wipe_plan.hpp says which and when): k_wipe writes the idle image of a list of regions in one launch,
// k_scan_idle counts the bytes of a region that differ from it.
//
// A region is rows x width bytes, rows `pitch` apart: a whole buffer of many GB is one long row, "columns < n of every 2 KiB row" is a
// few ten thousand short ones.  Both are cut into units of at most WIPE_UNIT_BYTES of one row (long rows) or of 256 / lanes_per_row whole
// rows (short rows), and the blocks of a bounded grid walk the units of the whole list with a grid stride: a launch beside the Z sum takes
// few wave slots, and descriptors of very different sizes still spread evenly.  Inside a unit a lane writes one 16-byte vector (plain
// stores: the lines are not read again, but whether a nontemporal store gains anything on a pure fill is unmeasured) and the unaligned
// head and tail go out byte by byte.  Every offset is 64 bits wide: the Z digits of a full lane pass 2^32 bytes.
#include "kernels.hpp"

namespace gsc {

namespace {
constexpr uint32_t WIPE_THREADS = 256;

// where unit u of descriptor d lies: the first row, the byte range [lo, hi) of each of its rows, the rows it holds
struct UnitGeom { uint64_t chunks_per_row; uint32_t lanes_per_row, rows_per_unit; };
__host__ __device__ inline UnitGeom unit_geom(const WipeDesc& d) {
    UnitGeom g;
    if (d.width > WIPE_UNIT_BYTES / 2) { g.chunks_per_row = (d.width + WIPE_UNIT_BYTES - 1) / WIPE_UNIT_BYTES; g.lanes_per_row = WIPE_THREADS; g.rows_per_unit = 1; return g; }
    // short rows: enough lanes for the row's vectors plus one (a row that starts off a 16-byte boundary straddles one more), a power of two
    uint32_t need = (uint32_t)((d.width + 15) / 16) + 1, l = 2;
    while (l < need) l <<= 1;
    g.chunks_per_row = 1; g.lanes_per_row = l; g.rows_per_unit = WIPE_THREADS / l;
    return g;
}
__host__ __device__ inline uint64_t unit_count(const WipeDesc& d) {
    if (!d.rows || !d.width) return 0;
    const UnitGeom g = unit_geom(d);
    return g.rows_per_unit > 1 ? (d.rows + g.rows_per_unit - 1) / g.rows_per_unit : d.rows * g.chunks_per_row;
}

// what this lane covers of unit u: bytes [p, e) of one row, and the image byte of that row; false: nothing
__device__ inline bool lane_span(const WipeDesc& d, uint64_t u, uint32_t t, uint8_t*& p, uint8_t*& e, uint32_t& slot, uint32_t& lanes, uint8_t& val) {
    const UnitGeom g = unit_geom(d);
    uint64_t row, lo, hi;
    if (g.rows_per_unit > 1) { row = u * g.rows_per_unit + t / g.lanes_per_row; lo = 0; hi = d.width; }
    else { row = u / g.chunks_per_row; lo = (u % g.chunks_per_row) * WIPE_UNIT_BYTES; hi = lo + WIPE_UNIT_BYTES < d.width ? lo + WIPE_UNIT_BYTES : d.width; }
    if (row >= d.rows) return false;
    slot = t % g.lanes_per_row; lanes = g.lanes_per_row;
    p = d.base + row * d.pitch + lo; e = d.base + row * d.pitch + hi;
    val = d.cls && d.cls[row % d.cls_period] ? (uint8_t)WS_PLANE_WIDE : (uint8_t)0;
    return true;
}
}  // namespace

__global__ __launch_bounds__(256) void k_wipe(const WipeList list) {
    for (uint64_t u = blockIdx.x; u < list.first[list.n]; u += gridDim.x) {
        uint32_t k = 0;
        while (u >= list.first[k + 1]) k++;      // (uniform over the block; at most WIPE_MAX_DESCS steps)
        uint8_t *p, *e; uint32_t slot, lanes; uint8_t val;
        if (!lane_span(list.d[k], u - list.first[k], threadIdx.x, p, e, slot, lanes, val)) continue;
        const uint64_t head = (16 - ((uint64_t)p & 15)) & 15;
        if ((uint64_t)(e - p) <= head) { for (uint8_t* q = p + slot; q < e; q += lanes) *q = val; continue; }      // no aligned vector inside
        uint8_t* const a0 = p + head; uint8_t* const a1 = a0 + ((uint64_t)(e - a0) & ~(uint64_t)15);
        const uint32_t w = val * 0x01010101u; const uint4 v = make_uint4(w, w, w, w);
        for (uint8_t* q = a0 + 16 * (uint64_t)slot; q < a1; q += 16 * (uint64_t)lanes) *reinterpret_cast<uint4*>(q) = v;
        for (uint8_t* q = p + slot; q < a0; q += lanes) *q = val;
        for (uint8_t* q = a1 + slot; q < e; q += lanes) *q = val;
    }
}

__device__ inline uint32_t bytes_off(uint32_t word, uint32_t image) {
    const uint32_t x = word ^ image;
    return ((x & 0xFFu) != 0) + ((x & 0xFF00u) != 0) + ((x & 0xFF0000u) != 0) + ((x & 0xFF000000u) != 0);
}

__global__ __launch_bounds__(256) void k_scan_idle(const WipeDesc d, unsigned long long* __restrict__ counter) {
    __shared__ unsigned long long part[WIPE_THREADS / 64];
    unsigned long long off = 0;
    const uint64_t units = unit_count(d);
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        uint8_t *p, *e; uint32_t slot, lanes; uint8_t val;
        if (!lane_span(d, u, threadIdx.x, p, e, slot, lanes, val)) continue;
        const uint64_t head = (16 - ((uint64_t)p & 15)) & 15;
        if ((uint64_t)(e - p) <= head) { for (const uint8_t* q = p + slot; q < e; q += lanes) off += *q != val; continue; }
        uint8_t* const a0 = p + head; uint8_t* const a1 = a0 + ((uint64_t)(e - a0) & ~(uint64_t)15);
        const uint32_t w = val * 0x01010101u;
        for (const uint8_t* q = a0 + 16 * (uint64_t)slot; q < a1; q += 16 * (uint64_t)lanes) {
            const uint4 v = *reinterpret_cast<const uint4*>(q);
            off += bytes_off(v.x, w) + bytes_off(v.y, w) + bytes_off(v.z, w) + bytes_off(v.w, w);
        }
        for (const uint8_t* q = p + slot; q < a0; q += lanes) off += *q != val;
        for (const uint8_t* q = a1 + slot; q < e; q += lanes) off += *q != val;
    }
    for (int s = 32; s; s >>= 1) off += __shfl_down(off, s, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = off;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (uint32_t k = 0; k < WIPE_THREADS / 64; k++) sum += part[k];
        if (sum) atomicAdd(counter, sum);
    }
}

static WipeDesc normalised(WipeDesc d) {
    // rows that touch each other are one long row (not a plane image: its rows differ)
    if (!d.cls && d.rows > 1 && d.pitch == d.width) { d.width *= d.rows; d.pitch = d.width; d.rows = 1; }
    return d;
}

void launch_wipe(const WipeDesc* descs, size_t n, unsigned max_blocks, hipStream_t s) {
    if (!max_blocks) max_blocks = WIPE_GRID_DEFAULT;
    for (size_t at = 0; at < n;) {
        WipeList list; list.n = 0; list.first[0] = 0;
        for (; at < n && list.n < WIPE_MAX_DESCS; at++) {
            const WipeDesc d = normalised(descs[at]);
            const uint64_t units = unit_count(d);
            if (!units) continue;
            list.d[list.n] = d; list.first[list.n + 1] = list.first[list.n] + units; list.n++;
        }
        const uint64_t total = list.first[list.n];
        if (!total) continue;
        hipLaunchKernelGGL(k_wipe, dim3((unsigned)(total < max_blocks ? total : max_blocks)), dim3(WIPE_THREADS), 0, s, list);
    }
}

void launch_scan_idle(const WipeDesc& desc, unsigned long long* counter, hipStream_t s) {
    const WipeDesc d = normalised(desc);
    const uint64_t units = unit_count(d);
    if (!units) return;
    hipLaunchKernelGGL(k_scan_idle, dim3((unsigned)(units < WIPE_GRID_SCAN ? units : WIPE_GRID_SCAN)), dim3(WIPE_THREADS), 0, s, d, counter);
}

}  // namespace gsc
