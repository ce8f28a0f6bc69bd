// Column sums of a sparse matrix over a vector of group elements (srs_columns.hpp): out[w] = sum over the terms of column
// w of c P[row], in G1 or G2, with the exact group law throughout (two terms of a column may name the same row; a coefficient and its
// negative may cancel; an empty column is the point at infinity).
//   k_srs_col_segments<P>  one wave per segment of at most kColSegTerms terms, lanes striding over the terms: a lane multiplies its points by
//                          their coefficients — sign and magnitude: +-1 costs nothing, a small |c| a short double-and-add, all public, so
//                          the code branches on the bits — and adds them up; block_sum (block_sum.hpp) adds the lanes.
//   k_srs_col_finish<P>    one thread per column: the sum of its segments, affine.
// Columns of an R1CS are skewed (the ONE wire and the bit sums are thousands of terms long, the typical column a handful), hence the
// segments: no wave walks a long column alone, and a short one costs a single wave whose idle lanes skip the loop.
#include "srs_columns_kernels.hpp"
#include "srs_columns.hpp"
#include "block_sum.hpp"

namespace gsc {
using namespace vfy;

namespace {

template <class P> struct ColGroup;
template <> struct ColGroup<VP1> { using F = bn254::Fp29f; };
template <> struct ColGroup<VP2> { using F = bn254::Fp2x; };

DEVFN VP1 col_affine(const bn254::Xyzz9<bn254::Fp29f>& p) { return g1_affine(p); }
DEVFN VP2 col_affine(const bn254::Xyzz9<bn254::Fp2x>& p) { return g2_affine(p); }

// |c| P by double-and-add from the magnitude's top bit (bits >= 1), negated when c's shorter form is r - |c|
template <class F>
DEVFN bn254::Xyzz9<F> col_term(const bn254::Aff9<F>& a, const uint32_t* mag, uint32_t meta) {
    using C = bn254::Curve9<F>;
    const int bits = (int)(meta & 0xFFFFu);
    bn254::Xyzz9<F> acc = C::from_aff(a);
    for (int i = bits - 2; i >= 0; i--) {
        acc = C::dbl(acc);
        if ((mag[i >> 5] >> (i & 31)) & 1u) acc = C::template madd<true>(acc, a);
    }
    if (meta >> 16) acc.y = F::norm(F::neg(acc.y));
    return acc;
}

template <class P>
__global__ __launch_bounds__(srs::kColLanes) void k_srs_col_segments(const P* rows, const uint32_t* seg_begin, const uint32_t* seg_end, const uint32_t* term_row,
                                                                     const uint32_t* term_coeff, const uint32_t* mag, const uint32_t* meta,
                                                                     bn254::Xyzz9<typename ColGroup<P>::F>* part) {
    using F = typename ColGroup<P>::F;
    using C = bn254::Curve9<F>;
    __shared__ bn254::Xyzz9<F> red[srs::kColLanes];
    const uint32_t end = seg_end[blockIdx.x];
    bn254::Xyzz9<F> acc = C::infinity();
    for (uint32_t i = seg_begin[blockIdx.x] + threadIdx.x; i < end; i += srs::kColLanes) {
        const uint32_t id = term_coeff[i], m = meta[id];
        const P p = rows[term_row[i]];
        if (p.inf || !(m & 0xFFFFu)) continue;                         // c = 0, or a row that is the point at infinity
        acc = C::add(acc, col_term<F>(bn254::Aff9<F>{p.x, p.y}, mag + 8 * (size_t)id, m));
    }
    const bn254::Xyzz9<F> total = block_sum<(int)srs::kColLanes>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

template <class P>
__global__ __launch_bounds__(srs::kColsPerBlock) void k_srs_col_finish(const bn254::Xyzz9<typename ColGroup<P>::F>* part, const uint32_t* col_seg, uint32_t n_cols, P* out) {
    using C = bn254::Curve9<typename ColGroup<P>::F>;
    const uint32_t w = blockIdx.x * srs::kColsPerBlock + threadIdx.x;
    if (w >= n_cols) return;
    auto acc = C::infinity();
    for (uint32_t s = col_seg[w]; s < col_seg[w + 1]; s++) acc = C::add(acc, part[s]);
    out[w] = col_affine(acc);
}

template <class P> void column_sums(const P* rows, const ColumnArgs& a, void* part, P* out, hipStream_t s) {
    using X = bn254::Xyzz9<typename ColGroup<P>::F>;
    if (a.n_segs) hipLaunchKernelGGL(k_srs_col_segments<P>, dim3(a.n_segs), dim3(srs::kColLanes), 0, s, rows, a.seg_begin, a.seg_end, a.term_row, a.term_coeff, a.mag, a.meta, static_cast<X*>(part));
    if (a.n_cols) hipLaunchKernelGGL(k_srs_col_finish<P>, dim3((a.n_cols + srs::kColsPerBlock - 1) / srs::kColsPerBlock), dim3(srs::kColsPerBlock), 0, s, (const X*)part, a.col_seg, a.n_cols, out);
}

}  // namespace

size_t column_part_bytes(uint32_t n_segs, bool g2) { return (size_t)(n_segs ? n_segs : 1) * (g2 ? sizeof(bn254::Xyzz9<bn254::Fp2x>) : sizeof(bn254::Xyzz9<bn254::Fp29f>)); }
void launch_column_sums(const VP1* rows, const ColumnArgs& a, void* part, VP1* out, hipStream_t s) { column_sums<VP1>(rows, a, part, out, s); }
void launch_column_sums(const VP2* rows, const ColumnArgs& a, void* part, VP2* out, hipStream_t s) { column_sums<VP2>(rows, a, part, out, s); }

}  // namespace gsc
