// Launchers of the column-sum kernels (k_srs_columns.hip).  Types come from verify_dev.hpp; the host side is srs_columns.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "verify_dev.hpp"

namespace gsc {
// everything on the device.  The host has checked: term_row < the rows' count, term_coeff < the coefficient table's size, the segments
// (srs_columns.hpp cut_columns) inside the term lists.  mag / meta: srs_columns.hpp CoeffTable.
struct ColumnArgs {
    const uint32_t *seg_begin, *seg_end, *col_seg;      // n_segs, n_segs, n_cols + 1 entries
    const uint32_t *term_row, *term_coeff;              // per term
    const uint32_t *mag, *meta;                         // per coefficient id: 8 words, 1 word
    uint32_t n_segs, n_cols;
};
// part: column_part_bytes(n_segs, g2) bytes of scratch; out: n_cols decoded points, the point at infinity flagged
size_t column_part_bytes(uint32_t n_segs, bool g2);
void launch_column_sums(const vfy::VP1* rows, const ColumnArgs& a, void* part, vfy::VP1* out, hipStream_t s);
void launch_column_sums(const vfy::VP2* rows, const ColumnArgs& a, void* part, vfy::VP2* out, hipStream_t s);
}  // namespace gsc
