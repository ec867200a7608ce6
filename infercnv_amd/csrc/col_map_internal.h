// K26: the check of a column map, shared by the two column-selected readers (their entries are in table_parse_api.hip and
// sparse_counts_api.hip; the kernels are in table_cols_kernels.hip).  DESIGN.md section 4 K26.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icnv {

constexpr int CM_E_RANGE = 1, CM_E_REPEAT = 2, CM_E_UNHIT = 3;
constexpr int32_t CM_UNHIT = 0x7f7f7f7f;

// col_map_dev [n_cols] (DEVICE): every entry in -1 .. n_cols_out - 1 and every output column hit exactly once, or ICNV_ERR_ARG
// with "<who>: ..." naming the first offending entry (a range error before a repeat before an unhit column).  Synchronises.
int check_col_map(const int32_t *col_map_dev, int64_t n_cols, int64_t n_cols_out, const char *who, hipStream_t s);

}  // namespace icnv
