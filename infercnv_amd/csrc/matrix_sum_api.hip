// C ABI of K23 (include/icnv.h "exact sum of a matrix"): validation, the launch, the download of the workgroups' records and
// the host's carry and rounding (matrix_sum_internal.h).  Kernel: matrix_sum_kernels.hip.  DESIGN.md section 4 K23.
#include <vector>

#include "icnv_internal.h"
#include "matrix_sum_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

int ms_check(const double *x, int64_t ld, int64_t G, int64_t C, const double *sum) {
    if (!x || !sum) ICNV_FAIL(ICNV_ERR_ARG, "matrix_sum: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, "matrix_sum: bad matrix dimensions");
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_matrix_sum_dev(const double *x, int64_t ld, int64_t G, int64_t C, double *sum, void *stream) {
    int rc;
    if ((rc = ms_check(x, ld, G, C, sum))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_max = matrix_sum_workgroups(ld, G, C);
    if (n_max < 1) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "matrix_sum: the matrix needs more than 2^31 - 1 workgroups");
    DevBuf d_records;
    if ((rc = d_records.alloc((size_t)n_max * MS_SLOTS * sizeof(int64_t)))) return rc;
    int64_t n_wg = 0;
    if ((rc = launch_matrix_sum(x, ld, G, C, d_records.as<int64_t>(), &n_wg, s))) return rc;
    std::vector<int64_t> records((size_t)n_wg * MS_SLOTS);
    ICNV_HIP(hipMemcpyAsync(records.data(), d_records.p, records.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    *sum = ms_finish(records.data(), n_wg);
    return ICNV_OK;
}

int icnv_matrix_sum(const double *x, int64_t ld, int64_t G, int64_t C, double *sum) {
    int rc;
    if ((rc = ms_check(x, ld, G, C, sum))) return rc;
    if (ld == G) {
        MatrixLease in;
        if ((rc = acquire_input(x, G * C, nullptr, in))) return rc;
        return icnv_matrix_sum_dev(in.dev, G, G, C, sum, nullptr);
    }
    // rows that lie apart: only the G values of each row are read from the host, so the padding is never touched
    DevBuf d_x;
    if ((rc = d_x.alloc((size_t)G * (size_t)C * sizeof(double)))) return rc;
    ICNV_HIP(hipMemcpy2DAsync(d_x.p, (size_t)G * sizeof(double), x, (size_t)ld * sizeof(double), (size_t)G * sizeof(double), (size_t)C,
                              hipMemcpyHostToDevice, nullptr));
    rc = icnv_matrix_sum_dev(d_x.as<double>(), G, G, C, sum, nullptr);
    return rc;
}

}  // extern "C"
