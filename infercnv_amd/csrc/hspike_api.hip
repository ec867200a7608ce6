// C ABI of K15 (include/icnv.h "hidden spike-in"): validation, the chunk plan of the group gene tables, the uploads of the
// splines and the means of the simulation.  Kernels: hspike_kernels.hip.  DESIGN.md section 4 K15.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "hspike_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

int tables_validate(const void *expr, int64_t G, int64_t C, int64_t ld, const int32_t *cell_idx, const int32_t *cell_off,
                    int32_t n_grp, const void *m, const void *v, const void *nzero) {
    if (!expr || !cell_idx || !cell_off || !m || !v || !nzero) ICNV_FAIL(ICNV_ERR_ARG, "group_gene_tables: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, "group_gene_tables: bad matrix dimensions");
    if (n_grp < 1 || n_grp > 65535) ICNV_FAIL(ICNV_ERR_ARG, "group_gene_tables: n_grp must be in 1 .. 65535");
    if (cell_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "group_gene_tables: offsets must start at 0");
    for (int32_t q = 0; q < n_grp; ++q)
        if (cell_off[q + 1] <= cell_off[q]) ICNV_FAIL(ICNV_ERR_ARG, "group_gene_tables: group " + std::to_string(q) + " is empty");
    for (int64_t i = 0; i < cell_off[n_grp]; ++i)
        if (cell_idx[i] < 0 || cell_idx[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "group_gene_tables: cell index out of range");
    return ICNV_OK;
}

int spline_validate(const char *name, const double *knots, const double *coef, int32_t nk, double xmin, double range) {
    const std::string who = std::string("hspike_simulate: ") + name + " spline: ";
    if (!knots || !coef) ICNV_FAIL(ICNV_ERR_ARG, who + "null argument");
    if (nk < 4) ICNV_FAIL(ICNV_ERR_ARG, who + "nk must be >= 4, got " + std::to_string(nk));
    if (!std::isfinite(xmin) || !std::isfinite(range) || !(range > 0.0)) ICNV_FAIL(ICNV_ERR_ARG, who + "xmin must be finite and range finite and > 0");
    for (int32_t j = 0; j < nk; ++j)
        if (!std::isfinite(coef[j])) ICNV_FAIL(ICNV_ERR_ARG, who + "coefficient " + std::to_string(j) + " is not finite");
    for (int32_t j = 0; j < 4; ++j)
        if (knots[j] != 0.0 || knots[nk + j] != 1.0) ICNV_FAIL(ICNV_ERR_ARG, who + "the end knots must be 0 and 1, four times each");
    for (int32_t j = 3; j < nk; ++j)
        if (!(knots[j] < knots[j + 1])) ICNV_FAIL(ICNV_ERR_ARG, who + "the interior knots must increase strictly");
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_group_gene_tables_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *cell_idx, const int32_t *cell_off,
                               int32_t n_grp, double *m, double *v, int32_t *nzero, void *stream) {
    int rc = tables_validate(expr, G, C, ld, cell_idx, cell_off, n_grp, m, v, nzero);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::vector<HsChunk> chunks;
    std::vector<int64_t> chunk_off((size_t)n_grp + 1, 0), coff((size_t)n_grp + 1);
    for (int32_t q = 0; q < n_grp; ++q) {
        for (int64_t b = cell_off[q]; b < cell_off[q + 1]; b += HS_CHUNK)
            chunks.push_back(HsChunk{q, b, std::min<int64_t>(b + HS_CHUNK, cell_off[q + 1])});
        chunk_off[q + 1] = (int64_t)chunks.size();
    }
    for (int32_t q = 0; q <= n_grp; ++q) coff[q] = cell_off[q];
    const int64_t n_chunks = (int64_t)chunks.size(), tiles = (G + 255) / 256;
    if (tiles > 65535 || tiles * n_chunks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "group_gene_tables: too many (gene tile, cell chunk) pairs");
    DevBuf d_idx, d_chunks, d_choff, d_coff, d_part, d_nz;
    if ((rc = upload(d_idx, cell_idx, (size_t)cell_off[n_grp], s)) || (rc = upload(d_chunks, chunks.data(), chunks.size(), s)) ||
        (rc = upload(d_choff, chunk_off.data(), chunk_off.size(), s)) || (rc = upload(d_coff, coff.data(), coff.size(), s)) ||
        (rc = d_part.alloc((size_t)n_chunks * 3 * G * sizeof(double))) || (rc = d_nz.alloc((size_t)n_chunks * G * sizeof(int32_t))))
        return rc;
    HsTables a{};
    a.x = expr; a.ld = ld; a.cell_idx = d_idx.as<int32_t>(); a.chunks = d_chunks.as<HsChunk>(); a.chunk_off = d_choff.as<int64_t>();
    a.cell_off = d_coff.as<int64_t>(); a.G = (int32_t)G; a.n_grp = n_grp; a.n_chunks = n_chunks; a.part = d_part.as<double>();
    a.part_nz = d_nz.as<int32_t>(); a.m = m; a.v = v; a.nzero = nzero;
    if ((rc = launch_hs_tables(a, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));   // the host vectors and the pool blocks outlive the kernels
    return ICNV_OK;
}

int icnv_group_gene_tables(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off, int32_t n_grp,
                           double *m, double *v, int32_t *nzero) {
    int rc = tables_validate(expr, G, C, G, cell_idx, cell_off, n_grp, m, v, nzero);
    if (rc) return rc;
    const size_t n = (size_t)n_grp * G;
    MatrixLease in;
    DevBuf d_m, d_v, d_nz;
    if ((rc = acquire_input(expr, G * C, nullptr, in)) || (rc = d_m.alloc(n * sizeof(double))) || (rc = d_v.alloc(n * sizeof(double))) ||
        (rc = d_nz.alloc(n * sizeof(int32_t))))
        return rc;
    if ((rc = icnv_group_gene_tables_dev(in.dev, G, C, G, cell_idx, cell_off, n_grp, d_m.as<double>(), d_v.as<double>(),
                                         d_nz.as<int32_t>(), nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(m, d_m.p, n * sizeof(double), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(v, d_v.p, n * sizeof(double), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(nzero, d_nz.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_hspike_simulate_dev(const double *means, int64_t n_genes, int32_t num_cells, int32_t n_mat, const double *var_knots,
                             const double *var_coef, int32_t var_nk, double var_xmin, double var_range, const double *p0_knots,
                             const double *p0_coef, int32_t p0_nk, double p0_xmin, double p0_range, uint64_t seed,
                             const uint64_t *tokens, double *out, void *stream) {
    if (!means || !tokens || !out) ICNV_FAIL(ICNV_ERR_ARG, "hspike_simulate: null argument");
    if (n_genes < 1 || n_genes > 0x7fffffff || num_cells < 1 || n_mat < 1 || n_mat > 65535)
        ICNV_FAIL(ICNV_ERR_ARG, "hspike_simulate: n_genes and num_cells must be >= 1, n_mat in 1 .. 65535");
    int rc;
    if ((rc = spline_validate("variance", var_knots, var_coef, var_nk, var_xmin, var_range)) ||
        (rc = spline_validate("p0", p0_knots, p0_coef, p0_nk, p0_xmin, p0_range)))
        return rc;
    const size_t n_means = (size_t)n_mat * n_genes;
    for (size_t i = 0; i < n_means; ++i) {
        if (!std::isfinite(means[i]))
            ICNV_FAIL(ICNV_ERR_ARG, "hspike_simulate: mean " + std::to_string(i % n_genes) + " of matrix " + std::to_string(i / n_genes) + " is not finite");
        if (means[i] > 1099511627776.0)
            ICNV_FAIL(ICNV_ERR_ARG, "hspike_simulate: mean " + std::to_string(i % n_genes) + " of matrix " + std::to_string(i / n_genes) + " is above 2^40");
    }
    hipStream_t s = (hipStream_t)stream;
    DevBuf d_means, d_tok, d_vk, d_vc, d_pk, d_pc;
    if ((rc = upload(d_means, means, n_means, s)) || (rc = upload(d_tok, tokens, (size_t)n_mat, s)) || (rc = upload(d_vk, var_knots, (size_t)var_nk + 4, s)) ||
        (rc = upload(d_vc, var_coef, (size_t)var_nk, s)) || (rc = upload(d_pk, p0_knots, (size_t)p0_nk + 4, s)) || (rc = upload(d_pc, p0_coef, (size_t)p0_nk, s)))
        return rc;
    HsSim a{};
    a.means = d_means.as<double>(); a.tokens = d_tok.as<uint64_t>(); a.n_genes = (int32_t)n_genes; a.num_cells = num_cells; a.n_mat = n_mat;
    a.var = HsSpline{d_vk.as<double>(), d_vc.as<double>(), var_nk, var_xmin, var_range};
    a.p0 = HsSpline{d_pk.as<double>(), d_pc.as<double>(), p0_nk, p0_xmin, p0_range};
    a.seed = seed; a.out = out;
    if ((rc = launch_hs_simulate(a, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

int icnv_hspike_simulate(const double *means, int64_t n_genes, int32_t num_cells, int32_t n_mat, const double *var_knots,
                         const double *var_coef, int32_t var_nk, double var_xmin, double var_range, const double *p0_knots,
                         const double *p0_coef, int32_t p0_nk, double p0_xmin, double p0_range, uint64_t seed, const uint64_t *tokens,
                         double *out) {
    if (!out) ICNV_FAIL(ICNV_ERR_ARG, "hspike_simulate: null argument");
    if (n_genes < 1 || num_cells < 1 || n_mat < 1) ICNV_FAIL(ICNV_ERR_ARG, "hspike_simulate: n_genes, num_cells and n_mat must be >= 1");
    const size_t n = (size_t)n_mat * (size_t)num_cells * (size_t)n_genes;
    DevBuf d_out;
    int rc;
    if ((rc = d_out.alloc(n * sizeof(double)))) return rc;
    if ((rc = icnv_hspike_simulate_dev(means, n_genes, num_cells, n_mat, var_knots, var_coef, var_nk, var_xmin, var_range, p0_knots, p0_coef,
                                       p0_nk, p0_xmin, p0_range, seed, tokens, d_out.as<double>(), nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(out, d_out.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

}  // extern "C"
