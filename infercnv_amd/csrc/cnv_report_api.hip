// C ABI of K24 (include/icnv.h "CNV region reports"): validation, the plan of one report file (string tables, per-gene prefix
// sum and record offsets, computed once), the planning of a chunk of whole records.  Kernels: cnv_report_kernels.hip.
// DESIGN.md section 4 K24.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cnv_report_internal.h"
#include "icnv_internal.h"

using namespace icnv;

struct icnv_cnv_report {
    CrArgs a{};
    DevBuf d_rec, d_grp_b, d_grp_off, d_chr_b, d_chr_off, d_gene_b, d_gene_off, d_gstart, d_gend, d_P, d_rec_off, d_line_base, d_rmin, d_rmax;
    std::vector<int64_t> rec_off, line_base;   // host copies: [n_rec + 1]
    int64_t largest = 0;                       // bytes of the largest record
};

namespace {

std::atomic<int64_t> g_cr[5];   // calls, records, lines, bytes, wall microseconds

int check_table(const char *what, const uint8_t *bytes, const int64_t *off, int64_t n) {
    const std::string w = std::string("cnv_report: the ") + what;
    if (n < 1 || n > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, w + " table must have 1 .. 2^31 - 1 entries");
    if (!off) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report: null argument");
    if (off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, w + " offsets must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) ICNV_FAIL(ICNV_ERR_ARG, w + " offsets must not descend");
    if (off[n] > 0 && !bytes) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report: null argument");
    return ICNV_OK;
}

// rec: HOST copy of the six arrays, `stride` entries apart
int check_records(const int32_t *rec, int64_t stride, int64_t n, int64_t n_groups, int64_t n_chr, int64_t G) {
    const int32_t *col = rec, *chr = rec + stride, *first = rec + 2 * stride, *last = rec + 3 * stride, *state = rec + 4 * stride;
    for (int64_t r = 0; r < n; ++r) {
        const std::string w = "cnv_report: record " + std::to_string(r);
        if (col[r] < 0 || col[r] >= n_groups) ICNV_FAIL(ICNV_ERR_ARG, w + ": the list position is outside the cell-group table");
        if (chr[r] < 0 || chr[r] >= n_chr) ICNV_FAIL(ICNV_ERR_ARG, w + ": the chromosome is outside the chromosome table");
        if (first[r] > last[r]) ICNV_FAIL(ICNV_ERR_ARG, w + ": gene_first > gene_last");
        if (first[r] < 0 || last[r] >= G) ICNV_FAIL(ICNV_ERR_ARG, w + ": the gene range leaves the gene table");
        if (state[r] < 0 || state[r] > 255) ICNV_FAIL(ICNV_ERR_ARG, w + ": the state is not a byte");
    }
    return ICNV_OK;
}

// records_dev / records_host: the same arrays on both sides (one of them may be null: it is copied from the other)
int cr_begin(icnv_cnv_report **plan, int32_t kind, const int32_t *records_dev, const int32_t *records_host, int64_t stride, int64_t n_rec,
             const uint8_t *grp_b, const int64_t *grp_off, int64_t n_groups, const uint8_t *chr_b, const int64_t *chr_off, int64_t n_chr,
             const uint8_t *gene_b, const int64_t *gene_off, const int64_t *gstart, const int64_t *gend, int64_t G, int64_t *totals,
             hipStream_t s) {
    int rc;
    if (!plan) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report: null argument");
    *plan = nullptr;
    if (kind != CR_GENES && kind != CR_REGIONS) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report: unknown kind of report");
    if (n_rec < 0 || stride < n_rec) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report: the record capacity is below the record count");
    if (n_rec > 0 && !records_dev && !records_host) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report: null argument");
    if (!gstart || !gend) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report: null argument");
    if ((rc = check_table("cell-group", grp_b, grp_off, n_groups)) || (rc = check_table("chromosome", chr_b, chr_off, n_chr)) ||
        (rc = check_table("gene", gene_b, gene_off, G)))
        return rc;
    std::vector<int32_t> copy;
    if (n_rec > 0 && !records_host) {                          // the device records are checked here, before any launch
        copy.resize((size_t)n_rec * 6);
        for (int f = 0; f < 6; ++f)
            ICNV_HIP(hipMemcpyAsync(copy.data() + (size_t)f * n_rec, records_dev + (size_t)f * stride, (size_t)n_rec * sizeof(int32_t),
                                    hipMemcpyDeviceToHost, s));
        ICNV_HIP(hipStreamSynchronize(s));
        if ((rc = check_records(copy.data(), n_rec, n_rec, n_groups, n_chr, G))) return rc;
    } else if (n_rec > 0 && (rc = check_records(records_host, stride, n_rec, n_groups, n_chr, G))) {
        return rc;
    }

    std::unique_ptr<icnv_cnv_report> p(new icnv_cnv_report);
    CrArgs &a = p->a;
    if (!records_dev && n_rec > 0) {
        if ((rc = p->d_rec.alloc((size_t)n_rec * 6 * sizeof(int32_t)))) return rc;
        for (int f = 0; f < 6; ++f)
            ICNV_HIP(hipMemcpyAsync(p->d_rec.as<int32_t>() + (size_t)f * n_rec, records_host + (size_t)f * stride,
                                    (size_t)n_rec * sizeof(int32_t), hipMemcpyHostToDevice, s));
        records_dev = p->d_rec.as<int32_t>();
        stride = n_rec;
    }
    if ((rc = upload(p->d_grp_b, grp_b, (size_t)grp_off[n_groups], s)) || (rc = upload(p->d_grp_off, grp_off, (size_t)n_groups + 1, s)) ||
        (rc = upload(p->d_chr_b, chr_b, (size_t)chr_off[n_chr], s)) || (rc = upload(p->d_chr_off, chr_off, (size_t)n_chr + 1, s)) ||
        (rc = upload(p->d_gene_b, gene_b, (size_t)gene_off[G], s)) || (rc = upload(p->d_gene_off, gene_off, (size_t)G + 1, s)) ||
        (rc = upload(p->d_gstart, gstart, (size_t)G, s)) || (rc = upload(p->d_gend, gend, (size_t)G, s)) ||
        (rc = p->d_P.alloc((size_t)(G + 1) * sizeof(int64_t))) || (rc = p->d_rec_off.alloc((size_t)(n_rec + 1) * sizeof(int64_t))) ||
        (rc = p->d_line_base.alloc((size_t)(n_rec + 1) * sizeof(int64_t))) || (rc = p->d_rmin.alloc((size_t)std::max<int64_t>(n_rec, 1) * sizeof(int64_t))) ||
        (rc = p->d_rmax.alloc((size_t)std::max<int64_t>(n_rec, 1) * sizeof(int64_t))))
        return rc;
    a.kind = kind;
    a.col = records_dev; a.chr = records_dev + stride; a.first = records_dev + 2 * stride; a.last = records_dev + 3 * stride;
    a.state = records_dev + 4 * stride; a.ordinal = records_dev + 5 * stride;
    a.n_rec = n_rec;
    a.grp_b = p->d_grp_b.as<uint8_t>(); a.grp_off = p->d_grp_off.as<int64_t>();
    a.chr_b = p->d_chr_b.as<uint8_t>(); a.chr_off = p->d_chr_off.as<int64_t>();
    a.gene_b = p->d_gene_b.as<uint8_t>(); a.gene_off = p->d_gene_off.as<int64_t>();
    a.gstart = p->d_gstart.as<int64_t>(); a.gend = p->d_gend.as<int64_t>(); a.G = G;
    a.P = p->d_P.as<int64_t>(); a.rec_off = p->d_rec_off.as<int64_t>(); a.line_base = p->d_line_base.as<int64_t>();
    a.rmin = p->d_rmin.as<int64_t>(); a.rmax = p->d_rmax.as<int64_t>();

    p->rec_off.assign((size_t)n_rec + 1, 0);
    p->line_base.assign((size_t)n_rec + 1, 0);
    if (n_rec > 0) {
        if (kind == CR_GENES && (rc = launch_cr_gene_prefix(a, s))) return rc;
        if ((rc = launch_cr_lengths(a, s))) return rc;
        ICNV_HIP(hipMemcpyAsync(p->rec_off.data(), a.rec_off, (size_t)(n_rec + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (kind == CR_GENES)
            ICNV_HIP(hipMemcpyAsync(p->line_base.data(), a.line_base, (size_t)(n_rec + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    }
    ICNV_HIP(hipStreamSynchronize(s));                         // the uploads read the caller's arrays: they are done when this returns
    if (kind == CR_REGIONS)
        for (int64_t r = 0; r <= n_rec; ++r) p->line_base[(size_t)r] = r;
    for (int64_t r = 0; r < n_rec; ++r) p->largest = std::max(p->largest, p->rec_off[(size_t)r + 1] - p->rec_off[(size_t)r]);
    if (totals) {
        totals[0] = p->rec_off[(size_t)n_rec];
        totals[1] = p->line_base[(size_t)n_rec];
        totals[2] = p->largest;
    }
    *plan = p.release();
    return ICNV_OK;
}

int check_format(const icnv_cnv_report *p, int64_t rec0, const void *out, int64_t capacity, const int64_t *recs_done, const int64_t *n_bytes,
                 int64_t &rec1) {
    if (!p || !out || !recs_done || !n_bytes) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report_format: null argument");
    if (rec0 < 0 || rec0 >= p->a.n_rec) ICNV_FAIL(ICNV_ERR_ARG, "cnv_report_format: the record range is empty or leaves the records");
    if (capacity > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "cnv_report_format: a capacity above 2^31 - 1");
    const int64_t base = p->rec_off[(size_t)rec0];
    // the last record boundary within the capacity
    rec1 = (std::upper_bound(p->rec_off.begin() + rec0, p->rec_off.end(), base + capacity) - p->rec_off.begin()) - 1;
    if (capacity < 1 || rec1 <= rec0)
        ICNV_FAIL(ICNV_ERR_ARG, "cnv_report_format: the capacity is below the first record (" + std::to_string(p->rec_off[(size_t)rec0 + 1] - base) +
                                    " bytes)");
    return ICNV_OK;
}

void finish_format(const icnv_cnv_report *p, int64_t rec0, int64_t rec1, int64_t *rec_offsets, int64_t *recs_done, int64_t *n_bytes) {
    const int64_t base = p->rec_off[(size_t)rec0];
    if (rec_offsets)
        for (int64_t r = rec0; r <= rec1; ++r) rec_offsets[r - rec0] = p->rec_off[(size_t)r] - base;
    *recs_done = rec1 - rec0;
    *n_bytes = p->rec_off[(size_t)rec1] - base;
}

}  // namespace

extern "C" {

int icnv_cnv_report_begin_dev(icnv_cnv_report_t **plan, int32_t kind, const int32_t *records, int64_t capacity, int64_t n_records,
                              const uint8_t *group_bytes, const int64_t *group_off, int64_t n_groups, const uint8_t *chr_bytes,
                              const int64_t *chr_off, int64_t n_chr, const uint8_t *gene_bytes, const int64_t *gene_off,
                              const int64_t *gene_start, const int64_t *gene_end, int64_t G, int64_t *totals, void *stream) {
    return cr_begin(plan, kind, records, nullptr, capacity, n_records, group_bytes, group_off, n_groups, chr_bytes, chr_off, n_chr, gene_bytes,
                    gene_off, gene_start, gene_end, G, totals, (hipStream_t)stream);
}

int icnv_cnv_report_begin(icnv_cnv_report_t **plan, int32_t kind, const int32_t *records, int64_t capacity, int64_t n_records,
                          const uint8_t *group_bytes, const int64_t *group_off, int64_t n_groups, const uint8_t *chr_bytes,
                          const int64_t *chr_off, int64_t n_chr, const uint8_t *gene_bytes, const int64_t *gene_off,
                          const int64_t *gene_start, const int64_t *gene_end, int64_t G, int64_t *totals) {
    return cr_begin(plan, kind, nullptr, records, capacity, n_records, group_bytes, group_off, n_groups, chr_bytes, chr_off, n_chr, gene_bytes,
                    gene_off, gene_start, gene_end, G, totals, nullptr);
}

int icnv_cnv_report_format_dev(icnv_cnv_report_t *plan, int64_t rec0, uint8_t *out, int64_t capacity, int64_t *rec_offsets,
                               int64_t *recs_done, int64_t *n_bytes, void *stream) {
    int64_t rec1 = 0;
    int rc;
    if ((rc = check_format(plan, rec0, out, capacity, recs_done, n_bytes, rec1))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = (hipStream_t)stream;
    const int64_t base = plan->rec_off[(size_t)rec0], bytes = plan->rec_off[(size_t)rec1] - base;
    if ((rc = launch_cr_emit(plan->a, rec0, rec1, base, bytes, out, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    finish_format(plan, rec0, rec1, rec_offsets, recs_done, n_bytes);
    g_cr[0] += 1; g_cr[1] += rec1 - rec0; g_cr[2] += plan->line_base[(size_t)rec1] - plan->line_base[(size_t)rec0]; g_cr[3] += bytes;
    g_cr[4] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}

int icnv_cnv_report_format(icnv_cnv_report_t *plan, int64_t rec0, uint8_t *out, int64_t capacity, int64_t *rec_offsets, int64_t *recs_done,
                           int64_t *n_bytes) {
    int64_t rec1 = 0, done = 0, bytes = 0;
    int rc;
    if ((rc = check_format(plan, rec0, out, capacity, recs_done, n_bytes, rec1))) return rc;
    const int64_t need = plan->rec_off[(size_t)rec1] - plan->rec_off[(size_t)rec0];
    DevBuf d_out;
    if ((rc = d_out.alloc((size_t)need))) return rc;
    if ((rc = icnv_cnv_report_format_dev(plan, rec0, d_out.as<uint8_t>(), need, rec_offsets, &done, &bytes, nullptr))) return rc;
    ICNV_HIP(hipMemcpy(out, d_out.p, (size_t)bytes, hipMemcpyDeviceToHost));
    *recs_done = done;
    *n_bytes = bytes;
    return ICNV_OK;
}

void icnv_cnv_report_end(icnv_cnv_report_t *plan) { delete plan; }

int icnv_cnv_report_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 5; ++i) out[i] = g_cr[i].load();
    return ICNV_OK;
}

void icnv_cnv_report_stats_reset(void) {
    for (auto &c : g_cr) c.store(0);
}

}  // extern "C"
