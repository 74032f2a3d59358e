// npore_api.cpp -- C ABI (include/npore_amd.h): the entry points; the only translation unit.  Compiled with hipcc for gfx950 only.
// There is no CPU execution path for the DP here: without a gfx950 device npore_ctx_create fails.  The device path of a batch of reads
// lives in align_engine.hpp, the batch slots and the file pipeline's stages in file_pipeline.hpp, the order of its batches in
// batch_order.hpp; what reads BAM / FASTA files and writes SAM text needs no device and lives in bam_reader.hpp / hostio.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/npore_amd.h"
#include "confusion.hpp"
#include "glue.hpp"
#include "hostio.hpp"
#include "bam_reader.hpp"
#include "kernels.hpp"
#include "prep_kernels.hpp"
#include "annot_wave.hpp"
#include "unpack_kernels.hpp"
#include "bam_emit_kernels.hpp"
#include "confusion_kernels.hpp"
#include "purity_kernels.hpp"
#include "inflate_kernels.hpp"
#include "align_engine.hpp"
#include "file_pipeline.hpp"

// No C++ exception may cross the C ABI: the entry points that allocate are function-try-blocks ending in one of these.
#define NPORE_CATCH_INT                                                                             \
    catch (const std::bad_alloc &) { return fail(NPORE_E_NOMEM, "out of host memory"); }           \
    catch (const std::exception &e) { return fail(NPORE_E_INVALID, std::string("internal: ") + e.what()); }
#define NPORE_CATCH_PTR                                                                             \
    catch (const std::bad_alloc &) { fail(NPORE_E_NOMEM, "out of host memory"); return nullptr; }  \
    catch (const std::exception &e) { fail(NPORE_E_INVALID, std::string("internal: ") + e.what()); return nullptr; }

namespace {
// The device inflation of ONE run on a handle (npore_ctx_set "device_inflate"): made in front of the run's BamRecordWalker,
// so that the walker -- and its inflater thread, the hook's only caller -- has gone when this does; leaves what
// npore_bam_inflate_info reports on the handle (all zeros after a host run).
struct InflateRun {
    npore_bam *b;
    std::unique_ptr<npore::DeviceInflater> dev;
    InflateRun(const npore_ctx *ctx, npore_bam *b_) : b(b_)
    {
        for (int64_t &v : b->inflate_info) v = 0;
        if (ctx->device_inflate) dev.reset(new npore::DeviceInflater(ctx->device));
    }
    ~InflateRun() { if (dev) dev->info(b->inflate_info); }
    npore::BgzfInflateFn hook() const { return dev ? dev->hook() : npore::BgzfInflateFn(); }
};
}  // namespace

extern "C" {

int npore_abi_version(void) { return NPORE_ABI_VERSION; }
#if defined(NPORE_EXPERIMENTS) && defined(NPORE_STATS)
extern "C" int npore_debug_stats(unsigned long long *out, int reset)
{
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(npore::g_npore_stats), sizeof z) != hipSuccess) return -1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(npore::g_npore_stats), z, sizeof z) != hipSuccess) return -1;
    return 0;
}
#endif
const char *npore_last_error(void) { return g_err.c_str(); }

int npore_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, i) == hipSuccess && std::strncmp(pr.gcnArchName, "gfx950", 6) == 0) ok++;
    }
    return ok;
}

npore_ctx *npore_ctx_create(const float *sub_scores, const float *np_scores, int max_n, int max_l, int device_id)
try {
    const bool tables = sub_scores && np_scores;
    if ((!tables && (sub_scores || np_scores)) || max_n < 1 || max_n > MAX_PERIOD || max_l < 2 || max_l > 127) {   // repeat counts travel in 7-bit fields (layout.hpp, annotate planes)
        fail(NPORE_E_INVALID, "npore_ctx_create: need both tables (or neither: annotation-only context), 1 <= max_n <= 6, 2 <= max_l <= 127");
        return nullptr;
    }
    if (tables) {
        // a NaN breaks the MIN3 form of the MAT choice (cell.hpp Env::MIN3), and a -inf meets the +inf history
        // sentinels (inf - inf): either gives strings that silently differ from the reference's, so both are refused
        const size_t np_n = (size_t)max_n * (max_l + 1) * (max_l + 1);
        for (size_t i = 0; i < 25 + np_n; i++) {
            const float v = i < 25 ? sub_scores[i] : np_scores[i - 25];
            if (v != v || v == -std::numeric_limits<float>::infinity()) {
                fail(NPORE_E_INVALID, std::string("npore_ctx_create: ") + (i < 25 ? "sub_scores" : "np_scores") + "[" +
                                          std::to_string(i < 25 ? i : i - 25) + "] is " + (v != v ? "NaN" : "-inf") +
                                          ": penalty tables must hold no NaN and no -inf entries");
                return nullptr;
            }
        }
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0 || device_id < 0 || device_id >= n) {
        fail(NPORE_E_NODEVICE, "npore_ctx_create: no HIP device " + std::to_string(device_id) +
                                   " (this library has no CPU path)");
        return nullptr;
    }
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device_id) != hipSuccess || std::strncmp(pr.gcnArchName, "gfx950", 6) != 0) {
        fail(NPORE_E_NODEVICE, std::string("npore_ctx_create: device is not gfx950: ") + pr.gcnArchName);
        return nullptr;
    }
    auto *ctx = new npore_ctx();
    g_live_ctx[device_id & 15]++;
    ctx->device = device_id;
    ctx->n_cus = pr.multiProcessorCount;
    if (const char *e = std::getenv("NPORE_DEVICE_GLUE")) ctx->device_glue = std::atoi(e) != 0;      // (A/B of the BAM -> SAM pipeline: scripts/bench_realign.py)
    ctx->max_n = max_n;
    ctx->max_l = max_l;
    const size_t np_elems = (size_t)max_n * (max_l + 1) * (max_l + 1);
    bool ok = hipSetDevice(device_id) == hipSuccess && hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->s_fill[0], hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->s_fill[1], hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->s_post, hipStreamNonBlocking) == hipSuccess;
    if (tables)
        ok = ok && hipMalloc((void **)&ctx->d_sub, 25 * sizeof(float)) == hipSuccess &&
             hipMalloc((void **)&ctx->d_np, np_elems * sizeof(float)) == hipSuccess &&
             hipMemcpy(ctx->d_sub, sub_scores, 25 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(ctx->d_np, np_scores, np_elems * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    for (hipEvent_t *e : {&ctx->ev_user, &ctx->ev_cms[0], &ctx->ev_cms[1]}) ok = ok && hipEventCreate(e) == hipSuccess;
    for (auto &w : ctx->ws) {
        for (auto &e : w.ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        for (auto &e : w.evc) ok = ok && hipEventCreate(&e) == hipSuccess;
    }
    if (!ok) {
        fail(NPORE_E_HIP, "npore_ctx_create: HIP initialisation failed");
        npore_ctx_destroy(ctx);
        return nullptr;
    }
    return ctx;
}
NPORE_CATCH_PTR

void npore_ctx_destroy(npore_ctx *ctx)
{
    if (!ctx) return;
    g_live_ctx[ctx->device & 15]--;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();       // nothing of this context may still be running: only then do its members die
    for (auto *sp : ctx->slots) delete sp;
    delete ctx;
}

int npore_align_batch(npore_ctx *ctx, int64_t n_reads, const uint8_t *refs, const int64_t *ref_off,
                      const uint8_t *seqs, const int64_t *seq_off, const char *cigars, const int64_t *cig_off,
                      float indel_start, float indel_extend, int max_b_rows, int r, char *out,
                      const int64_t *out_off, int64_t *out_len, int32_t *status)
try {
    AlignArgs a = host_batch_args(n_reads, ref_off, seq_off, cig_off, indel_start, indel_extend, max_b_rows, r, out, out_off, out_len, status);
    a.h_refs = refs; a.h_seqs = seqs; a.h_cigs = cigars;
    return align_batch(ctx, a, true);
}
NPORE_CATCH_INT

int npore_align_batch_async(npore_ctx *ctx, int64_t n_reads, const uint8_t *refs, const int64_t *ref_off,
                            const uint8_t *seqs, const int64_t *seq_off, const char *cigars, const int64_t *cig_off,
                            float indel_start, float indel_extend, int max_b_rows, int r, char *out,
                            const int64_t *out_off, int64_t *out_len, int32_t *status)
try {
    AlignArgs a = host_batch_args(n_reads, ref_off, seq_off, cig_off, indel_start, indel_extend, max_b_rows, r, out, out_off, out_len, status);
    a.h_refs = refs; a.h_seqs = seqs; a.h_cigs = cigars;
    return align_batch(ctx, a, false);
}
NPORE_CATCH_INT

int npore_align_batch_cigars(npore_ctx *ctx, int64_t n_reads, const uint8_t *refs, const int64_t *ref_off,
                             const uint8_t *seqs, const int64_t *seq_off, const char *cigars, const int64_t *cig_off,
                             float indel_start, float indel_extend, int max_b_rows, int r, char *out,
                             const int64_t *out_off, int64_t *out_len, int32_t *status)
try {
    AlignArgs a = host_batch_args(n_reads, ref_off, seq_off, cig_off, indel_start, indel_extend, max_b_rows, r, out, out_off, out_len, status);
    a.h_refs = refs; a.h_seqs = seqs; a.h_cigs = cigars;
    a.final_text = true;                 // (no a.compact: the text of every read into the caller's slot)
    return align_batch(ctx, a, true);
}
NPORE_CATCH_INT

int npore_align_batch_device(npore_ctx *ctx, int64_t n_reads, const uint8_t *d_refs, const int64_t *d_ref_off,
                             const uint8_t *d_seqs, const int64_t *d_seq_off, const char *d_cigars,
                             const int64_t *d_cig_off, float indel_start, float indel_extend, int max_b_rows,
                             int r, char *d_out, const int64_t *d_out_off, int64_t *d_out_len,
                             int32_t *d_status, void *stream, int sync)
try {
    if (!ctx) return fail(NPORE_E_INVALID, "null context");
    if (n_reads < 0) return fail(NPORE_E_INVALID, "n_reads < 0");
    if (n_reads == 0) return NPORE_OK;
    if (!d_ref_off || !d_seq_off || !d_cig_off || !d_out_off || !d_out_len || !d_status)
        return fail(NPORE_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->deferred_rc) return quiesce(ctx);   // a group of an earlier asynchronous call failed
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // the host only needs the three offset arrays (24 bytes per read) to size work buffers
    const int64_t n = n_reads;
    // (into page-locked memory: three truly asynchronous copies and one wait instead of three staged ones)
    if (int rc = ctx->h_offs.ensure(3 * (size_t)(n + 1) * 8)) return rc;
    int64_t *offs = ctx->h_offs.as<int64_t>();
    HIP_TRY(hipMemcpyAsync(offs, d_ref_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(offs + (n + 1), d_seq_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(offs + 2 * (n + 1), d_cig_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    AlignArgs a;
    a.n_reads = n;
    a.d_refs = d_refs; a.d_ref_off = d_ref_off;
    a.d_seqs = d_seqs; a.d_seq_off = d_seq_off;
    a.d_cigs = d_cigars; a.d_cig_off = d_cig_off;
    a.h_ref_off = offs; a.h_seq_off = offs + (n + 1); a.h_cig_off = offs + 2 * (n + 1);
    a.indel_start = indel_start; a.indel_extend = indel_extend; a.max_b_rows = max_b_rows; a.r = r;
    OutTarget ot{reinterpret_cast<uint8_t *>(d_out), d_out_off, d_out_len, d_status};
    return run_core(ctx, a, ot, (hipStream_t)stream, sync != 0);
}
NPORE_CATCH_INT

int npore_ctx_wait(npore_ctx *ctx)
try {
    if (!ctx) return fail(NPORE_E_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    return quiesce(ctx);
}
NPORE_CATCH_INT

// get_np_info() of the sequences in ctx->in_seqs (host offsets `off`, n of them) by one wave per segment (annot_wave.hpp
// np_info_wave_kernel): raw (L, L_IDX) values into out32, or the byte planes of the region kernels into planes
static int launch_np_info(npore_ctx *ctx, hipStream_t s, const int64_t *off, int64_t n, int32_t *out32, uint8_t *planes)
{
    NpInfoParams q;
    q.max_n = ctx->max_n;
    q.max_l = ctx->max_l;
    q.seg = 16384;
    int warm = 0;
    for (int k = 1; k <= ctx->max_n; k++) warm += (ctx->max_l + 2) * k;
    q.warm = (warm + 63) & ~63;
    std::vector<int2> work;
    for (int64_t k = 0; k < n; k++)
        for (int64_t g = 0; g * q.seg < off[k + 1] - off[k]; g++) work.push_back(make_int2((int)k, (int)g));
    if (work.empty()) return NPORE_OK;
    if (int rc = ctx->in_off.ensure((size_t)(n + 1) * 8)) return rc;
    if (int rc = ctx->ws[0].rd_i32.ensure(work.size() * 8 + 16)) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->in_off.p, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctx->ws[0].rd_i32.p, work.data(), work.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                // (`work` is pageable host memory that dies with this call)
    q.seqs = ctx->in_seqs.as<uint8_t>();
    q.seq_off = ctx->in_off.as<int64_t>();
    q.work = ctx->ws[0].rd_i32.as<int2>();
    q.n_work = (int)work.size();
    q.out32 = out32;
    q.planes = planes;
    const dim3 grid((unsigned)work.size()), block(64);
    const bool alln = ctx->max_n == MAX_PERIOD;
    if (out32) {
        if (alln) hipLaunchKernelGGL((np_info_wave_kernel<ANNOT_RAW, true>), grid, block, 0, s, q);
        else hipLaunchKernelGGL((np_info_wave_kernel<ANNOT_RAW, false>), grid, block, 0, s, q);
    } else {
        if (alln) hipLaunchKernelGGL((np_info_wave_kernel<ANNOT_PLANES, true>), grid, block, 0, s, q);
        else hipLaunchKernelGGL((np_info_wave_kernel<ANNOT_PLANES, false>), grid, block, 0, s, q);
    }
    HIP_TRY(hipGetLastError());
    return NPORE_OK;
}

int npore_get_np_info(npore_ctx *ctx, const uint8_t *seq, int64_t len, int32_t *out)
try {
    if (!ctx || (len > 0 && (!seq || !out))) return fail(NPORE_E_INVALID, "null argument");
    if (len <= 0) return NPORE_OK;
    if (len > (1ll << 30)) return fail(NPORE_E_UNSUPPORTED, "sequence too long");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = quiesce(ctx)) return rc;
    const int mn = ctx->max_n;
    const size_t out_bytes = (size_t)len * 2 * mn * 4;
    // work buffers of the align path are reused (nothing else runs on this context meanwhile): grow-only, kept
    if (int rc = ctx->in_seqs.ensure((size_t)len + 16)) return rc;
    if (int rc = ctx->out.ensure(out_bytes)) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->in_seqs.p, seq, (size_t)len, hipMemcpyHostToDevice, s));
    const int64_t one_off[2] = {0, len};
    int32_t *L = ctx->out.as<int32_t>();
    if (int rc = launch_np_info(ctx, s, one_off, 1, L, nullptr)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, L, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return NPORE_OK;
}
NPORE_CATCH_INT

int npore_np_regions(npore_ctx *ctx, const uint8_t *seqs, const int64_t *seq_off, int64_t n_slices, int64_t *counts,
                     const int32_t **pos, const int32_t **reps, int64_t *total)
try {
    if (!ctx || n_slices < 0 || (n_slices > 0 && (!seqs || !seq_off || !counts)) || !pos || !reps || !total)
        return fail(NPORE_E_INVALID, "null argument");
    *pos = *reps = nullptr;
    *total = 0;
    if (n_slices == 0) return NPORE_OK;
    if (n_slices > (1 << 24)) return fail(NPORE_E_UNSUPPORTED, "too many slices in one call");
    const int64_t bases = seq_off[n_slices] - seq_off[0];
    for (int64_t k = 0; k < n_slices; k++) {
        const int64_t l = seq_off[k + 1] - seq_off[k];
        if (l < 0 || l >= (1ll << 30)) return fail(NPORE_E_INVALID, "slice length out of range");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = quiesce(ctx)) return rc;
    const int mn = ctx->max_n;
    const size_t m = (size_t)mn * n_slices;
    // work buffers of the align path are reused (nothing else runs on this context meanwhile)
    if (int rc = ctx->in_seqs.ensure((size_t)bases + 16)) return rc;
    if (int rc = ctx->in_off.ensure((size_t)(n_slices + 1) * 8)) return rc;
    if (int rc = ctx->ws[0].seql.ensure((size_t)bases * mn + 64)) return rc;
    if (int rc = ctx->ws[0].rd_i64.ensure((m + 2) * 8)) return rc;
    std::vector<int64_t> off((size_t)n_slices + 1);
    for (int64_t k = 0; k <= n_slices; k++) off[k] = seq_off[k] - seq_off[0];
    hipStream_t s = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->in_seqs.p, seqs + seq_off[0], (size_t)bases, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctx->in_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
    RegionParams rp;
    rp.seqs = ctx->in_seqs.as<uint8_t>();
    rp.seq_off = ctx->in_off.as<int64_t>();
    rp.n_slices = (int)n_slices;
    rp.max_n = mn;
    rp.max_l = ctx->max_l;
    rp.planes = ctx->ws[0].seql.as<uint8_t>();
    rp.counts = ctx->ws[0].rd_i64.as<int64_t>();
    rp.out_pos = rp.out_reps = nullptr;
    if (int rc = launch_np_info(ctx, s, off.data(), n_slices, nullptr, ctx->ws[0].seql.as<uint8_t>())) return rc;
    hipLaunchKernelGGL(region_count_kernel, dim3((unsigned)n_slices), dim3(1024), 0, s, rp);
    hipLaunchKernelGGL(region_scan_kernel, dim3(1), dim3(1024), 0, s, rp);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> offs(m + 1);
    HIP_TRY(hipMemcpyAsync(offs.data(), rp.counts, (m + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t tot = offs[m];
    for (size_t k = 0; k < m; k++) counts[k] = offs[k + 1] - offs[k];
    ctx->regions.resize((size_t)tot * 2);
    if (tot > 0) {
        if (int rc = ctx->out.ensure((size_t)tot * 8)) return rc;
        rp.out_pos = ctx->out.as<int32_t>();
        rp.out_reps = rp.out_pos + tot;
        hipLaunchKernelGGL(region_emit_kernel, dim3((unsigned)n_slices, (unsigned)mn), dim3(256), 0, s, rp);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ctx->regions.data(), rp.out_pos, (size_t)tot * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *pos = ctx->regions.data();
    *reps = ctx->regions.data() + tot;
    *total = tot;
    return NPORE_OK;
}
NPORE_CATCH_INT

int npore_last_timing(npore_ctx *ctx, double *ms, int n)
{
    if (!ctx || !ms) return fail(NPORE_E_INVALID, "null argument");
    for (int i = 0; i < n && i < 8; i++) ms[i] = ctx->timing[i];
    return NPORE_OK;
}

int npore_total_timing(npore_ctx *ctx, double *ms, int n)
{
    if (!ctx || !ms) return fail(NPORE_E_INVALID, "null argument");
    for (int i = 0; i < n && i < 8; i++) ms[i] = ctx->totals[i];
    return NPORE_OK;
}

int64_t npore_round_chunks(npore_ctx *ctx, int r)
{
    FillGeom g;
    if (!ctx || !fill_geometry(r, g)) return 0;
    return (int64_t)fill_round_workgroups(g, g.cmax, ctx->n_cus) * g.cmax;
}

int npore_fill_shape(npore_ctx *ctx, int r, int32_t *out, int n)
{
    FillGeom g;
    if (!ctx || !out) return fail(NPORE_E_INVALID, "null argument");
    if (!fill_geometry(r, g)) return fail(NPORE_E_UNSUPPORTED, "band half-width r > 511");
    const size_t lds = fill_lds_floats(g.nw, g.cmax, g.hw, g.rwin) * sizeof(float);
    const int wg_per_cu = std::max(1, std::min((int)((160 * 1024) / std::max<size_t>(lds, 1)), 2048 / (64 * g.nw * g.cmax)));
    const int32_t v[5] = {g.nw, g.cmax, wg_per_cu, fill_round_workgroups(g, g.cmax, ctx->n_cus), (int32_t)lds};
    for (int i = 0; i < n && i < 5; i++) out[i] = v[i];
    return NPORE_OK;
}

int npore_ctx_set(npore_ctx *ctx, const char *key, int64_t value)
try {
    if (!ctx || !key) return fail(NPORE_E_INVALID, "null argument");
    const std::string k(key);
    if (k == "tb_budget_mb") ctx->tb_budget_mb = value;
    else if (k == "force_chunks") ctx->force_chunks = (int)value;
    else if (k == "coresident") ctx->coresident = value != 0;
    else if (k == "device_glue") ctx->device_glue = value != 0;
    else if (k == "device_pack") ctx->device_pack = value != 0;
    else if (k == "device_inflate") ctx->device_inflate = value != 0;
    else if (k == "cms_batch_reads") { if (value < 1) return fail(NPORE_E_INVALID, "cms_batch_reads: at least 1"); ctx->cms_batch_reads = value; }
    else if (k == "purity_window") { if (value < 64 || value > (1ll << 24)) return fail(NPORE_E_INVALID, "purity_window: 64 .. 2^24"); ctx->purity_window = value; }
    else if (k == "fill_streams") { if (value < 1 || value > 2) return fail(NPORE_E_INVALID, "fill_streams: 1 or 2"); ctx->fill_streams = (int)value; }
    else return fail(NPORE_E_INVALID, "unknown key " + k);
    return NPORE_OK;
}
NPORE_CATCH_INT

static int standardize_batch_impl(bool expanded, int64_t n_reads, const char *alns, const int64_t *aln_off, const uint8_t *refs,
                            const int64_t *ref_off, const uint8_t *seqs, const int64_t *seq_off, char *out,
                            const int64_t *out_off, int64_t *out_len, int threads)
try {
    if (n_reads < 0 || (n_reads > 0 && (!alns || !aln_off || !ref_off || !seq_off || !out || !out_off || !out_len)))
        return fail(NPORE_E_INVALID, "null argument");
    const int nt = threads > 0 ? threads : (int)std::max(1u, std::thread::hardware_concurrency());
    std::atomic<int64_t> next{0};
    std::atomic<int> bad{0};
    auto work = [&] {
        for (;;) {
            const int64_t i = next.fetch_add(1);
            if (i >= n_reads) break;
            if (expanded) {       // never longer than the align() string
                if (aln_off[i + 1] - aln_off[i] > out_off[i + 1] - out_off[i]) { out_len[i] = -1; bad++; continue; }
                out_len[i] = standardize_expanded(alns + aln_off[i], aln_off[i + 1] - aln_off[i], refs + ref_off[i],
                                                  ref_off[i + 1] - ref_off[i], seqs + seq_off[i],
                                                  seq_off[i + 1] - seq_off[i], out + out_off[i]);
                continue;
            }
            const std::string c = standardize_collapsed(alns + aln_off[i], aln_off[i + 1] - aln_off[i],
                                                        refs + ref_off[i], ref_off[i + 1] - ref_off[i],
                                                        seqs + seq_off[i], seq_off[i + 1] - seq_off[i]);
            if ((int64_t)c.size() > out_off[i + 1] - out_off[i]) { out_len[i] = -1; bad++; continue; }
            std::memcpy(out + out_off[i], c.data(), c.size());
            out_len[i] = (int64_t)c.size();
        }
    };
    if (nt <= 1 || n_reads <= 1) work();
    else {
        std::vector<std::thread> pool;
        for (int t = 0; t < std::min<int64_t>(nt, n_reads); t++) pool.emplace_back(work);
        for (auto &t : pool) t.join();
    }
    return bad ? fail(NPORE_E_INVALID, "output slot too small") : NPORE_OK;
}
NPORE_CATCH_INT

int npore_standardize_batch(int64_t n_reads, const char *alns, const int64_t *aln_off, const uint8_t *refs,
                            const int64_t *ref_off, const uint8_t *seqs, const int64_t *seq_off, char *out,
                            const int64_t *out_off, int64_t *out_len, int threads)
{
    return standardize_batch_impl(false, n_reads, alns, aln_off, refs, ref_off, seqs, seq_off, out, out_off, out_len, threads);
}

int npore_standardize_ops_batch(int64_t n_reads, const char *alns, const int64_t *aln_off, const uint8_t *refs,
                                const int64_t *ref_off, const uint8_t *seqs, const int64_t *seq_off, char *out,
                                const int64_t *out_off, int64_t *out_len, int threads)
{
    return standardize_batch_impl(true, n_reads, alns, aln_off, refs, ref_off, seqs, seq_off, out, out_off, out_len, threads);
}

// ---- confusion matrices from pileup text (confusion.hpp) -------------------------------------------
int npore_confusion_counts(const char *lines, const int64_t *line_off, int64_t n_lines, const uint8_t *ref_codes,
                           int64_t n_ref, const char *ref_text, int64_t ref_text_len, const int32_t *np_info,
                           int64_t np_len, int max_n, int max_l, int64_t *subs, int64_t *nps, int64_t *inss,
                           int64_t *dels, int64_t *bad_lines, int threads)
try {
    if (n_lines < 0 || max_n < 1 || max_l < 1 || !subs || !nps || !inss || !dels ||
        (n_lines > 0 && (!lines || !line_off || !ref_codes || !ref_text || !np_info)))
        return fail(NPORE_E_INVALID, "bad argument");
    const size_t dim = (size_t)max_l + 1, n_nps = (size_t)max_n * dim * dim;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads > 0 ? threads : (int)std::thread::hardware_concurrency(),
                                                                 (n_lines + 4095) / 4096));
    // per-thread matrices (25 + max_n (max_l+1)^2 + 2 (max_l+1) counters), summed at the end
    std::vector<std::vector<int64_t>> acc((size_t)nt, std::vector<int64_t>(25 + n_nps + 2 * dim, 0));
    std::vector<int64_t> bad((size_t)nt, 0);
    std::atomic<int64_t> next{0};
    auto work = [&](int t) {
        int64_t *a = acc[(size_t)t].data();
        const ConfusionOut o{a, a + 25, a + 25 + n_nps, a + 25 + n_nps + dim};
        for (;;) {
            const int64_t b0 = next.fetch_add(1024);
            if (b0 >= n_lines) break;
            for (int64_t k = b0; k < std::min(n_lines, b0 + 1024); k++)
                if (!confusion_count_line(lines + line_off[k], line_off[k + 1] - line_off[k], k, ref_codes, n_ref, ref_text,
                                          ref_text_len, np_info, np_len, max_n, max_l, o))
                    bad[(size_t)t]++;
        }
    };
    if (nt == 1) work(0);
    else {
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; t++) pool.emplace_back(work, t);
        for (auto &th : pool) th.join();
    }
    int64_t nbad = 0;
    for (int t = 0; t < nt; t++) {
        const int64_t *a = acc[(size_t)t].data();
        for (size_t k = 0; k < 25; k++) subs[k] += a[k];
        for (size_t k = 0; k < n_nps; k++) nps[k] += a[25 + k];
        for (size_t k = 0; k < dim; k++) { inss[k] += a[25 + n_nps + k]; dels[k] += a[25 + n_nps + dim + k]; }
        nbad += bad[(size_t)t];
    }
    if (bad_lines) *bad_lines = nbad;
    return NPORE_OK;
}
NPORE_CATCH_INT

// ---- confusion matrices from BAM records (confusion_rec.hpp, confusion_kernels.hpp) ------------------------------
namespace {
struct CmsContig {
    std::vector<CmsRange> ranges;        // layer after layer
    std::vector<int32_t> layer_off;
    int64_t bases = 0;                   // of all slices
    int64_t lo = 0, hi = 0;              // hull of the ranges: what the reader selects by
};

// the caller's ranges of one contig (clipped to it) in layers of ascending, disjoint ranges, their slices laid out back to back
void cms_layers(std::vector<CmsRange> rs, int max_n, CmsContig &c)
{
    std::sort(rs.begin(), rs.end(), [](const CmsRange &a, const CmsRange &b) { return a.st != b.st ? a.st < b.st : a.en < b.en; });
    std::vector<std::vector<CmsRange>> layers;
    int64_t off = 0;
    c.lo = rs.front().st;
    c.hi = 0;
    for (CmsRange r : rs) {
        r.ann = off * max_n;
        off += r.slen;
        c.hi = std::max(c.hi, r.en);
        size_t y = 0;
        while (y < layers.size() && layers[y].back().en > r.st) y++;
        if (y == layers.size()) layers.emplace_back();
        layers[y].push_back(r);
    }
    c.bases = off;
    c.layer_off.assign(1, 0);
    for (auto &l : layers) {
        c.ranges.insert(c.ranges.end(), l.begin(), l.end());
        c.layer_off.push_back((int32_t)c.ranges.size());
    }
}

struct CmsHostTally {
    int64_t t[CMS_N_TALLIES] = {};
};
}  // namespace

// the planes of a contig's range slices (ws[0].seql) and its range table (cms_ranges) on the device
static int cms_contig_planes(npore_ctx *ctx, const CmsContig &c, const char *d_contig, hipStream_t s)
{
    const int mn = ctx->max_n;
    const size_t n = c.ranges.size(), rbytes = n * sizeof(CmsRange), lbytes = c.layer_off.size() * 4;
    if (int rc = ctx->in_seqs.ensure((size_t)c.bases + 16)) return rc;
    if (int rc = ctx->ws[0].seql.ensure((size_t)c.bases * mn + 64)) return rc;
    if (int rc = ctx->cms_ranges.ensure(rbytes + lbytes + 16)) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->cms_ranges.p, c.ranges.data(), rbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctx->cms_ranges.as<char>() + rbytes, c.layer_off.data(), lbytes, hipMemcpyHostToDevice, s));
    SliceCodesParams sp{d_contig, ctx->cms_ranges.as<CmsRange>(), (int)n, mn, ctx->in_seqs.as<uint8_t>()};
    hipLaunchKernelGGL(slice_codes_kernel, dim3((unsigned)n), dim3(256), 0, s, sp);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> off(n + 1);
    for (size_t k = 0; k < n; k++) off[k] = c.ranges[k].ann / mn;
    off[n] = c.bases;
    std::sort(off.begin(), off.end());               // (the table is in layer order, the slices lie in the order of their starts)
    return launch_np_info(ctx, s, off.data(), (int64_t)n, nullptr, ctx->ws[0].seql.as<uint8_t>());
}

int npore_bam_confusion(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, int64_t n_ranges,
                        const int32_t *ref_id, const int64_t *start, const int64_t *stop, int min_bq, uint32_t exclude_flags,
                        int64_t *subs, int64_t *nps, int64_t *inss, int64_t *dels, int64_t *tallies)
try {
    if (!ctx || !b || !fa || !fasta_of_ref || n_ranges < 0 || (n_ranges > 0 && (!ref_id || !start || !stop)) || !subs || !nps || !inss ||
        !dels || !tallies)
        return fail(NPORE_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = quiesce(ctx)) return rc;
    const int mn = ctx->max_n, dim = ctx->max_l + 1;
    const size_t n_nps = (size_t)mn * dim * dim, n_counts = 25 + n_nps + 2 * (size_t)dim + CMS_N_TALLIES;
    const size_t n_refs = b->ref_names.size();
    // the ranges by contig
    std::vector<CmsContig> contigs(n_refs);
    {
        std::vector<std::vector<CmsRange>> by(n_refs);
        for (int64_t k = 0; k < n_ranges; k++) {
            if (ref_id[k] < 0 || ref_id[k] >= (int32_t)n_refs) continue;      // (a contig the BAM does not know has no records)
            const int fi = fasta_of_ref[ref_id[k]];
            if (fi < 0 || fi >= (int)fa->names.size()) return fail(NPORE_E_INVALID, "a range lies on a contig that is not in the FASTA");
            const int64_t clen = fa->len((size_t)fi);
            if (clen >= (1ll << 30)) return fail(NPORE_E_UNSUPPORTED, "contig too long");
            CmsRange r;
            if (cms_clip(start[k], stop[k], clen, r)) by[(size_t)ref_id[k]].push_back(r);
        }
        for (size_t r = 0; r < n_refs; r++)
            if (!by[r].empty()) cms_layers(std::move(by[r]), mn, contigs[r]);
    }
    std::vector<int32_t> h_rid;
    std::vector<int64_t> h_lo, h_hi;
    for (size_t r = 0; r < n_refs; r++)
        if (!contigs[r].ranges.empty()) { h_rid.push_back((int32_t)r); h_lo.push_back(contigs[r].lo); h_hi.push_back(contigs[r].hi); }
    if (int rc = device_fasta(ctx, b, fa, fasta_of_ref)) return rc;
    std::vector<CtgEntry> ctg(std::max<size_t>(1, n_refs), CtgEntry{nullptr, 0});
    for (size_t k = 0; k < n_refs; k++) {
        const int fi = fasta_of_ref[k];
        if (fi >= 0 && fi < (int)fa->names.size()) ctg[k] = CtgEntry{ctx->d_fasta.as<char>() + fa->off[(size_t)fi], fa->len((size_t)fi)};
    }
    hipStream_t s = ctx->stream;
    if (int rc = ctx->cms_counts.ensure(n_counts * 8)) return rc;
    HIP_TRY(hipMemsetAsync(ctx->cms_counts.p, 0, n_counts * 8, s));

    // the reader: one pass where the handle allows it (mode 3: no record index), else selection on the index; the flags
    // are this function's business (drop_flags = 0), unplaced records never arrive
    const bool one_pass = b->file && !b->blocks.empty() && b->rec_off.empty();
    const int threads = 0;
    const int64_t batch_reads = ctx->cms_batch_reads;
    InflateRun infl(ctx, b);
    std::unique_ptr<BamRecordWalker> walker;
    std::vector<int64_t> idx;
    int64_t idx_at = 0;
    if (one_pass) {
        if (int rc = one_pass_args_check(b, (int)h_rid.size(), h_rid.data(), 0)) return rc;
        walker.reset(new BamRecordWalker(b, (int)h_rid.size(), h_rid.data(), h_lo.data(), h_hi.data(), 0, threads, 0u, infl.hook()));
    } else {
        const int64_t k = bam_select(b, (int)h_rid.size(), h_rid.data(), h_lo.data(), h_hi.data(), 0, nullptr, 0, 0u);
        if (k < 0) return (int)k;
        idx.assign((size_t)k + 1, 0);
        if (bam_select(b, (int)h_rid.size(), h_rid.data(), h_lo.data(), h_hi.data(), 0, idx.data(), k, 0u) != k) return fail(NPORE_E_INVALID, "select is not repeatable");
        idx.resize((size_t)k);
    }
    RecFetch rf;
    std::vector<std::shared_ptr<RawBuf>> keep;
    PinnedBuf raw, rawo_pin;
    std::vector<int32_t> gate;
    std::vector<int64_t> rawo;
    std::vector<int32_t> kept_rid;
    CmsHostTally ht;
    double kernel_ms = 0.0;
    int32_t cur_rid = -1;
    for (;;) {
        keep.clear();
        int64_t m;
        if (one_pass) m = walker->next_batch(rf, keep, batch_reads);
        else {
            m = std::min<int64_t>(batch_reads, (int64_t)idx.size() - idx_at);
            if (m > 0) { if (int rc = fetch_records(b, idx.data() + idx_at, m, threads, rf)) return rc; }
            idx_at += std::max<int64_t>(m, 0);
        }
        if (m < 0) return (int)m;
        if (m == 0) break;
        // the gate (confusion_rec.hpp cms_gate), on all cores
        gate.assign((size_t)m, -1);
        const int64_t per = 64;
        parallel_for((m + per - 1) / per, threads, [&](int64_t tix) {
            for (int64_t k = tix * per; k < std::min(m, (tix + 1) * per); k++) {
                const RecView r = rec_of(rf, k);
                const int32_t rid = r.ref_id();
                if (rid < 0 || rid >= (int32_t)n_refs || contigs[(size_t)rid].ranges.empty()) continue;
                const CmsContig &c = contigs[(size_t)rid];
                const RecCigar cg = rec_cigar(r);
                gate[(size_t)k] = cms_gate((uint32_t)r.flag(), r.pos(), r.l_seq(), cg.w, (int)cg.n, exclude_flags, c.ranges.data(),
                                           c.layer_off.data(), (int)c.layer_off.size() - 1);
            }
        });
        rawo.assign(1, 0);
        kept_rid.clear();
        std::vector<int64_t> kept;
        for (int64_t k = 0; k < m; k++) {
            const int g = gate[(size_t)k];
            if (g > 0) ht.t[g]++;
            if (g != 0) continue;
            kept.push_back(k);
            kept_rid.push_back(rec_of(rf, k).ref_id());
            rawo.push_back(rawo.back() + ((staged_head_bytes(rf.ptr[(size_t)k], true) + 7) & ~7ll));
        }
        ht.t[CMS_T_BATCHES]++;
        const int64_t n = (int64_t)kept.size();
        if (n == 0) continue;
        if (int rc = raw.ensure((size_t)rawo[(size_t)n] + 64)) return rc;
        if (int rc = rawo_pin.ensure((size_t)(n + 1) * 8)) return rc;
        std::memcpy(rawo_pin.p, rawo.data(), (size_t)(n + 1) * 8);
        parallel_for((n + per - 1) / per, threads, [&](int64_t tix) {
            for (int64_t k = tix * per; k < std::min(n, (tix + 1) * per); k++)
                stage_record_head(rf.ptr[(size_t)kept[(size_t)k]], true, reinterpret_cast<uint8_t *>(raw.p) + rawo[(size_t)k]);
        });
        if (int rc = ctx->cms_raw.ensure((size_t)rawo[(size_t)n] + 64)) return rc;
        if (int rc = ctx->cms_off.ensure((size_t)(n + 1) * 8)) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->cms_raw.p, raw.p, (size_t)rawo[(size_t)n], hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ctx->cms_off.p, rawo_pin.p, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        for (int64_t k0 = 0; k0 < n;) {
            int64_t k1 = k0 + 1;
            while (k1 < n && kept_rid[(size_t)k1] == kept_rid[(size_t)k0]) k1++;
            const int32_t rid = kept_rid[(size_t)k0];
            const CmsContig &c = contigs[(size_t)rid];
            if (rid != cur_rid) {                    // one contig's planes at a time
                if (int rc = cms_contig_planes(ctx, c, ctg[(size_t)rid].bases, s)) return rc;
                cur_rid = rid;
            }
            CmsParams cp;
            cp.raw = ctx->cms_raw.as<uint8_t>();
            cp.raw_off = ctx->cms_off.as<int64_t>() + k0;
            cp.n_reads = k1 - k0;
            cp.contig = ctg[(size_t)rid].bases;
            cp.clen = ctg[(size_t)rid].len;
            cp.ranges = ctx->cms_ranges.as<CmsRange>();
            cp.layer_off = reinterpret_cast<const int32_t *>(ctx->cms_ranges.as<char>() + c.ranges.size() * sizeof(CmsRange));
            cp.n_layers = (int)c.layer_off.size() - 1;
            cp.planes = ctx->ws[0].seql.as<uint8_t>();
            cp.max_n = mn;
            cp.max_l = ctx->max_l;
            cp.min_bq = min_bq;
            cp.counts = ctx->cms_counts.as<unsigned long long>();
            HIP_TRY(hipEventRecord(ctx->ev_cms[0], s));
            hipLaunchKernelGGL(confusion_records_kernel, dim3((unsigned)(k1 - k0)), dim3(256), 0, s, cp);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ctx->ev_cms[1], s));
            HIP_TRY(hipStreamSynchronize(s));        // (the staging buffers and the planes are free again)
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_cms[0], ctx->ev_cms[1]));
            kernel_ms += ms;
            k0 = k1;
        }
    }
    std::vector<unsigned long long> h(n_counts);
    HIP_TRY(hipMemcpyAsync(h.data(), ctx->cms_counts.p, n_counts * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t k = 0; k < 25; k++) subs[k] += (int64_t)h[k];
    for (size_t k = 0; k < n_nps; k++) nps[k] += (int64_t)h[25 + k];
    for (int k = 0; k < dim; k++) { inss[k] += (int64_t)h[25 + n_nps + k]; dels[k] += (int64_t)h[25 + n_nps + dim + k]; }
    for (int k = 0; k < CMS_N_TALLIES; k++) tallies[k] += (int64_t)h[25 + n_nps + 2 * dim + k] + ht.t[k];
    tallies[CMS_T_KERNEL_NS] += (int64_t)(kernel_ms * 1e6);
    return NPORE_OK;
}
NPORE_CATCH_INT

// ---- Gini purity of pileups from BAM records (purity_rec.hpp, purity_kernels.hpp) --------------------------------------
namespace {
struct PurContig {
    std::vector<CmsRange> ranges;        // merged: ascending, disjoint, ann = dense index of the first position
    int64_t P = 0, base = 0;             // positions; where its rows begin among all contigs'
    int64_t lo = 0, hi = 0;              // hull
};

// the caller's ranges of one contig (clipped to it) merged into a disjoint ascending set
void pur_merge(std::vector<CmsRange> rs, PurContig &c)
{
    std::sort(rs.begin(), rs.end(), [](const CmsRange &a, const CmsRange &b) { return a.st != b.st ? a.st < b.st : a.en < b.en; });
    for (const CmsRange &r : rs) {
        if (!c.ranges.empty() && r.st <= c.ranges.back().en) c.ranges.back().en = std::max(c.ranges.back().en, r.en);
        else c.ranges.push_back(r);
    }
    int64_t off = 0;
    for (CmsRange &r : c.ranges) {
        r.ann = off;
        r.slen = r.en - r.st;
        off += r.slen;
    }
    c.P = off;
    c.lo = c.ranges.front().st;
    c.hi = c.ranges.back().en;
}
// the contig position of dense index d
int64_t pur_ref_of_dense(const PurContig &c, int64_t d)
{
    size_t l = 0, h = c.ranges.size();   // last range with ann <= d
    while (h - l > 1) {
        const size_t mid = (l + h) / 2;
        if (c.ranges[mid].ann <= d) l = mid; else h = mid;
    }
    return c.ranges[l].st + (d - c.ranges[l].ann);
}

// One run of npore_bam_purity: the device side of a window and the batch on its way to it.
struct PurRun {
    npore_ctx *ctx;
    hipStream_t s;
    int min_bq;
    int64_t W, stride;                   // window size; plane stride (W, or fewer where no contig has as many positions)
    int64_t batch_reads;
    int64_t *pos_stats;
    const PurContig *c = nullptr;        // the current contig, its window
    int64_t w = 0, win_lo = 0, win_hi = 0, ref_lo = 0, ref_hi = 0;
    bool dirty = false;
    int64_t ev_bound = 0;                // no more events than this lie behind the cursor
    struct Item { const uint8_t *q; bool staged; };      // a record of the reader, or a carried staged head
    std::vector<Item> batch;
    int64_t batch_ins = 0;
    PinnedBuf raw, rawo_pin;
    std::vector<int64_t> rawo;
    double kernel_ms = 0.0;
    int64_t windows = 0, batches = 0;

    uint32_t *cnt() const { return ctx->pur_cnt.as<uint32_t>(); }
    unsigned long long *hist() const { return ctx->pur_out.as<unsigned long long>(); }
    unsigned long long *d_tallies() const { return hist() + 2 * PUR_BINS; }
    uint32_t *cursor() const { return reinterpret_cast<uint32_t *>(d_tallies() + PUR_D_TALLIES); }
    static size_t out_bytes() { return (2 * PUR_BINS + PUR_D_TALLIES + 1) * 8; }

    int timed_begin() { HIP_TRY(hipEventRecord(ctx->ev_cms[0], s)); return NPORE_OK; }
    int timed_end()
    {
        HIP_TRY(hipEventRecord(ctx->ev_cms[1], s));
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_cms[0], ctx->ev_cms[1]));
        kernel_ms += ms;
        return NPORE_OK;
    }
    int set_contig(const PurContig &pc)
    {
        c = &pc;
        const size_t bytes = pc.ranges.size() * sizeof(CmsRange);
        if (int rc = ctx->cms_ranges.ensure(bytes + 16)) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->cms_ranges.p, pc.ranges.data(), bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        set_window(0);
        return NPORE_OK;
    }
    void set_window(int64_t win)
    {
        w = win;
        win_lo = win * W;
        win_hi = std::min(c->P, win_lo + W);
        ref_lo = pur_ref_of_dense(*c, win_lo);
        ref_hi = pur_ref_of_dense(*c, win_hi - 1) + 1;
    }
    int64_t n_windows() const { return (c->P + W - 1) / W; }
    // the bytes of a staged head with its qualities (staged_head.hpp)
    static int64_t staged_bytes(const uint8_t *h)
    {
        const uint8_t *cg, *sq;
        int nc;
        staged_cigar(h + 4, cg, nc, sq);
        const int64_t l_seq = rdi32(h + 4 + 16);
        return (int64_t)(sq - h) + (l_seq + 1) / 2 + l_seq;
    }
    int add(const uint8_t *q, int64_t ins_ops, bool staged = false)
    {
        batch.push_back(Item{q, staged});
        batch_ins += ins_ops;
        return (int64_t)batch.size() >= batch_reads ? flush() : NPORE_OK;
    }
    // the batch through purity_records_kernel, into the current window
    int flush()
    {
        const int64_t n = (int64_t)batch.size();
        if (n == 0) return NPORE_OK;
        rawo.assign(1, 0);
        for (const Item &it : batch)
            rawo.push_back(rawo.back() + (((it.staged ? staged_bytes(it.q) : staged_head_bytes(it.q, true)) + 7) & ~7ll));
        if (int rc = raw.ensure((size_t)rawo[(size_t)n] + 64)) return rc;
        if (int rc = rawo_pin.ensure((size_t)(n + 1) * 8)) return rc;
        std::memcpy(rawo_pin.p, rawo.data(), (size_t)(n + 1) * 8);
        const int64_t per = 64;
        parallel_for((n + per - 1) / per, 0, [&](int64_t tix) {
            for (int64_t k = tix * per; k < std::min(n, (tix + 1) * per); k++) {
                const Item &it = batch[(size_t)k];
                if (it.staged) std::memcpy(raw.p + rawo[(size_t)k], it.q, (size_t)staged_bytes(it.q));
                else stage_record_head(it.q, true, reinterpret_cast<uint8_t *>(raw.p) + rawo[(size_t)k]);
            }
        });
        if (int rc = ctx->cms_raw.ensure((size_t)rawo[(size_t)n] + 64)) return rc;
        if (int rc = ctx->cms_off.ensure((size_t)(n + 1) * 8)) return rc;
        // the events of the window so far stay where they are when their buffer grows
        const size_t ev_need = (size_t)(ev_bound + batch_ins + 1) * sizeof(PurEvent);
        if (ev_need > ctx->pur_ev.cap) {
            DevBuf nb;
            if (int rc = nb.ensure(ev_need + ev_need / 2)) return rc;
            if (ev_bound > 0) HIP_TRY(hipMemcpyAsync(nb.p, ctx->pur_ev.p, (size_t)ev_bound * sizeof(PurEvent), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
            std::swap(nb.p, ctx->pur_ev.p);
            std::swap(nb.cap, ctx->pur_ev.cap);
        }
        HIP_TRY(hipMemcpyAsync(ctx->cms_raw.p, raw.p, (size_t)rawo[(size_t)n], hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ctx->cms_off.p, rawo_pin.p, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        PurParams p;
        p.raw = ctx->cms_raw.as<uint8_t>();
        p.raw_off = ctx->cms_off.as<int64_t>();
        p.n_reads = n;
        p.ranges = ctx->cms_ranges.as<CmsRange>();
        p.n_ranges = (int)c->ranges.size();
        p.win_lo = win_lo;
        p.win_hi = win_hi;
        p.ref_lo = ref_lo;
        p.ref_hi = ref_hi;
        p.W = stride;
        p.min_bq = min_bq;
        p.cnt = cnt();
        p.events = ctx->pur_ev.as<PurEvent>();
        p.cursor = cursor();
        p.ev_cap = (uint32_t)std::min<int64_t>(ev_bound + batch_ins, UINT32_MAX);
        p.tallies = d_tallies();
        if (int rc = timed_begin()) return rc;
        hipLaunchKernelGGL(purity_records_kernel, dim3((unsigned)n), dim3(256), 0, s, p);
        HIP_TRY(hipGetLastError());
        if (int rc = timed_end()) return rc;     // (the staging buffers are free again)
        ev_bound += batch_ins;
        batch.clear();
        batch_ins = 0;
        batches++;
        dirty = true;
        return NPORE_OK;
    }
    // the window's end: buckets, pair counts, scores; the window is zero afterwards
    int finish_window()
    {
        if (int rc = flush()) return rc;
        if (!dirty) return NPORE_OK;
        const int64_t n = win_hi - win_lo;
        if (ev_bound >= (int64_t)UINT32_MAX) return fail(NPORE_E_UNSUPPORTED, "more than 2^32 insertions in one window: choose a smaller purity_window");
        const uint32_t cap = (uint32_t)ev_bound;
        const unsigned n_blocks = (unsigned)((n + PUR_SCAN_PER_BLOCK - 1) / PUR_SCAN_PER_BLOCK);
        if (cap > 0) {
            if (int rc = ctx->pur_bsum.ensure((size_t)n_blocks * 4 + 16)) return rc;
            if (int rc = ctx->pur_sorted.ensure((size_t)cap * sizeof(PurEvent))) return rc;
        }
        if (pos_stats)
            if (int rc = ctx->pur_rows.ensure((size_t)n * 32)) return rc;
        if (int rc = timed_begin()) return rc;
        if (cap > 0) {
            uint32_t *t_plane = cnt() + 5 * stride, *off = cnt() + 6 * stride;
            hipLaunchKernelGGL(purity_scan_blocks_kernel, dim3(n_blocks), dim3(256), 0, s, t_plane, off, ctx->pur_bsum.as<uint32_t>(), n);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(purity_scan_top_kernel, dim3(1), dim3(256), 0, s, ctx->pur_bsum.as<uint32_t>(), (int)n_blocks);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(purity_scan_add_kernel, dim3(n_blocks), dim3(256), 0, s, off, ctx->pur_bsum.as<uint32_t>(), n);
            HIP_TRY(hipGetLastError());
            const unsigned eb = (cap + 255u) / 256u;
            hipLaunchKernelGGL(purity_scatter_kernel, dim3(eb), dim3(256), 0, s, ctx->pur_ev.as<PurEvent>(), cursor(), cap, off, ctx->pur_sorted.as<PurEvent>());
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(purity_pairs_kernel, dim3(eb), dim3(256), 0, s, ctx->pur_sorted.as<PurEvent>(), cursor(), cap, t_plane, off,
                               ctx->pur_v2.as<unsigned long long>());
            HIP_TRY(hipGetLastError());
        }
        PurFinalParams fp{cnt(), ctx->pur_v2.as<unsigned long long>(), stride, n, hist(), d_tallies(), pos_stats ? ctx->pur_rows.as<int64_t>() : nullptr};
        hipLaunchKernelGGL(purity_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fp);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(cursor(), 0, 4, s));
        if (int rc = timed_end()) return rc;
        if (pos_stats) {
            HIP_TRY(hipMemcpyAsync(pos_stats + 4 * (c->base + win_lo), ctx->pur_rows.p, (size_t)n * 32, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        windows++;
        dirty = false;
        ev_bound = 0;
        return NPORE_OK;
    }
};
}  // namespace

int npore_bam_purity(npore_ctx *ctx, npore_bam *b, int64_t n_ranges, const int32_t *ref_id, const int64_t *start, const int64_t *stop,
                     int min_bq, uint32_t exclude_flags, int64_t *base_hist, int64_t *ins_hist, int64_t *pos_stats, int64_t pos_cap,
                     int64_t *tallies)
try {
    if (!ctx || !b || n_ranges < 0 || (n_ranges > 0 && (!ref_id || !start || !stop)) || !base_hist || !ins_hist || !tallies || (pos_stats && pos_cap < 0))
        return fail(NPORE_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = quiesce(ctx)) return rc;
    const size_t n_refs = b->ref_names.size();
    // the ranges by contig, merged; P = the positions of all of them, contigs in header order
    std::vector<PurContig> contigs(n_refs);
    int64_t P = 0, max_p = 0;
    {
        std::vector<std::vector<CmsRange>> by(n_refs);
        for (int64_t k = 0; k < n_ranges; k++) {
            if (ref_id[k] < 0 || ref_id[k] >= (int32_t)n_refs) continue;
            const int64_t clen = b->ref_lens[(size_t)ref_id[k]];
            if (clen >= (1ll << 31)) return fail(NPORE_E_UNSUPPORTED, "contig too long");
            CmsRange r;
            if (cms_clip(start[k], stop[k], clen, r)) by[(size_t)ref_id[k]].push_back(r);
        }
        for (size_t r = 0; r < n_refs; r++) {
            if (by[r].empty()) continue;
            pur_merge(std::move(by[r]), contigs[r]);
            contigs[r].base = P;
            P += contigs[r].P;
            max_p = std::max(max_p, contigs[r].P);
        }
    }
    if (pos_stats && P > pos_cap) return fail(NPORE_E_INVALID, "pos_stats holds fewer rows than the ranges have positions");
    std::vector<int32_t> h_rid;
    std::vector<int64_t> h_lo, h_hi;
    for (size_t r = 0; r < n_refs; r++)
        if (!contigs[r].ranges.empty()) { h_rid.push_back((int32_t)r); h_lo.push_back(contigs[r].lo); h_hi.push_back(contigs[r].hi); }

    PurRun run;
    run.ctx = ctx;
    run.s = ctx->stream;
    run.min_bq = min_bq;
    run.W = ctx->purity_window;
    run.stride = std::max<int64_t>(64, std::min(run.W, max_p));
    run.batch_reads = ctx->cms_batch_reads;
    run.pos_stats = pos_stats;
    hipStream_t s = run.s;
    if (int rc = ctx->pur_cnt.ensure((size_t)run.stride * PUR_PLANES * 4)) return rc;
    if (int rc = ctx->pur_v2.ensure((size_t)run.stride * 8)) return rc;
    if (int rc = ctx->pur_out.ensure(PurRun::out_bytes())) return rc;
    HIP_TRY(hipMemsetAsync(ctx->pur_cnt.p, 0, (size_t)run.stride * PUR_PLANES * 4, s));
    HIP_TRY(hipMemsetAsync(ctx->pur_v2.p, 0, (size_t)run.stride * 8, s));
    HIP_TRY(hipMemsetAsync(ctx->pur_out.p, 0, PurRun::out_bytes(), s));
    if (pos_stats && P > 0) std::memset(pos_stats, 0, (size_t)P * 32);
    int64_t ht[PUR_N_TALLIES] = {};

    // What the host needs of every record of a reader's batch, found on all cores: the gate (cms_gate: 0 = walked, -1 = none
    // of the ranges' records, else the tally it goes to), its I operations, the windows its positions lie in
    struct RecInfo {
        int gate;
        int32_t no_entry, ins_ops;
        int64_t w0, w1;
    };
    std::vector<RecInfo> info;
    RecFetch rf;                         // the reader's batch
    auto survey = [&](int64_t m) {
        info.assign((size_t)m, RecInfo{-1, 0, 0, -1, -1});
        const int64_t per = 64;
        parallel_for((m + per - 1) / per, 0, [&](int64_t tix) {
            for (int64_t k = tix * per; k < std::min(m, (tix + 1) * per); k++) {
                const RecView r = rec_of(rf, k);
                const int32_t rid = r.ref_id();
                if (rid < 0 || rid >= (int32_t)n_refs || contigs[(size_t)rid].ranges.empty()) continue;
                const PurContig &c = contigs[(size_t)rid];
                const int32_t one_layer[2] = {0, (int32_t)c.ranges.size()};
                RecInfo &ri = info[(size_t)k];
                const RecCigar cg = rec_cigar(r);
                ri.gate = cms_gate((uint32_t)r.flag(), r.pos(), r.l_seq(), cg.w, (int)cg.n, exclude_flags, c.ranges.data(), one_layer, 1);
                if (ri.gate < 0) continue;
                const int64_t end = r.pos() + cms_span(cg.w, (int)cg.n).rl;
                ri.w0 = pur_first_dense(c.ranges.data(), (int)c.ranges.size(), r.pos(), end) / run.W;
                ri.w1 = pur_last_dense(c.ranges.data(), (int)c.ranges.size(), r.pos(), end) / run.W;
                if (ri.gate != 0) continue;
                ri.no_entry = pur_ins_no_entry(cg.w, (int)cg.n);
                ri.ins_ops = pur_ins_ops(cg.w, (int)cg.n);
            }
        });
    };
    // true: walked.  first: count what is a matter of the record, not of a window
    auto gate = [&](const RecInfo &ri, bool first) -> bool {
        if (ri.gate > 0 && first) ht[ri.gate]++;
        if (ri.gate != 0) return false;
        if (first) {
            ht[PUR_T_RECORDS]++;
            ht[PUR_T_INS_NO_ENTRY] += ri.no_entry;
        }
        return true;
    };

    const bool one_pass = b->file && !b->blocks.empty() && b->rec_off.empty();
    const int threads = 0;
    InflateRun infl(ctx, b);
    if (one_pass) {
        // ONE PASS over a coordinate-sorted file: the windows advance with the records; a record that reaches past the
        // window's end is carried (a copy of its head) into the next one
        if (int rc = one_pass_args_check(b, (int)h_rid.size(), h_rid.data(), 0)) return rc;
        BamRecordWalker walker(b, (int)h_rid.size(), h_rid.data(), h_lo.data(), h_hi.data(), 0, threads, 0u, infl.hook());
        std::vector<std::shared_ptr<RawBuf>> keep;
        struct Carried { std::vector<uint8_t> bytes; int64_t w1, ins_ops; };
        std::vector<Carried> carry;
        // to window `target` of the current contig, through every window on the way that a carried record has positions in
        auto advance_to = [&](int64_t target) -> int {
            while (run.c && run.w < target) {
                if (int rc = run.finish_window()) return rc;
                std::vector<Carried> still;
                for (Carried &cr : carry)
                    if (cr.w1 > run.w) still.push_back(std::move(cr));
                carry = std::move(still);
                if (carry.empty()) {
                    if (target < run.n_windows()) run.set_window(target);
                    break;
                }
                run.set_window(run.w + 1);
                for (const Carried &cr : carry)
                    if (int rc = run.add(cr.bytes.data(), cr.ins_ops, true)) return rc;
            }
            return NPORE_OK;
        };
        int32_t cur_rid = -1;
        int64_t last_pos = -1;
        for (;;) {
            keep.clear();
            const int64_t m = walker.next_batch(rf, keep, run.batch_reads);
            if (m < 0) return (int)m;
            if (m == 0) break;
            survey(m);
            for (int64_t k = 0; k < m; k++) {
                const RecView r = rec_of(rf, k);
                const int32_t rid = r.ref_id();
                if (rid < 0 || rid >= (int32_t)n_refs || contigs[(size_t)rid].ranges.empty()) continue;
                if (rid == cur_rid && r.pos() < last_pos)
                    return fail(NPORE_E_UNSUPPORTED, "the BAM is not sorted by position: one-pass purity needs a coordinate-sorted file");
                if (rid != cur_rid) {
                    if (int rc = advance_to(INT64_MAX)) return rc;
                    if (int rc = run.finish_window()) return rc;
                    carry.clear();
                    if (int rc = run.set_contig(contigs[(size_t)rid])) return rc;
                    cur_rid = rid;
                }
                last_pos = r.pos();
                const RecInfo &ri = info[(size_t)k];
                if (!gate(ri, true)) continue;
                if (ri.w0 > run.w)
                    if (int rc = advance_to(ri.w0)) return rc;
                if (ri.w1 > run.w) {
                    // (carried as the staged head: its real CIGAR is resolved once)
                    carry.push_back(Carried{std::vector<uint8_t>((size_t)staged_head_bytes(rf.ptr[(size_t)k], true)), ri.w1, ri.ins_ops});
                    stage_record_head(rf.ptr[(size_t)k], true, carry.back().bytes.data());
                    if (int rc = run.add(carry.back().bytes.data(), ri.ins_ops, true)) return rc;
                } else if (int rc = run.add(rf.ptr[(size_t)k], ri.ins_ops)) return rc;
            }
            if (int rc = run.flush()) return rc;     // (the records' bytes go with the reader's next batch)
        }
        if (int rc = advance_to(INT64_MAX)) return rc;
        if (int rc = run.finish_window()) return rc;
    } else {
        // INDEXED reader: select per window
        std::vector<int64_t> idx;
        for (size_t q = 0; q < h_rid.size(); q++) {
            const int32_t rid = h_rid[q];
            const PurContig &c = contigs[(size_t)rid];
            if (int rc = run.set_contig(c)) return rc;
            for (int64_t w = 0; w < run.n_windows(); w++) {
                run.set_window(w);
                const int64_t k = bam_select(b, 1, &rid, &run.ref_lo, &run.ref_hi, 0, nullptr, 0, 0u);
                if (k < 0) return (int)k;
                if (k == 0) continue;
                idx.assign((size_t)k + 1, 0);
                if (bam_select(b, 1, &rid, &run.ref_lo, &run.ref_hi, 0, idx.data(), k, 0u) != k) return fail(NPORE_E_INVALID, "select is not repeatable");
                for (int64_t at = 0; at < k; at += run.batch_reads) {
                    const int64_t m = std::min(run.batch_reads, k - at);
                    if (int rc = fetch_records(b, idx.data() + at, m, threads, rf)) return rc;
                    survey(m);
                    for (int64_t i = 0; i < m; i++) {
                        const RecInfo &ri = info[(size_t)i];
                        if (ri.gate < 0 || w < ri.w0 || w > ri.w1) continue;      // (the window's hull holds positions of no range, too)
                        if (!gate(ri, w == ri.w0)) continue;
                        if (int rc = run.add(rf.ptr[(size_t)i], ri.ins_ops)) return rc;
                    }
                    if (int rc = run.flush()) return rc;
                }
                if (int rc = run.finish_window()) return rc;
            }
        }
    }
    std::vector<unsigned long long> h(PurRun::out_bytes() / 8);
    HIP_TRY(hipMemcpyAsync(h.data(), ctx->pur_out.p, PurRun::out_bytes(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h[2 * PUR_BINS + PUR_D_OVERFLOW] != 0) return fail(NPORE_E_INVALID, "internal: the insertion event buffer was too small");
    for (int k = 0; k < PUR_BINS; k++) { base_hist[k] += (int64_t)h[(size_t)k]; ins_hist[k] += (int64_t)h[(size_t)(PUR_BINS + k)]; }
    for (int k = 0; k < PUR_N_TALLIES; k++) tallies[k] += (int64_t)h[(size_t)(2 * PUR_BINS + k)] + ht[k];
    tallies[PUR_T_WINDOWS] += run.windows;
    tallies[PUR_T_BATCHES] += run.batches;
    tallies[PUR_T_KERNEL_NS] += (int64_t)(run.kernel_ms * 1e6);
    return NPORE_OK;
}
NPORE_CATCH_INT

// debug / self-test entries (used by tests -m gpu)
int npore_debug_inflate(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_len, int force)
{
    if (!in || !out || in_len < 0 || out_len < 0) return fail(NPORE_E_INVALID, "null argument");
    return inflate_block(in, (size_t)in_len, out, (size_t)out_len, force) ? 1 : 0;
}

int npore_debug_inflate_pair(const uint8_t *in_a, int64_t in_len_a, uint8_t *out_a, int64_t out_len_a, const uint8_t *in_b, int64_t in_len_b,
                             uint8_t *out_b, int64_t out_len_b, int force)
{
    if (!in_a || !out_a || !in_b || !out_b || in_len_a < 0 || out_len_a < 0 || in_len_b < 0 || out_len_b < 0) return fail(NPORE_E_INVALID, "null argument");
    // (through the readers' own entry: a list of blocks for one thread; the pair three times over, so that more lanes than
    // two -- NPORE_INFLATE_LANES -- are exercised too: every copy must agree)
    std::vector<uint8_t> ca((size_t)out_len_a * 2 + 1), cb((size_t)out_len_b * 2 + 1);
    const FastInflate::Job jobs[6] = {{in_a, (size_t)in_len_a, out_a, (size_t)out_len_a}, {in_b, (size_t)in_len_b, out_b, (size_t)out_len_b},
                                      {in_a, (size_t)in_len_a, ca.data(), (size_t)out_len_a}, {in_b, (size_t)in_len_b, cb.data(), (size_t)out_len_b},
                                      {in_b, (size_t)in_len_b, cb.data() + out_len_b, (size_t)out_len_b}, {in_a, (size_t)in_len_a, ca.data() + out_len_a, (size_t)out_len_a}};
    bool ok[6] = {false, false, false, false, false, false};
    if (force != 2) inflate_raw_fast_many(jobs, 6, ok);
    if (force != 1)
        for (int k = 0; k < 6; k++)
            if (!ok[k]) ok[k] = inflate_block(jobs[k].in, jobs[k].in_len, jobs[k].out, jobs[k].out_len, 2);
    const bool oa = ok[0], ob = ok[1];
    if (ok[2] != oa || ok[5] != oa || ok[3] != ob || ok[4] != ob) return fail(NPORE_E_INVALID, "copies of one stream disagree");
    if (oa && (std::memcmp(out_a, ca.data(), (size_t)out_len_a) || std::memcmp(out_a, ca.data() + out_len_a, (size_t)out_len_a)))
        return fail(NPORE_E_INVALID, "copies of stream a differ");
    if (ob && (std::memcmp(out_b, cb.data(), (size_t)out_len_b) || std::memcmp(out_b, cb.data() + out_len_b, (size_t)out_len_b)))
        return fail(NPORE_E_INVALID, "copies of stream b differ");
    return (oa ? 1 : 0) | (ob ? 2 : 0);
}

// n streams and where their bytes go: every range inside its buffer, no stream longer than a BGZF member's
static bool inflate_wave_args_ok(const uint8_t *in, int64_t in_bytes, const int64_t *in_off, const int64_t *in_len, const uint8_t *out, int64_t out_bytes,
                                 const int64_t *out_off, const int64_t *out_len, int64_t n, const int32_t *status)
{
    if (n < 0 || in_bytes < 0 || out_bytes < 0 || (in_bytes > 0 && !in) || (out_bytes > 0 && !out)) return false;
    if (n > 0 && (!in_off || !in_len || !out_off || !out_len || !status)) return false;
    for (int64_t k = 0; k < n; k++)
        if (in_off[k] < 0 || in_len[k] < 0 || in_len[k] > (int64_t)IW_MAX_IN || in_off[k] > in_bytes - in_len[k] || out_off[k] < 0 || out_len[k] < 0 ||
            out_len[k] > (int64_t)IW_MAX_OUT || out_off[k] > out_bytes - out_len[k])
            return false;
    return true;
}

int npore_debug_inflate_wave_host(const uint8_t *in, int64_t in_bytes, const int64_t *in_off, const int64_t *in_len, uint8_t *out, int64_t out_bytes,
                                  const int64_t *out_off, const int64_t *out_len, int64_t n, int32_t *status)
{
    if (!inflate_wave_args_ok(in, in_bytes, in_off, in_len, out, out_bytes, out_off, out_len, n, status)) return fail(NPORE_E_INVALID, "bad argument");
    inflate_wave_host(in, in_off, in_len, out, out_off, out_len, n, status);
    return NPORE_OK;
}

int npore_debug_inflate_device(npore_ctx *ctx, const uint8_t *in, int64_t in_bytes, const int64_t *in_off, const int64_t *in_len, uint8_t *out,
                               int64_t out_bytes, const int64_t *out_off, const int64_t *out_len, int64_t n, int32_t *status)
try {
    if (!ctx || !inflate_wave_args_ok(in, in_bytes, in_off, in_len, out, out_bytes, out_off, out_len, n, status)) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = quiesce(ctx)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return NPORE_OK;
    DevBuf d_in, d_out, d_meta;
    if (int rc = d_in.ensure((size_t)in_bytes + 64)) return rc;
    if (int rc = d_out.ensure((size_t)out_bytes + 64)) return rc;
    if (int rc = d_meta.ensure((size_t)n * 36)) return rc;
    int64_t *const dm = d_meta.as<int64_t>();
    int32_t *const d_status = reinterpret_cast<int32_t *>(dm + 4 * n);
    hipStream_t s = ctx->s_post;
    if (in_bytes > 0) HIP_TRY(hipMemcpyAsync(d_in.p, in, (size_t)in_bytes, hipMemcpyHostToDevice, s));
    if (out_bytes > 0) HIP_TRY(hipMemcpyAsync(d_out.p, out, (size_t)out_bytes, hipMemcpyHostToDevice, s));
    const int64_t *const host4[4] = {in_off, in_len, out_off, out_len};
    for (int q = 0; q < 4; q++) HIP_TRY(hipMemcpyAsync(dm + q * n, host4[q], (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n * 4, s));
    launch_inflate_blocks(d_in.as<uint8_t>(), dm, dm + n, d_out.as<uint8_t>(), dm + 2 * n, dm + 3 * n, n, d_status, s);
    HIP_TRY(hipGetLastError());
    if (out_bytes > 0) HIP_TRY(hipMemcpyAsync(out, d_out.p, (size_t)out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(status, d_status, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return NPORE_OK;
}
NPORE_CATCH_INT

int npore_bam_inflate_info(const npore_bam *b, int64_t *out8)
{
    if (!b || !out8) return fail(NPORE_E_INVALID, "null argument");
    for (int k = 0; k < 8; k++) out8[k] = b->inflate_info[k];
    return NPORE_OK;
}

int64_t npore_debug_crc32(const uint8_t *p, int64_t n, uint32_t crc)
{
    if ((!p && n > 0) || n < 0) return fail(NPORE_E_INVALID, "null argument");
    return (int64_t)crc32_fast(crc, p, (size_t)n);
}

int64_t npore_debug_deflate_member_mode(const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int mode)
try {
    if ((!in && n > 0) || !out || n < 0 || n > (int64_t)BGZF_STORED_PAYLOAD || cap < n + (int64_t)BGZF_STORED_OVERHEAD ||
        (mode != DEFLATE_MODE_HUFFMAN && mode != DEFLATE_MODE_MATCH))
        return fail(NPORE_E_INVALID, "bad argument");
    return (int64_t)deflate_member_host(in, (size_t)n, crc32_fast(0, in, (size_t)n), out, mode);
}
NPORE_CATCH_INT

int64_t npore_debug_deflate_member(const uint8_t *in, int64_t n, uint8_t *out, int64_t cap)
{
    return npore_debug_deflate_member_mode(in, n, out, cap, DEFLATE_MODE_HUFFMAN);
}

int npore_debug_deflate_device(npore_ctx *ctx, const uint8_t *bytes, int64_t n, int64_t phase, uint8_t *members, int64_t members_cap,
                               uint32_t *sizes, int64_t sizes_cap, uint8_t *head, uint8_t *tail, int64_t *info)
{
    return npore_debug_deflate_device_mode(ctx, bytes, n, phase, members, members_cap, sizes, sizes_cap, head, tail, info, DEFLATE_MODE_HUFFMAN);
}

int npore_debug_deflate_device_mode(npore_ctx *ctx, const uint8_t *bytes, int64_t n, int64_t phase, uint8_t *members, int64_t members_cap,
                                    uint32_t *sizes, int64_t sizes_cap, uint8_t *head, uint8_t *tail, int64_t *info, int mode)
try {
    if (!ctx || (mode != DEFLATE_MODE_HUFFMAN && mode != DEFLATE_MODE_MATCH) || (!bytes && n > 0) || n < 0 || phase < 0 || !info || members_cap < 0 || sizes_cap < 0 || (members_cap > 0 && !members) ||
        (sizes_cap > 0 && !sizes) || !head || !tail)
        return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = quiesce(ctx)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    npore_batch_slot s;
    DevBuf d_recs, d_total;
    const unsigned long long total = (unsigned long long)n, pos = (unsigned long long)phase;
    if (int rc = d_recs.ensure((size_t)n + 64)) return rc;
    if (int rc = d_total.ensure(64)) return rc;
    if (int rc = ctx->d_stream_pos.ensure(64)) return rc;
    if (int rc = slot_deflate_buffers(s, n, mode)) return rc;
    if (n > 0) HIP_TRY(hipMemcpy(d_recs.p, bytes, (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_total.p, &total, 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_stream_pos.p, &pos, 8, hipMemcpyHostToDevice));
    const DeflateParams dp = slot_deflate_params(s, d_recs.as<uint8_t>(), d_total.as<unsigned long long>(), ctx->d_stream_pos.as<unsigned long long>(), mode);
    launch_deflate(dp, ctx->s_post);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->s_post));
    int64_t in4[4];
    unsigned long long pos_after = 0;
    HIP_TRY(hipMemcpy(in4, dp.info, 32, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&pos_after, ctx->d_stream_pos.p, 8, hipMemcpyDeviceToHost));
    const int64_t nm = in4[0], comp = in4[1], hd = in4[2], tl = in4[3];
    if (nm < 0 || nm > s.max_members || hd < 0 || tl < 0 || hd + nm * (int64_t)BGZF_STORED_PAYLOAD + tl != n || comp < 0 || comp > dp.comp_cap)
        return fail(NPORE_E_HIP, "internal: the coded members do not add up to the buffer's bytes");
    if (nm > sizes_cap || comp > members_cap) return fail(NPORE_E_INVALID, "the members need more room than the caller gave");
    if (nm > 0) HIP_TRY(hipMemcpy(sizes, dp.sizes, (size_t)nm * 4, hipMemcpyDeviceToHost));
    if (comp > 0) HIP_TRY(hipMemcpy(members, dp.comp, (size_t)comp, hipMemcpyDeviceToHost));
    if (hd > 0) HIP_TRY(hipMemcpy(head, dp.comp + comp, (size_t)hd, hipMemcpyDeviceToHost));           // (where emit_deflate_kernel put them)
    if (tl > 0) HIP_TRY(hipMemcpy(tail, dp.comp + comp + hd, (size_t)tl, hipMemcpyDeviceToHost));
    info[0] = nm; info[1] = comp; info[2] = hd; info[3] = tl; info[4] = (int64_t)pos_after;
    return NPORE_OK;
}
NPORE_CATCH_INT

int npore_debug_dpp(uint32_t *out128)
{
    DevBuf d;
    if (int rc = d.ensure(128 * 4)) return rc;
    hipLaunchKernelGGL(dpp_selftest_kernel, dim3(1), dim3(64), 0, 0, d.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out128, d.p, 128 * 4, hipMemcpyDeviceToHost));
    return NPORE_OK;
}

int npore_debug_divcheck(int64_t *mismatches)
{
    DevBuf d;
    unsigned long long h = 0;
    if (int rc = d.ensure(8)) return rc;
    HIP_TRY(hipMemset(d.p, 0, 8));
    hipLaunchKernelGGL(divcheck_kernel, dim3(256), dim3(256), 0, 0, d.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&h, d.p, 8, hipMemcpyDeviceToHost));
    *mismatches = (int64_t)h;
    return NPORE_OK;
}

// Copies the device-prepared arrays of the LAST group of the last align call to the host
// (what: 0 steps, 1 inss, 2 descs, 3 seqw, 4 refw, 5 refl, 6 sched, 7 counters).
int npore_debug_fetch(npore_ctx *ctx, int what, void *dst, int64_t bytes)
{
    if (!ctx || !dst) return fail(NPORE_E_INVALID, "null argument");
    if (int rc = quiesce(ctx)) return rc;
    WorkSet *w = ctx->last_ws ? ctx->last_ws : &ctx->ws[0];
    DevBuf *b[] = {&w->steps, &w->inss, &w->descs, &w->seqw, &w->refw, &w->refl, &w->sched, &w->counters};
    if (what < 0 || what > 7) return fail(NPORE_E_INVALID, "bad selector");
    if ((size_t)bytes > b[what]->cap) return fail(NPORE_E_INVALID, "more bytes than the buffer holds");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(dst, b[what]->p, bytes, hipMemcpyDeviceToHost));
    return NPORE_OK;
}

// Debug: `bytes` of the last group's traceback words from byte `offset` on (a chunk's words start at 4 * tb_off of its
// descriptor, one row of tb_stride(r) words per anti-diagonal)
#if defined(NPORE_EXPERIMENTS)
extern "C" int npore_debug_fetch_dbg(npore_ctx *ctx, int64_t offset, void *dst, int64_t bytes)
{
    if (!ctx || !dst || offset < 0 || bytes < 0) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = quiesce(ctx)) return rc;
    WorkSet *w = ctx->last_ws ? ctx->last_ws : &ctx->ws[0];
    if ((size_t)(offset + bytes) > w->dbg.cap) return fail(NPORE_E_INVALID, "beyond the debug buffer");
    HIP_TRY(hipMemcpy(dst, static_cast<const char *>(w->dbg.p) + offset, bytes, hipMemcpyDeviceToHost));
    return NPORE_OK;
}
#endif
int npore_debug_fetch_tb(npore_ctx *ctx, int64_t offset, void *dst, int64_t bytes)
{
    if (!ctx || !dst || offset < 0 || bytes < 0) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = quiesce(ctx)) return rc;
    WorkSet *w = ctx->last_ws ? ctx->last_ws : &ctx->ws[0];
    if ((size_t)(offset + bytes) > w->tb.cap) return fail(NPORE_E_INVALID, "beyond the traceback buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(dst, static_cast<const char *>(w->tb.p) + offset, bytes, hipMemcpyDeviceToHost));
    return NPORE_OK;
}


// ---- BAM ingest / SAM emit (bam_reader.hpp) -----------------------------------------------------
// mode 0: automatic (streamed when the file is BGZF and larger than NPORE_BAM_STREAM_MB, default 1024 MB), 1: whole file
// resident, 2: streamed, 3: one-pass (header only; the reads through npore_bam_realign_sequential).  index_path (may be NULL): a record index saved by npore_bam_save_index for this very file --
// a streamed handle then skips its indexing pass (one process of a node indexes, the others load).
npore_bam *npore_bam_open_mode(const char *path, int threads, int mode, const char *index_path)
try {
    return bam_open(path, threads, mode, index_path);
}
NPORE_CATCH_PTR
npore_bam *npore_bam_open(const char *path, int threads) { return npore_bam_open_mode(path, threads, 0, nullptr); }
int npore_bam_is_streamed(const npore_bam *b) { return b && b->streamed ? 1 : 0; }

// The record index of a handle (header + per-record offsets and metadata: 22 bytes per record), complete or not there
// at all, for npore_bam_open_mode(..., index_path) in the other processes of a node.
int npore_bam_save_index(const npore_bam *b, const char *path)
try {
    return bam_save_index(b, path);
}
NPORE_CATCH_INT
void npore_bam_close(npore_bam *b) { delete b; }

int64_t npore_bam_inflated_size(const npore_bam *b) { return b ? (int64_t)b->data_size : 0; }

int npore_bam_dump_inflated(const npore_bam *b, const char *path)
try {
    return bam_dump_inflated(b, path);
}
NPORE_CATCH_INT
int64_t npore_bam_n_records(const npore_bam *b) { return b ? (int64_t)b->rec_off.size() : 0; }
int npore_bam_n_refs(const npore_bam *b) { return b ? (int)b->ref_names.size() : 0; }
const char *npore_bam_ref_name(const npore_bam *b, int i) { return (b && i >= 0 && i < (int)b->ref_names.size()) ? b->ref_names[(size_t)i].c_str() : ""; }
int64_t npore_bam_ref_len(const npore_bam *b, int i) { return (b && i >= 0 && i < (int)b->ref_lens.size()) ? b->ref_lens[(size_t)i] : -1; }
int npore_bam_ref_has_reads(const npore_bam *b, int i) { return (b && i >= 0 && i < (int)b->ref_has_reads.size()) ? b->ref_has_reads[(size_t)i] : 0; }

int64_t npore_bam_select(const npore_bam *b, int n_regions, const int32_t *ref_id, const int64_t *start, const int64_t *stop,
                         int64_t max_reads, int64_t *out_idx, int64_t cap)
{
    return bam_select(b, n_regions, ref_id, start, stop, max_reads, out_idx, cap);
}

// ... keeping the records whose flag has a bit of flag_mask (a subset of 0x904), to pass through (npore_bam_set_output_pass)
int64_t npore_bam_select_pass(const npore_bam *b, int n_regions, const int32_t *ref_id, const int64_t *start, const int64_t *stop,
                              int64_t max_reads, int flag_mask, int64_t *out_idx, int64_t cap)
{
    if (flag_mask & ~(int)PASS_FLAGS) return fail(NPORE_E_INVALID, "bad argument");
    return bam_select(b, n_regions, ref_id, start, stop, max_reads, out_idx, cap, PASS_FLAGS, (uint32_t)flag_mask);
}

npore_fasta *npore_fasta_open(const char *path)
try {
    if (!path) { fail(NPORE_E_INVALID, "null path"); return nullptr; }
    MappedFile mf;
    if (!mf.open(path)) { fail(NPORE_E_INVALID, std::string("could not open FASTA '") + path + "'"); return nullptr; }
    std::unique_ptr<npore_fasta> hold(new npore_fasta());
    static std::atomic<uint64_t> next_serial{1};
    hold->serial = next_serial.fetch_add(1);
    npore_fasta *f = hold.get();
    if (!fasta_parse(ByteSpan{mf.p, mf.n}, 0, *f)) { fail(NPORE_E_NOMEM, "FASTA: out of memory"); return nullptr; }
    return hold.release();
}
NPORE_CATCH_PTR
void npore_fasta_close(npore_fasta *f) { delete f; }
int npore_fasta_n(const npore_fasta *f) { return f ? (int)f->names.size() : 0; }
const char *npore_fasta_name(const npore_fasta *f, int i) { return (f && i >= 0 && i < (int)f->names.size()) ? f->names[(size_t)i].c_str() : ""; }
const char *npore_fasta_seq(const npore_fasta *f, int i) { return (f && i >= 0 && i < (int)f->names.size()) ? f->seq((size_t)i) : nullptr; }
int64_t npore_fasta_len(const npore_fasta *f, int i) { return (f && i >= 0 && i < (int)f->names.size()) ? f->len((size_t)i) : -1; }

int npore_bam_pack_sizes(const npore_bam *b, const int64_t *idx, int64_t n, int64_t *ref_off, int64_t *seq_off, int64_t *cig_off)
try {
    if (!pack_args_ok(b, idx, n) || !ref_off || !seq_off || !cig_off) return fail(NPORE_E_INVALID, "bad argument");
    RecFetch rf;          // (local to the call: the handle is const here, and two threads may size / pack from one handle)
    if (int rc = fetch_records(b, idx, n, 0, rf)) return rc;
    pack_sizes_of(rf, n, ref_off, seq_off, cig_off, 0, b->out_rec.pass_mask);      // (a record that passes has empty slices)
    return NPORE_OK;
}
NPORE_CATCH_INT

int npore_bam_pack(const npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx, int64_t n,
                   uint8_t *refs, const int64_t *ref_off, uint8_t *seqs, const int64_t *seq_off, char *cigs,
                   const int64_t *cig_off, int threads)
try {
    if (!pack_args_ok(b, idx, n) || !fa || !fasta_of_ref || !ref_off || !seq_off || !cig_off ||
        (n > 0 && (!refs || !seqs || !cigs)))
        return fail(NPORE_E_INVALID, "bad argument");
    RecFetch rf;
    if (int rc = fetch_records(b, idx, n, threads, rf)) return rc;
    return pack_records(b, rf, fa, fasta_of_ref, n, refs, ref_off, seqs, seq_off, cigs, cig_off, threads, false, b->out_rec.pass_mask);
}
NPORE_CATCH_INT

int npore_bam_format_sam(npore_bam *b, const int64_t *idx, int64_t n, const char *finals, const int64_t *final_off,
                         const int64_t *final_len, const int32_t *status, int threads, const char **sam, int64_t *sam_len)
try {
    if (!pack_args_ok(b, idx, n) || !sam) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = fetch_records(b, idx, n, threads, b->api_fetch)) return rc;
    const int rc = format_sam_into(b, b->api_fetch, n, finals, final_off, final_len, status, threads, b->sam, sam_len);
    *sam = b->sam.p;
    return rc;
}
NPORE_CATCH_INT

int npore_bam_format_bam(npore_bam *b, const int64_t *idx, int64_t n, const char *finals, const int64_t *final_off,
                         const int64_t *final_len, const int32_t *status, int threads, const uint8_t **recs, int64_t *recs_len)
try {
    if (!pack_args_ok(b, idx, n) || !recs) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = fetch_records(b, idx, n, threads, b->api_fetch)) return rc;
    const int rc = format_bam_into(b, b->api_fetch, n, finals, final_off, final_len, status, threads, b->recs, recs_len, nullptr, ReadCodes{});
    *recs = reinterpret_cast<const uint8_t *>(b->recs.p);
    return rc;
}
NPORE_CATCH_INT

namespace {
// the code arrays align() would get of the fetched records (pack_records), for the FULL records' NM
struct PackedCodes {
    std::vector<int64_t> ro, so, co;
    std::vector<uint8_t> refs, seqs;
    std::vector<char> cigs;
    int pack(const npore_bam *b, const RecFetch &rf, const npore_fasta *fa, const int32_t *fasta_of_ref, int64_t n, int threads, uint32_t pass_mask)
    {
        for (auto *v : {&ro, &so, &co}) v->assign((size_t)n + 1, 0);
        pack_sizes_of(rf, n, ro.data(), so.data(), co.data(), threads, pass_mask);
        refs.resize((size_t)ro[(size_t)n] + 64); seqs.resize((size_t)so[(size_t)n] + 64); cigs.resize((size_t)co[(size_t)n] + 64);
        return pack_records(b, rf, fa, fasta_of_ref, n, refs.data(), ro.data(), seqs.data(), so.data(), cigs.data(), co.data(), threads, false, pass_mask);
    }
};
}  // namespace

int npore_bam_format_bam_full(npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx, int64_t n,
                              const char *finals, const int64_t *final_off, const int64_t *final_len, const int32_t *status, int threads,
                              const uint8_t **recs, int64_t *recs_len)
{
    return npore_bam_format_bam_full_md(b, fa, fasta_of_ref, idx, n, finals, final_off, final_len, status, threads, recs, recs_len, 0);
}

// ... with flags: NPORE_OUT_MD, the MD tag behind NM (0: the records above)
int npore_bam_format_bam_full_md(npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx, int64_t n,
                                 const char *finals, const int64_t *final_off, const int64_t *final_len, const int32_t *status, int threads,
                                 const uint8_t **recs, int64_t *recs_len, int flags)
{
    return npore_bam_format_bam_full_tags(b, fa, fasta_of_ref, idx, n, finals, final_off, final_len, status, threads, recs, recs_len, flags, 0);
}

// The FULL records of the host and debug entries, whose `flags` know NPORE_OUT_MD alone: what the three setters make of the same
// options for a FULL BAM run (rec_spec_of)
static bool full_rec_spec(int flags, int tags, int pass_mask, RecSpec &rec)
{
    return !(flags & ~NPORE_OUT_MD) && rec_spec_of(NPORE_OUT_BAM, NPORE_OUT_FULL | flags, tags, pass_mask, rec);
}

// ... and with tags: NPORE_TAG_*, cs and de behind MD (0: the records above)
int npore_bam_format_bam_full_tags(npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx, int64_t n,
                                   const char *finals, const int64_t *final_off, const int64_t *final_len, const int32_t *status, int threads,
                                   const uint8_t **recs, int64_t *recs_len, int flags, int tags)
{
    return npore_bam_format_bam_full_pass(b, fa, fasta_of_ref, idx, n, finals, final_off, final_len, status, threads, recs, recs_len, flags, tags, 0);
}

// ... and with pass_mask: the records whose flag has one of its bits (a subset of 0x904) are the input's bytes (0: the records above)
int npore_bam_format_bam_full_pass(npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx, int64_t n,
                                   const char *finals, const int64_t *final_off, const int64_t *final_len, const int32_t *status, int threads,
                                   const uint8_t **recs, int64_t *recs_len, int flags, int tags, int pass_mask)
try {
    RecSpec rec;
    if (!pack_args_ok(b, idx, n) || !fa || !fasta_of_ref || !recs || !full_rec_spec(flags, tags, pass_mask, rec)) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = fetch_records(b, idx, n, threads, b->api_fetch)) return rc;
    PackedCodes pc;
    if (int rc = pc.pack(b, b->api_fetch, fa, fasta_of_ref, n, threads, rec.pass_mask)) return rc;
    const ReadCodes codes{rec, pc.refs.data(), pc.ro.data(), pc.seqs.data(), pc.so.data()};
    const int rc = format_bam_into(b, b->api_fetch, n, finals, final_off, final_len, status, threads, b->recs, recs_len, nullptr, codes);
    *recs = reinterpret_cast<const uint8_t *>(b->recs.p);
    return rc;
}
NPORE_CATCH_INT

// The device side of the FULL records on a caller's final CIGARs: the inputs of npore_bam_format_bam_full through the
// staging (STAGE_FULL), unpack_records_kernel, nm_count_kernel, place_bam_full_kernel and emit_bam_full_kernel, and back
int npore_debug_format_bam_full_device(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx,
                                       int64_t n, const char *finals, const int64_t *final_off, const int64_t *final_len, const int32_t *status,
                                       uint8_t *recs, int64_t cap, int64_t *recs_len, int32_t *nm)
{
    return npore_debug_format_bam_full_md_device(ctx, b, fa, fasta_of_ref, idx, n, finals, final_off, final_len, status, recs, cap, recs_len, nm, 0, nullptr);
}

// ... with flags: NPORE_OUT_MD puts md_size_kernel in front of the placement and emit_md_kernel behind the records; the
// reads' MD text lengths to md_len[n]
int npore_debug_format_bam_full_md_device(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx,
                                          int64_t n, const char *finals, const int64_t *final_off, const int64_t *final_len, const int32_t *status,
                                          uint8_t *recs, int64_t cap, int64_t *recs_len, int32_t *nm, int flags, int32_t *md_len)
{
    return npore_debug_format_bam_full_tags_device(ctx, b, fa, fasta_of_ref, idx, n, finals, final_off, final_len, status, recs, cap, recs_len, nm, flags,
                                                   md_len, 0);
}

// ... and with tags: NPORE_TAG_* puts cs_size_kernel beside md_size_kernel and emit_cs_kernel behind emit_md_kernel
int npore_debug_format_bam_full_tags_device(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx,
                                            int64_t n, const char *finals, const int64_t *final_off, const int64_t *final_len, const int32_t *status,
                                            uint8_t *recs, int64_t cap, int64_t *recs_len, int32_t *nm, int flags, int32_t *md_len, int tags)
{
    return npore_debug_format_bam_full_pass_device(ctx, b, fa, fasta_of_ref, idx, n, finals, final_off, final_len, status, recs, cap, recs_len, nm, flags,
                                                   md_len, tags, 0);
}

// ... and with pass_mask: a record that passes is staged verbatim, skipped by the unpack and tag kernels, placed by its own size
// and copied by one wave
int npore_debug_format_bam_full_pass_device(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx,
                                            int64_t n, const char *finals, const int64_t *final_off, const int64_t *final_len, const int32_t *status,
                                            uint8_t *recs, int64_t cap, int64_t *recs_len, int32_t *nm, int flags, int32_t *md_len, int tags,
                                            int pass_mask)
try {
    RecSpec rec;
    if (!ctx || !pack_args_ok(b, idx, n) || !fa || !fasta_of_ref || !recs_len || cap < 0 || (cap > 0 && !recs) || !full_rec_spec(flags, tags, pass_mask, rec) ||
        (n > 0 && (!finals || !final_off || !final_len || !status || !nm || (rec.md && !md_len))))
        return fail(NPORE_E_INVALID, "bad argument");
    *recs_len = 0;
    if (n == 0) return NPORE_OK;
    if (int rc = quiesce(ctx)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = device_fasta(ctx, b, fa, fasta_of_ref)) return rc;
    RecFetch &rf = b->api_fetch;
    if (int rc = fetch_records(b, idx, n, 0, rf)) return rc;
    // stage: sizes, the finals as words in slots at multiples of 4, and the file pipeline's plan of the staged heads with the
    // bound of a caller's final (plan_staged_heads; hostio.hpp words_final_extent)
    const size_t N = (size_t)n;
    std::vector<int64_t> off(OFF_ARRAYS * (N + 1), 0), aux(N, 0), wlen(N, 0);
    int64_t *ro = group_off(off.data(), OFF_REF, n), *so = group_off(off.data(), OFF_SEQ, n), *co = group_off(off.data(), OFF_CIG, n),
            *wo = group_off(off.data(), OFF_OUT, n), *rawo = group_off(off.data(), OFF_RAW, n);
    pack_sizes_of(rf, n, ro, so, co, 0, rec.pass_mask);
    std::vector<std::vector<uint8_t>> fin(N);
    for (size_t k = 0; k < N; k++) {
        const bool skip = (status[k] & NPORE_ST_BAD_INPUT) || staged_passes(rec_of(rf, (int64_t)k).p, rec.pass_mask);
        const int64_t ops = skip ? 0 : cigar_text_ops(finals + final_off[k], final_len[k]);
        if (ops < 0) return fail(NPORE_E_UNSUPPORTED, "a final CIGAR is no CIGAR text (BAM output)");
        if (!skip) fin[k] = cigar_text_words(finals + final_off[k], final_len[k], ops);
        wlen[k] = 4 * ops;
        wo[k + 1] = wo[k] + 4 * ops + 16;
    }
    int64_t bound = 0;
    if (int rc = plan_staged_heads(b, rf, n, fasta_of_ref, (int)fa->names.size(), rec, STAGE_FULL, so, rawo, aux.data(), &bound,
                                   [&](int64_t k) { return words_final_extent(fin[(size_t)k].data(), wlen[(size_t)k] / 4); }))
        return rc;
    std::vector<uint8_t> raw((size_t)rawo[N] + 64, 0), words((size_t)wo[N] + 64, 0);
    for (size_t k = 0; k < N; k++) {
        stage_record(rf.ptr[k], STAGE_FULL, raw.data() + rawo[k], rec);
        if (wlen[k]) std::memcpy(words.data() + wo[k], fin[k].data(), (size_t)wlen[k]);
    }
    // ... into a work set as upload_group leaves a staged group there, and the shared wiring (align_engine.hpp)
    WorkSet w;
    DevBuf d_recs, d_cursor;
    int rce = 0;
    if ((rce = w.in_raw.ensure(raw.size())) || (rce = w.in_off.ensure(off.size() * 8)) || (rce = w.out.ensure(words.size())) ||
        (rce = w.in_refs.ensure((size_t)ro[N] + 64)) || (rce = w.in_seqs.ensure((size_t)so[N] + 64)) || (rce = w.in_cigs.ensure((size_t)co[N] + 64)) ||
        (rce = d_recs.ensure((size_t)bound + 64)) || (rce = d_cursor.ensure(64)) || (rce = w.status.ensure(N * 4 + 64)) || (rce = w.reserve_emit_tags(rec, N)))
        return rce;
    for (DevBuf *d : {&w.out_len, &w.in_hp, &w.rec_off, &w.rec_len})
        if (int rc = d->ensure(N * 8 + 64)) return rc;
    HIP_TRY(hipMemcpy(w.in_raw.p, raw.data(), raw.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.in_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.out.p, words.data(), words.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.out_len.p, wlen.data(), N * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.in_hp.p, aux.data(), N * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.status.p, status, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_cursor.p, 0, 8));
    hipStream_t st = ctx->s_post;
    hipLaunchKernelGGL(unpack_records_kernel, dim3((unsigned)n), dim3(256), 0, st, wire_unpack(&w, n, ctx->d_ctg.as<CtgEntry>(), ctx->n_ctg, rec.pass_mask));
    launch_bam_emit(wire_bam_emit(&w, n, d_recs.as<uint8_t>(), bound, d_cursor.as<unsigned long long>(), rec), true, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    // copy back
    unsigned long long total = 0;
    std::vector<int64_t> rlen(N, 0);
    HIP_TRY(hipMemcpy(&total, d_cursor.p, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rlen.data(), w.rec_len.p, N * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nm, w.nm.p, N * 4, hipMemcpyDeviceToHost));
    if (rec.md) HIP_TRY(hipMemcpy(md_len, w.md_len.p, N * 4, hipMemcpyDeviceToHost));
    if (int rc = check_record_sizes(rlen.data(), n, (int64_t)total, bound)) return rc;
    if ((int64_t)total > cap) return fail(NPORE_E_INVALID, "the records need more room than the caller gave");
    if (total > 0) HIP_TRY(hipMemcpy(recs, d_recs.p, (size_t)total, hipMemcpyDeviceToHost));
    *recs_len = (int64_t)total;
    return NPORE_OK;
}
NPORE_CATCH_INT

int npore_bam_set_output(npore_bam *b, int format, const char *bai_path, int flags)
{
    // the writer's own rules (a FULL run says what it writes: the end of a file or a rank's part); the records': rec_spec_of
    RecSpec rec;
    if (!b || (format != NPORE_OUT_SAM && format != NPORE_OUT_BAM) || ((flags & NPORE_OUT_DEFLATE) && format != NPORE_OUT_BAM) ||
        ((flags & NPORE_OUT_MATCH) && !(flags & NPORE_OUT_DEFLATE)) || ((flags & NPORE_OUT_FULL) && !(flags & (NPORE_OUT_EOF | NPORE_OUT_PART))) ||
        !rec_spec_of(format, flags, 0, 0, rec))
        return fail(NPORE_E_INVALID, "bad argument");
    b->out_format = format;
    b->out_bai = (format == NPORE_OUT_BAM && bai_path) ? bai_path : "";
    b->out_flags = flags;
    b->out_rec = rec;
    return NPORE_OK;
}

// The two setters behind a FULL npore_bam_set_output (only a FULL record can be the input's or carry cs and de): the setting's
// spec made again with the one option replaced
static int set_output_option(npore_bam *b, int tags, int pass)
{
    if (!b || !b->out_rec.full || !rec_spec_of(b->out_format, b->out_flags, tags, pass, b->out_rec)) return fail(NPORE_E_INVALID, "bad argument");
    return NPORE_OK;
}
int npore_bam_set_output_pass(npore_bam *b, int flag_mask) { return set_output_option(b, b ? b->out_rec.tags : 0, flag_mask); }
int npore_bam_set_output_tags(npore_bam *b, int tags) { return set_output_option(b, tags, b ? (int)b->out_rec.pass_mask : 0); }

int npore_bam_output_info(const npore_bam *b, int64_t *out4)
{
    if (!b || !out4) return fail(NPORE_E_INVALID, "null argument");
    for (int k = 0; k < 4; k++) out4[k] = b->out_info[k];
    return NPORE_OK;
}

int npore_bam_write_file(npore_bam *b, const int64_t *idx, int64_t n, int64_t batch_reads, const char *finals, const int64_t *final_off,
                         const int64_t *final_len, const int32_t *status, int threads, const char *out_path)
try {
    if (!pack_args_ok(b, idx, n) || !out_path || batch_reads < 1 || (n > 0 && (!finals || !final_off || !final_len || !status)))
        return fail(NPORE_E_INVALID, "bad argument");
    if (b->out_format != NPORE_OUT_BAM) return fail(NPORE_E_INVALID, "npore_bam_write_file writes BAM: npore_bam_set_output first");
    BgzfStoredWriter w;
    const OutputSetting o = take_output_setting(b);
    if (o.rec.full)
        return fail(NPORE_E_UNSUPPORTED, "npore_bam_write_file has no reference to count NM from: FULL records come from a realign run or npore_bam_format_bam_full");
    if (int rc = w.open(out_path, b->ref_names.size(), o.bai.empty() ? nullptr : o.bai.c_str(), (o.flags & NPORE_OUT_EOF) != 0,
                        (o.flags & NPORE_OUT_PART) != 0, out_deflate_mode(o.flags), host_threads(threads))) return rc;
    std::vector<BamRecMeta> meta;
    for (int64_t k0 = 0; k0 < n; k0 += batch_reads) {
        const int64_t m = std::min(batch_reads, n - k0);
        if (int rc = fetch_records(b, idx + k0, m, threads, b->api_fetch)) return rc;
        int64_t len = 0;
        if (int rc = format_bam_into(b, b->api_fetch, m, finals, final_off + k0, final_len + k0, status + k0, threads, b->recs, &len, &meta, ReadCodes{})) return rc;
        if (int rc = w.add(reinterpret_cast<const uint8_t *>(b->recs.p), len, meta.data(), (int64_t)meta.size())) return rc;
    }
    return w.finish(b->out_info);
}
NPORE_CATCH_INT

int npore_bam_realign_batch(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx,
                            int64_t n, float indel_start, float indel_extend, int max_b_rows, int r, int threads,
                            const char **sam, int64_t *sam_len, int32_t *status)
try {
    if (!ctx || !b || !status || !sam || !sam_len) return fail(NPORE_E_INVALID, "null argument");
    using clk = std::chrono::steady_clock;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!pack_args_ok(b, idx, n)) return fail(NPORE_E_INVALID, "bad argument");
    if (!ctx->slots[0]) ctx->slots[0] = new npore_batch_slot();
    npore_batch_slot &s = *ctx->slots[0];
    const PipeMode host{};                 // one synchronous batch: host pack, host glue, SAM text
    auto t0 = clk::now();
    s.m = n;
    if (int rc = fetch_records(b, idx, n, threads, s.rf)) return rc;
    if (int rc = slot_pack(b, fa, fasta_of_ref, threads, s, host)) return rc;
    b->stage_ms[0] = ms_since(t0);
    t0 = clk::now();
    if (int rc = npore_align_batch(ctx, n, reinterpret_cast<uint8_t *>(s.refs.p), s.ro.data(), reinterpret_cast<uint8_t *>(s.seqs.p), s.so.data(), s.cigs.p,
                                   s.co.data(), indel_start, indel_extend, max_b_rows, r, s.alns.p, s.oo.data(), s.olen.data(), status)) return rc;
    b->stage_ms[1] = ms_since(t0);
    t0 = clk::now();
    double ms_std = 0.0;
    const int rc = slot_collect(b, status, threads, s, host, &ms_std);
    b->stage_ms[2] = ms_std;
    b->stage_ms[3] = ms_since(t0) - ms_std;
    *sam = s.sam.p; *sam_len = s.sam_len;
    return rc;
}
NPORE_CATCH_INT

int npore_bam_set_share(npore_bam *b, int rank, int world, const char *bai_path)
try {
    return bam_set_share(b, rank, world, bai_path);
}
NPORE_CATCH_INT

int npore_bam_share_info(const npore_bam *b, int64_t *out4)
{
    if (!b || !out4) return fail(NPORE_E_INVALID, "null argument");
    out4[0] = b->has_share ? 1 : 0;
    out4[1] = b->share_begin == UINT64_MAX ? -1 : (int64_t)b->share_begin;
    out4[2] = b->share_end == UINT64_MAX ? -1 : (int64_t)b->share_end;
    out4[3] = (int64_t)b->share_block;
    return NPORE_OK;
}

int npore_bam_realign_file(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx,
                           int64_t n, int64_t batch_reads, float indel_start, float indel_extend, int max_b_rows, int r,
                           int threads, const char *out_path, int32_t *status)
try {
    if (!ctx || !b || !fa || !fasta_of_ref || !out_path || (n > 0 && (!idx || !status)) || batch_reads < 1 || !pack_args_ok(b, idx, n))
        return fail(NPORE_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    RunOutput out;
    if (int rco = out.open(b, out_path, threads)) return rco;
    int rc = file_pipeline(ctx, b, fa, fasta_of_ref, AlignKnobs{indel_start, indel_extend, max_b_rows, r}, threads, out, false,
                           [&](int64_t k, npore_batch_slot &s) -> int64_t {
                               const int64_t m = std::min(batch_reads, n - k * batch_reads);
                               if (m <= 0) return 0;
                               const int rcf = fetch_records(b, idx + k * batch_reads, m, threads, s.rf);
                               return rcf ? (int64_t)rcf : m;
                           },
                           [&](int64_t k, int64_t m, const int32_t *st) { std::memcpy(status + k * batch_reads, st, (size_t)m * 4); });
    return out.close(rc);
}
NPORE_CATCH_INT

int npore_bam_realign_sequential(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, int n_regions,
                                 const int32_t *ref_id, const int64_t *start, const int64_t *stop, int64_t max_reads,
                                 int64_t batch_reads, float indel_start, float indel_extend, int max_b_rows, int r, int threads,
                                 const char *out_path, int64_t *counts, int64_t *bad_ord, int32_t *bad_status, int64_t bad_cap)
try {
    if (!ctx || !b || !fa || !fasta_of_ref || !out_path || !counts || batch_reads < 1 || n_regions < 0 ||
        (n_regions > 0 && (!ref_id || !start || !stop)) || (bad_cap > 0 && (!bad_ord || !bad_status)))
        return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = one_pass_args_check(b, n_regions, ref_id, max_reads)) return rc;
    counts[0] = counts[1] = counts[2] = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    InflateRun infl(ctx, b);
    // (npore_bam_set_output_pass: the reader keeps what the run passes through; the setter has seen to it that the run writes FULL records)
    BamRecordWalker walker(b, n_regions, ref_id, start, stop, max_reads, threads, PASS_FLAGS, infl.hook(), b->out_rec.pass_mask);
    RunOutput out;
    if (int rco = out.open(b, out_path, threads)) return rco;
    int64_t n_bad = 0, ordinal0 = 0;
    auto on_status = [&](int64_t, int64_t m, const int32_t *st) {
        for (int64_t i = 0; i < m; i++)
            if (st[i] & ~NPORE_ST_PASSED) {       // (a record that passed is neither refused nor inconsistent)
                counts[(st[i] & NPORE_ST_BAD_INPUT) ? 1 : 2]++;
                if (n_bad < bad_cap) { bad_ord[n_bad] = ordinal0 + i; bad_status[n_bad] = st[i]; }
                n_bad++;
            }
        ordinal0 += m;
    };
    int rc = file_pipeline(ctx, b, fa, fasta_of_ref, AlignKnobs{indel_start, indel_extend, max_b_rows, r}, threads, out, true,
                           [&](int64_t, npore_batch_slot &s) { return walker.next_batch(s.rf, s.keep, batch_reads); }, on_status);
    counts[0] = ordinal0;
    return out.close(rc);
}
NPORE_CATCH_INT

int npore_bam_file_timing(const npore_bam *b, double *ms, int n)
{
    if (!b || !ms) return fail(NPORE_E_INVALID, "null argument");
    for (int k = 0; k < n; k++) ms[k] = k < 8 ? b->file_ms[k] : 0.0;
    return NPORE_OK;
}

int npore_bam_last_timing(const npore_bam *b, double *ms, int n)
{
    if (!b || !ms) return fail(NPORE_E_INVALID, "null argument");
    for (int k = 0; k < n; k++) ms[k] = k < 4 ? b->stage_ms[k] : 0.0;
    return NPORE_OK;
}

}  // extern "C"
