// npore_api.cpp -- C ABI (include/npore_amd.h) and host orchestration.
// Compiled with hipcc for gfx950 only.  There is no CPU execution path for the
// DP here: without a gfx950 device npore_ctx_create fails.  What reads BAM / FASTA
// files and writes SAM text needs no device and lives in bam_reader.hpp / hostio.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <future>
#include <limits>
#include <mutex>
#include <memory>
#include <numeric>
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

using namespace npore;

namespace {

// No C++ exception may cross the C ABI: the entry points that allocate are function-try-blocks ending in one of these.
#define NPORE_CATCH_INT                                                                             \
    catch (const std::bad_alloc &) { return fail(NPORE_E_NOMEM, "out of host memory"); }           \
    catch (const std::exception &e) { return fail(NPORE_E_INVALID, std::string("internal: ") + e.what()); }
#define NPORE_CATCH_PTR                                                                             \
    catch (const std::bad_alloc &) { fail(NPORE_E_NOMEM, "out of host memory"); return nullptr; }  \
    catch (const std::exception &e) { fail(NPORE_E_INVALID, std::string("internal: ") + e.what()); return nullptr; }
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(NPORE_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return NPORE_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        AllocTrace tr("hipMalloc", want);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(NPORE_E_NOMEM, "hipMalloc(" + std::to_string(want) + "): " + hipGetErrorString(e));
        }
        cap = want;
        return NPORE_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // best effort, no head-room: another buffer of the same role already has this capacity (presize_like)
    void match(const DevBuf &o)
    {
        if (o.cap <= cap) return;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        AllocTrace tr("hipMalloc like", o.cap);
        if (hipMalloc(&p, o.cap) == hipSuccess) cap = o.cap;
        else { p = nullptr; (void)hipGetLastError(); }
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct HostBuf {   // pinned staging
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return NPORE_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        AllocTrace tr("hipHostMalloc", want);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(NPORE_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        }
        cap = want;
        return NPORE_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Page-locked staging (hipHostMalloc) of the BAM -> SAM pipeline: the buffers of a batch that cross PCIe.  Unlike HostBuf
// it does not fail where the runtime has no page-locked memory left: the buffer is pageable from then on.
struct PinnedBuf {
    char *p = nullptr;
    size_t cap = 0;
    bool pinned = true;        // false once hipHostMalloc has failed: pageable (RawBuf::alloc) for the rest of its life
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    void release()
    {
        if (!p) return;
        if (pinned) (void)hipHostFree(p);
        else std::free(p);
        p = nullptr;
        cap = 0;
    }
    bool ensure(size_t n)
    {
        if (n <= cap) return true;
        release();
        n += n / 4;            // head-room: batches of a run differ a little in size
        if (pinned) {
            void *q = nullptr;
            AllocTrace tr("hipHostMalloc", n);
            if (hipHostMalloc(&q, n, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                pinned = false;
                if (std::getenv("NPORE_DEBUG")) std::fprintf(stderr, "npore: hipHostMalloc(%zu) failed, pageable staging buffer\n", n);
            }
            else p = static_cast<char *>(q);
        }
        if (!pinned) p = RawBuf::alloc(n);
        cap = p ? n : 0;
        return p != nullptr;
    }
};

}  // namespace

// One batch on its way through the BAM -> SAM pipeline: host staging (page-locked where it crosses PCIe) and offsets.
// The file pipeline's texts compacted on the device (unpack_kernels.hpp compact_texts_kernel): what a batch's align call needs
// to know about it
struct TextCompact {
    uint8_t *d_ctext;
    unsigned long long *d_cursor;
    int64_t cap;                 // bytes of d_ctext (all slots: it cannot overflow)
    int64_t *h_coff;             // [n_reads] page-locked
    char *h_ctext;               // page-locked
    int64_t h_bytes;             // how much of the compact buffer's front to send with the batch's last group
};

// The file pipeline's BAM mode with the records built on the device (bam_emit_kernels.hpp): what a batch's align call needs
// to know about it
struct BamEmit {
    uint8_t *d_recs;             // the batch's record buffer
    int64_t cap;
    unsigned long long *d_cursor;
    const int64_t *h_hp;         // [n_reads] page-locked: the reads' HP values
    int64_t *h_rec_len;          // [n_reads] page-locked: bytes of every read's record (0: not written)
    unsigned long long *h_total; // page-locked: bytes of the batch's records
};

struct npore_batch_slot {
    PinnedBuf refs, seqs, cigs, alns;
    RawBuf finals, sam;
    PinnedBuf raw;               // device pack: the heads of the batch's records (fixed fields ... 4-bit bases), one after the other
    std::vector<int64_t> rawo;   // ... and where each starts
    // device glue: the batch's texts compacted on the device (unpack_kernels.hpp compact_texts_kernel) -- the compact buffer
    // and its cursor there, the copied front of it and the reads' offsets here (page-locked)
    DevBuf d_ctext, d_cursor;
    PinnedBuf ctext_pin, coff_pin;
    // BAM mode, records built on the device: the batch's record buffer there (the cursor is d_cursor) and its upper bound,
    // the reads' HP values, and what comes back: the records' lengths, their total, the bytes
    DevBuf d_recs;
    int64_t rec_cap = 0;
    PinnedBuf hp_pin, reclen_pin, total_pin, recs_pin;
    int64_t ctext_copied = 0;              // bytes of the compact buffer the batch's last group sent behind its kernels
    PinnedBuf olen_pin, st_pin;            // lengths / status bits of an ASYNCHRONOUS batch land here (page-locked: a copy into
                                           // pageable memory would make the enqueueing call wait for the whole batch)
    hipEvent_t done = nullptr;             // ... behind which this event is recorded (npore_bam_realign_file)
    std::vector<std::shared_ptr<RawBuf>> keep;   // one-pass ingest: the inflated windows the batch's records lie in
    ~npore_batch_slot() { if (done) (void)hipEventDestroy(done); }
    RecFetch rf;                 // the batch's BAM records (streamed handles: inflated for the batch)
    double t_ms[6] = {0, 0, 0, 0, 0, 0};   // npore_bam_realign_file: fetch + pack, align call, standardise, format, write, (spare)
    std::vector<int64_t> ro, so, co, oo, fo, olen, flen;
    std::vector<BamRecMeta> meta;  // BAM output: what the index needs of every record written (sam then holds record bytes)
    int64_t sam_len = 0;
    int64_t m = 0;               // reads of the batch
    int rc = 0;
    std::string err;
};

// Work buffers of one group of reads on its way through the device stages (grow-only, reused).  A context has
// N_SETS of them: while the fill kernel works on one group, the next group is prepared in another set and the previous
// group's traceback / gather drains from a third (run_core).
struct WorkSet {
    DevBuf rd_i32, rd_i64, steps, inss, descs, sched, hist, counters; // path + chunks
    DevBuf tiles, cwoff;                                             // CIGAR tiles; chunk positions in the output
    DevBuf seqw, refw, refl, seql;                                   // annotation
    DevBuf tb, cout_, clen, cstat, cnruns;                           // fill / traceback (cout_: uint32 runs)
    DevBuf dbg;                                                      // experiments build: MAT.VAL per cell (NPORE_DBGMAT=1)
    HostBuf h_cnt;                                                   // counters read back with the group
    // host-buffer entry points: the group's slice of the caller's inputs / outputs on the device, its offset
    // arrays rebased to the slice (page-locked copy for the upload)
    DevBuf in_refs, in_seqs, in_cigs, in_off, out, out_len, status;
    DevBuf in_raw;               // device pack (unpack_kernels.hpp): the group's record heads
    DevBuf coff;                 // compacted texts: where each read of the group begins in the batch's compact buffer
    DevBuf in_hp, rec_off, rec_len;   // BAM records built on the device: the group's HP values, its records' places and sizes
    HostBuf h_off;
    hipEvent_t evc[4] = {};      // H2D start / end, D2H start / end of a staged group
    bool staged = false;
    hipEvent_t ev[6] = {};       // prep start / end, fill start / end, traceback + gather start / end (= group done)
    bool busy = false;           // enqueued, not collected yet
    // An idle set takes the capacities of one that has just been given a group: the groups of a run are alike, so its
    // own first group then finds its buffers in place instead of allocating tens of GB in front of its kernels (with
    // three sets that was the THIRD step of a run -- 0.4 s in a timed region that had two warm-up steps)
    void presize_like(const WorkSet &o)
    {
        DevBuf WorkSet::*const all[] = {&WorkSet::rd_i32, &WorkSet::rd_i64, &WorkSet::steps, &WorkSet::inss, &WorkSet::descs, &WorkSet::sched,
                                        &WorkSet::hist, &WorkSet::counters, &WorkSet::tiles, &WorkSet::cwoff, &WorkSet::seqw, &WorkSet::refw,
                                        &WorkSet::refl, &WorkSet::seql, &WorkSet::tb, &WorkSet::cout_, &WorkSet::clen, &WorkSet::cstat,
                                        &WorkSet::cnruns, &WorkSet::in_refs, &WorkSet::in_seqs, &WorkSet::in_cigs, &WorkSet::in_off,
                                        &WorkSet::out, &WorkSet::out_len, &WorkSet::status, &WorkSet::in_raw, &WorkSet::coff,
                                        &WorkSet::in_hp, &WorkSet::rec_off, &WorkSet::rec_len};
        for (auto m : all) (this->*m).match(o.*m);
    }
    int64_t cells = 0, call_id = 0;
    DevBuf *all[31] = {&rd_i32, &rd_i64, &steps, &inss, &descs, &sched, &hist, &counters, &tiles, &cwoff,
                       &seqw, &refw, &refl, &seql, &tb, &cout_, &clen, &cstat, &cnruns,
                       &in_refs, &in_seqs, &in_cigs, &in_off, &out, &out_len, &status, &in_raw, &coff, &in_hp, &rec_off, &rec_len};
};

// Work sets of a context: group k + 1 is prepared while group k is in the fill kernel and group k - 1 in its traceback;
// the third set lets the host enqueue group k + 1's preparation without waiting for group k - 1's traceback to end
// (with two, that wait sits between every pair of groups; measured equal within 1 % either way on this hardware --
// what binds the pipelined r = 30 case is the preparation's own duration beside a running fill kernel, LABNOTES.md).
constexpr int N_SETS = 3;

struct npore_ctx {
    int device = 0;
    int n_cus = 256;
    int max_n = 6, max_l = 100;
    // three non-blocking streams: preparation (also every copy), fill kernels, traceback + gather; events order
    // the stages of a group, the streams let stages of neighbouring groups run side by side
    hipStream_t stream = nullptr, s_fill[2] = {nullptr, nullptr}, s_post = nullptr;
    int next_fill = 0;           // the fill stream the next group's fill kernel goes to
    int fill_streams = 2;        // 1: every fill kernel on one stream (npore_ctx_set "fill_streams")
    hipEvent_t ev[8] = {};       // [4..7] H2D / D2H of the host-buffer entry point, [0] the caller's stream
    float *d_sub = nullptr, *d_np = nullptr;   // NULL in an annotation-only context (created without tables)
    WorkSet ws[N_SETS];
    int next_ws = 0;             // set the next group goes into (the oldest of them)
    WorkSet *last_ws = nullptr;  // set of the group enqueued last (npore_debug_fetch)
    int64_t call_id = 0, timing_call = -1;
    int deferred_rc = 0;         // failure found while collecting a group of an asynchronous call
    std::string deferred_err;
    double totals[8] = {};       // like timing[], summed over every group since the context was made
    // tunables
    int64_t tb_budget_mb = 0;   // 0 = auto
    int force_chunks = 0;
    int device_glue = 1;        // BAM -> SAM pipeline: realign_read's glue on the device (0: on the host, from the op strings)
    int coresident = 1;         // kernel shapes that fit beside a fill kernel for a group that overlaps another one's
    int device_pack = 1;        // BAM -> SAM pipeline with the glue on the device: align()'s inputs unpacked from the records on the device
    // device pack: the FASTA of the current run on the device (uploaded once per FASTA), the contig of every BAM reference
    DevBuf d_fasta, d_ctg;
    // recount of the confusion matrices from BAM records (npore_bam_confusion): the batch's record heads and their offsets,
    // the current contig's ranges, the counters
    DevBuf cms_raw, cms_off, cms_ranges, cms_counts;
    int64_t cms_batch_reads = 4000;
    uint64_t d_fasta_serial = 0;
    size_t d_fasta_bytes = 0;
    int n_ctg = 0;
    bool fill_has_room = false; // the last fill launch left LDS for such kernels on its CUs
    HostBuf h_offs;             // offset arrays of a device-resident batch (npore_align_batch_device)
    // device buffers (grow-only, reused across calls)
    DevBuf in_refs, in_seqs, in_cigs, in_off;                       // raw inputs (host-buffer entry point)
    std::vector<int32_t> regions;                                    // npore_np_regions: positions, then repeat counts
    DevBuf out, out_off, out_len, status;                            // outputs (host-buffer entry point)
    // host staging of the BAM -> SAM pipeline (npore_bam_realign_batch / _file): grow-only, reused across batches and files
    double file_mark[2] = {0, 0};      // totals at the start of npore_bam_realign_file (kernels, PCIe)
    static constexpr int N_SLOTS = 6;
    npore_batch_slot *slots[N_SLOTS] = {};
    // second context of the file pipeline (its own stream and work buffers), so that the transfers, preparation and
    // traceback of one batch run beside the fill kernel of its neighbour; made on first use from the host copy of the tables
    std::vector<float> h_sub, h_np;
    npore_ctx *peer = nullptr;
    double timing[8] = {};
};

namespace {

std::atomic<int> g_live_ctx[16];   // contexts alive per device (they share its memory: run_core's budget)

// waves per chunk: the smallest count whose 64 * nw lanes cover the band (the kernel relies on band
// column 2r lying in the last wave); 0 if the band is too wide
int pick_shape(int r)
{
    const int nw = (2 * r + 1 + 63) / 64;
    return nw <= MAX_WAVES_PER_CHUNK ? nw : 0;
}

int pow2_at_least(int x)
{
    int p = 64;
    while (p < x) p <<= 1;
    return p;
}

// Geometry of a fill launch for band half-width r: LDS sizes, chunks per workgroup and how many workgroups the
// GPU holds at a time.
struct FillGeom {
    int nw = 0, hw = 0, rwin = 0, cmax = 0;
};
bool fill_geometry(int r, FillGeom &g)
{
    g.nw = pick_shape(r);
    if (!g.nw) return false;
    g.hw = 2 * r + 1 + HIST_PAD;
    // reference-L window: the band (2r+1), 96 positions of read-ahead and the 6 positions below the band that the
    // generic SHR path looks back on -- plus 16 of margin, because the first wave of a chunk may run NW - 2
    // anti-diagonals behind the last one, which refills the window
    // (a chunk of ONE wave refills for itself, 32 positions at a time with 8 of slack: kernels.hpp WIN_STEP / WIN_SLACK;
    // r <= 31 then needs 2r + 6 + 8 + 32 <= 128 entries, which leaves the CU 16 KB of LDS at r = 30 -- room for the
    // kernels of the neighbouring batches beside 16 chunks)
    g.rwin = g.nw == 1 ? pow2_at_least(2 * r + 6 + 8 + 32) : pow2_at_least(2 * r + 101 + 16);
    const size_t lds_cap = 160 * 1024 / sizeof(float);
    if (fill_lds_floats(g.nw, 1, g.hw, g.rwin) > lds_cap) return false;
    g.cmax = 1;
    while ((g.cmax + 1) * g.nw * 64 <= 1024 && fill_lds_floats(g.nw, g.cmax + 1, g.hw, g.rwin) <= lds_cap) g.cmax++;
    return true;
}
// workgroups of `chunks` chunks that are resident together: the size of a persistent fill launch
int fill_round_workgroups(const FillGeom &g, int chunks, int n_cus)
{
    const size_t lds = fill_lds_floats(g.nw, chunks, g.hw, g.rwin) * sizeof(float);
    const int wg_per_cu = std::max(1, std::min((int)((160 * 1024) / std::max<size_t>(lds, 1)), 2048 / (64 * g.nw * chunks)));
    return std::max(1, n_cus) * wg_per_cu;
}

// NW waves per chunk, `chunks` chunks per workgroup (they share the LDS score table).
// leave_room: groups of reads overlap on the device (run_core), so the next group's preparation and this one's
// gather will look for room BESIDE fill workgroups: where the fill would take (nearly) all of a CU's LDS -- r = 30:
// 16 chunks = 159.75 KB -- a workgroup takes one chunk less (measured at r = 30, 8 000 reads per batch: 154 k
// instead of 144 k reads/s; the scans and the gather need ~3.5 KB of LDS).
// (NWT = 0: the instantiation that takes its wave count from the launch -- bands of 9 ... 16 waves, one chunk per workgroup)
template <int NWT>
hipError_t launch_fill(KParams kp, int max_chunks, int force_chunks, int n_cus, hipStream_t s, bool leave_room, bool *has_room)
{
    constexpr int MAXT = 1024;
    FillGeom g;
    if (!fill_geometry(kp.r, g) || (NWT ? g.nw != NWT : g.nw <= 8)) return hipErrorInvalidValue;
    const int NW = g.nw;
    kp.hw = g.hw;
    kp.rwin = g.rwin;
    const int cmax = g.cmax;
    // few chunks: spread them over the CUs; many: pack workgroups so that the table is amortised
    int chunks = std::min(cmax, std::max(1, (max_chunks + 255) / 256));
    if (leave_room && chunks > 1 && fill_lds_floats(NW, chunks, kp.hw, kp.rwin) * sizeof(float) + 4096 > 160 * 1024) {
        // ... unless exactly that chunk per workgroup decides whether the batch's full-size chunks (about half of
        // the upper bound: a read's last chunk is a short tail) are resident all at once (r = 30, 4 000 reads per
        // batch: 142 k reads/s with 16 chunks per workgroup, 127 k with 15)
        const int64_t big = (max_chunks + 1) / 2, wgs = fill_round_workgroups(g, chunks, n_cus);
        if (!(big <= wgs * chunks && big > wgs * (chunks - 1))) chunks--;
    }
    if (force_chunks > 0) chunks = std::min(cmax, force_chunks);
    const size_t lds = fill_lds_floats(NW, chunks, kp.hw, kp.rwin) * sizeof(float);
    *has_room = lds + 4096 <= 160 * 1024;      // other kernels' light workgroups fit beside this launch's
    // the kernel addresses its score tables by absolute LDS address (kernels.hpp: lds_abs_f32): it must not
    // own any static LDS, so that the dynamic array starts at address 0
    static const hipError_t no_static_lds = [] {
        hipFuncAttributes at;
        const hipError_t e0 = hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&fill_kernel<NWT, MAXT>));
        return e0 != hipSuccess ? e0 : (at.sharedSizeBytes == 0 ? hipSuccess : hipErrorInvalidDeviceFunction);
    }();
    if (no_static_lds != hipSuccess) return no_static_lds;
    // A persistent launch: as many workgroups as the GPU keeps resident (or fewer, if the batch is small); their
    // groups of NW waves pull the chunks of the schedule (largest first) from a device-side queue (kernels.hpp)
    const int resident = fill_round_workgroups(g, chunks, n_cus);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&fill_kernel<NWT, MAXT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((fill_kernel<NWT, MAXT>), dim3(std::min((max_chunks + chunks - 1) / chunks, resident)),
                       dim3(64 * NW * chunks), lds, s, kp);
    return hipGetLastError();
}

struct OutTarget {
    uint8_t *d_out;
    const int64_t *d_out_off;
    int64_t *d_out_len;
    int32_t *d_status;
};

// device pointers to the raw batch + host copies of the three offset arrays
struct AlignArgs {
    int64_t n_reads;
    const uint8_t *d_refs;
    const int64_t *d_ref_off;
    const uint8_t *d_seqs;
    const int64_t *d_seq_off;
    const char *d_cigs;
    const int64_t *d_cig_off;
    const int64_t *h_ref_off, *h_seq_off, *h_cig_off;
    float indel_start, indel_extend;
    int max_b_rows, r;
    // host-buffer entry points (d_* above are NULL then): every group uploads its slice of these, and downloads
    // its slice of the results, around its own kernels -- the copies of one group overlap the kernels of its neighbours
    const uint8_t *h_refs = nullptr, *h_seqs = nullptr;
    const char *h_cigs = nullptr;
    char *h_out = nullptr;
    const int64_t *h_out_off = nullptr;
    int64_t *h_out_len = nullptr;
    int32_t *h_status = nullptr;
    // the output is the collapsed, standardised CIGAR text (realign_read's glue on the device, kernels.hpp
    // standardize_kernel) instead of the op string; out_len = bytes of text
    bool final_text = false;
    // device pack: instead of h_refs / h_seqs / h_cigs the heads of the BAM records; every group uploads its slice and
    // unpacks it on the device (unpack_kernels.hpp)
    const uint8_t *h_raw = nullptr;
    const int64_t *h_raw_off = nullptr;
    const CtgEntry *d_ctg = nullptr;
    int n_ctg = 0;
    // the file pipeline with the device glue: the texts compacted on the device, the used front of the compact buffer and
    // the reads' offsets copied instead of the slots (nullptr: the slots, as the public entry points promise)
    const TextCompact *compact = nullptr;
    // BAM mode of the file pipeline (device pack + device glue): the final CIGARs stay on the device as words and the
    // records are assembled there; neither the slots nor a compact buffer are copied
    const BamEmit *bam = nullptr;
    bool staged() const { return h_out != nullptr; }
};


int64_t chunk_bound(int64_t cig_len, int max_b_rows)
{
    const int64_t cm1 = max_b_rows - 1;
    return std::max<int64_t>(1, (2 * cig_len + cm1 - 1) / cm1);
}

// Reads [g0,g1): everything from the raw bytes to the gathered output, on stream s,
// without host synchronisation.
int run_group(npore_ctx *ctx, WorkSet *w, const AlignArgs &a, int64_t g0, int64_t g1, const OutTarget &ot, int shape,
              bool overlapping)
{
    // overlapping: another group of this context is on the device.  beside_fill: ... and the fill launch it belongs to
    // left room on its CUs (launch_fill), so kernels of light shapes can run beside it.
    const bool beside_fill = overlapping && ctx->fill_has_room;
    // beside_fill: another group of this context is on the device, most likely in its fill kernel, whose persistent
    // workgroups hold nearly all the LDS and most of the vector registers of every CU until they have emptied their
    // queue.  The preparation and gather kernels of THIS group then run in shapes that find room beside a fill
    // workgroup instead of waiting for it to leave: 256-thread scans (one wave per SIMD), the LDS-free annotation
    // (prep_kernels.hpp) and the gather without its LDS tile (kernels.hpp).
    const unsigned scan_threads = beside_fill ? 256 : 1024;
    hipStream_t s = ctx->stream;      // preparation; the fill and traceback stages go to their own streams below
    const int64_t nr = g1 - g0;
    const int r = a.r;
    const int tbs = tb_stride(r);
    const int64_t cig_bytes = a.h_cig_off[g1] - a.h_cig_off[g0];
    const int64_t S_tot = a.h_seq_off[g1] - a.h_seq_off[g0], R_tot = a.h_ref_off[g1] - a.h_ref_off[g0];
    // longest chunk slice of the group: a slice never exceeds its sequence, nor max_b_rows + 1 bases
    int64_t max_len = 0;
    for (int64_t i = g0; i < g1; i++)
        max_len = std::max({max_len, a.h_seq_off[i + 1] - a.h_seq_off[i], a.h_ref_off[i + 1] - a.h_ref_off[i]});
    int64_t max_chunks = 0;
    for (int64_t k = g0; k < g1; k++) max_chunks += chunk_bound(a.h_cig_off[k + 1] - a.h_cig_off[k], a.max_b_rows);
    if (max_chunks > (1ll << 30)) return fail(NPORE_E_UNSUPPORTED, "too many chunks in one group");
    const int64_t steps_cap = 2 * cig_bytes + 512;
    const int64_t tb_words = (2 * cig_bytes + max_chunks) * tbs;

    // CIGAR tiles (prep_kernels.hpp): every read has at least one
    int64_t max_tiles = 0;
    for (int64_t k = g0; k < g1; k++)
        max_tiles += std::max<int64_t>(1, (a.h_cig_off[k + 1] - a.h_cig_off[k] + CIGAR_TILE - 1) / CIGAR_TILE);
    if (max_tiles > (1ll << 30)) return fail(NPORE_E_UNSUPPORTED, "too many CIGAR tiles in one group");
    if (int rc = w->rd_i32.ensure((size_t)(5 * nr + 16) * 4)) return rc;
    if (int rc = w->tiles.ensure((size_t)max_tiles * 24 + 64)) return rc;
    if (int rc = w->cwoff.ensure((size_t)max_chunks * 8 + 64)) return rc;
    if (int rc = w->rd_i64.ensure((size_t)(nr + 2) * 8)) return rc;
    if (int rc = w->steps.ensure(steps_cap)) return rc;
    if (int rc = w->inss.ensure((size_t)(2 * cig_bytes + nr + 16) * 4)) return rc;
    if (int rc = w->descs.ensure((size_t)max_chunks * sizeof(ChunkDesc))) return rc;
    if (int rc = w->sched.ensure((size_t)max_chunks * 4)) return rc;
    if (int rc = w->hist.ensure((size_t)(a.max_b_rows + 2) * 4)) return rc;
    if (int rc = w->counters.ensure(64)) return rc;
    if (int rc = w->seqw.ensure((size_t)(S_tot + max_chunks + 16) * 4)) return rc;
    if (int rc = w->refw.ensure((size_t)(R_tot + max_chunks + 16) * 16)) return rc;
    if (int rc = w->refl.ensure((size_t)(R_tot + max_chunks + 16) * 8)) return rc;
    if (int rc = w->tb.ensure((size_t)tb_words * 4 + 64)) return rc;
#if defined(NPORE_EXPERIMENTS)
    if (std::getenv("NPORE_DBGMAT") && w->dbg.p) (void)hipMemsetAsync(w->dbg.p, 0, w->dbg.cap, ctx->stream);     // (steps of the compiled path leave zeros)
    if (std::getenv("NPORE_DBGMAT")) { if (int rc = w->dbg.ensure((size_t)tb_words * 4 * (size_t)std::max(1, std::atoi(std::getenv("NPORE_DBGMAT"))) + 64)) return rc; }
#endif
    if (int rc = w->cout_.ensure(((size_t)(S_tot + R_tot) + 64) * 4)) return rc;
    if (int rc = w->cnruns.ensure((size_t)max_chunks * 4 + 64)) return rc;
    if (int rc = w->clen.ensure((size_t)max_chunks * 4 + 64)) return rc;
    if (int rc = w->cstat.ensure((size_t)max_chunks * 4 + 64)) return rc;

    PrepParams pp;
    pp.n_reads = nr;
    pp.refs = a.d_refs; pp.ref_off = a.d_ref_off + g0;
    pp.seqs = a.d_seqs; pp.seq_off = a.d_seq_off + g0;
    pp.cigs = a.d_cigs; pp.cig_off = a.d_cig_off + g0;
    OutTarget got = ot;                  // where the gather writes, and the index of this group's first read in it
    int64_t out_read_base = g0;
    w->staged = a.staged();
    if (a.staged()) {
        // upload the group's slice: bases + CIGAR ops as they lie, the four offset arrays rebased to the slice
        const int64_t out_bytes = a.h_out_off[g1] - a.h_out_off[g0];
        if (int rc = w->h_off.ensure((size_t)5 * (nr + 1) * 8)) return rc;
        if (int rc = w->in_refs.ensure((size_t)R_tot + 64)) return rc;
        if (int rc = w->in_seqs.ensure((size_t)S_tot + 64)) return rc;
        if (int rc = w->in_cigs.ensure((size_t)cig_bytes + 64)) return rc;
        if (int rc = w->in_off.ensure((size_t)5 * (nr + 1) * 8)) return rc;
        if (int rc = w->out.ensure((size_t)out_bytes + 64)) return rc;
        if (int rc = w->out_len.ensure((size_t)nr * 8)) return rc;
        if (int rc = w->status.ensure((size_t)nr * 4)) return rc;
        int64_t *ho = w->h_off.as<int64_t>(), *hro = ho, *hso = ho + (nr + 1), *hco = ho + 2 * (nr + 1), *hoo = ho + 3 * (nr + 1);
        for (int64_t i = 0; i <= nr; i++) {
            hro[i] = a.h_ref_off[g0 + i] - a.h_ref_off[g0]; hso[i] = a.h_seq_off[g0 + i] - a.h_seq_off[g0];
            hco[i] = a.h_cig_off[g0 + i] - a.h_cig_off[g0]; hoo[i] = a.h_out_off[g0 + i] - a.h_out_off[g0];
        }
        const int64_t raw_bytes = a.h_raw ? a.h_raw_off[g1] - a.h_raw_off[g0] : 0;
        if (a.h_raw) {
            int64_t *hwo = ho + 4 * (nr + 1);
            for (int64_t i = 0; i <= nr; i++) hwo[i] = a.h_raw_off[g0 + i] - a.h_raw_off[g0];
            if (int rc = w->in_raw.ensure((size_t)raw_bytes + 64)) return rc;
        }
        HIP_TRY(hipEventRecord(w->evc[0], s));
        if (a.h_raw) {
            HIP_TRY(hipMemcpyAsync(w->in_raw.p, a.h_raw + a.h_raw_off[g0], (size_t)raw_bytes, hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync(w->in_refs.p, a.h_refs + a.h_ref_off[g0], (size_t)R_tot, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(w->in_seqs.p, a.h_seqs + a.h_seq_off[g0], (size_t)S_tot, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(w->in_cigs.p, a.h_cigs + a.h_cig_off[g0], (size_t)cig_bytes, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipMemcpyAsync(w->in_off.p, ho, (size_t)5 * (nr + 1) * 8, hipMemcpyHostToDevice, s));
        if (a.bam) {
            if (int rc = w->in_hp.ensure((size_t)nr * 8 + 64)) return rc;
            HIP_TRY(hipMemcpyAsync(w->in_hp.p, a.bam->h_hp + g0, (size_t)nr * 8, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipEventRecord(w->evc[1], s));
        const int64_t *d_off = w->in_off.as<int64_t>();
        if (a.h_raw) {          // align()'s three inputs from the record heads (unpack_kernels.hpp), where the copies above would have put them
            UnpackParams up;
            up.raw = w->in_raw.as<uint8_t>(); up.raw_off = d_off + 4 * (nr + 1);
            up.ctg = a.d_ctg; up.n_ctg = a.n_ctg;
            up.refs = w->in_refs.as<uint8_t>(); up.ref_off = d_off;
            up.seqs = w->in_seqs.as<uint8_t>(); up.seq_off = d_off + (nr + 1);
            up.cigs = w->in_cigs.as<char>(); up.cig_off = d_off + 2 * (nr + 1);
            up.n_reads = nr;
            hipLaunchKernelGGL(unpack_records_kernel, dim3((unsigned)nr), dim3(256), 0, s, up);
            HIP_TRY(hipGetLastError());
        }
        pp.refs = w->in_refs.as<uint8_t>(); pp.ref_off = d_off;
        pp.seqs = w->in_seqs.as<uint8_t>(); pp.seq_off = d_off + (nr + 1);
        pp.cigs = w->in_cigs.as<char>(); pp.cig_off = d_off + 2 * (nr + 1);
        got = OutTarget{w->out.as<uint8_t>(), d_off + 3 * (nr + 1), w->out_len.as<int64_t>(), w->status.as<int32_t>()};
        out_read_base = 0;
    }
    pp.max_b_rows = a.max_b_rows; pp.r = r; pp.tbstride = tbs; pp.max_n = ctx->max_n; pp.max_l = ctx->max_l;
    pp.max_chunks = (int)max_chunks;
    int32_t *i32 = w->rd_i32.as<int32_t>();
    pp.rd_nsteps = i32;
    pp.rd_nchunks = i32 + nr;
    pp.rd_status = i32 + 2 * nr;
    pp.rd_chunk_first = i32 + 3 * nr;   // nr + 1 entries
    pp.rd_tile_first = i32 + 4 * nr + 4;   // nr + 1 entries
    pp.tile_cnt = w->tiles.as<int4>();
    pp.tile_base = reinterpret_cast<int2 *>(w->tiles.as<char>() + (size_t)max_tiles * 16);
    pp.rd_steps_off = w->rd_i64.as<int64_t>();
    pp.steps = w->steps.as<uint8_t>();
    pp.inss = w->inss.as<int32_t>();
    pp.descs = w->descs.as<ChunkDesc>();
    pp.sched = w->sched.as<int32_t>();
    pp.hist = w->hist.as<int32_t>();
    pp.counters = w->counters.as<int32_t>();
    pp.seqw = w->seqw.as<uint32_t>();
    pp.refw = w->refw.as<uint4>();
    pp.refl = w->refl.as<uint2>();

    if (int rc = w->h_cnt.ensure(64)) return rc;
    HIP_TRY(hipEventRecord(w->ev[0], s));
    HIP_TRY(hipMemsetAsync(pp.hist, 0, (size_t)(a.max_b_rows + 2) * 4, s));
    const unsigned rd_blocks = (unsigned)((nr + 3) / 4), ch_blocks = (unsigned)((max_chunks + 255) / 256);
    const unsigned tile_blocks = (unsigned)((max_tiles + 3) / 4);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(scan_threads), 0, s, pp);
    hipLaunchKernelGGL(cigar_tile_kernel, dim3(tile_blocks), dim3(256), 0, s, pp);
    hipLaunchKernelGGL(cigar_scan_kernel, dim3(rd_blocks), dim3(256), 0, s, pp);
    hipLaunchKernelGGL(read_scan_kernel, dim3(1), dim3(scan_threads), 0, s, pp);
    hipLaunchKernelGGL(expand_path_kernel, dim3(tile_blocks), dim3(256), 0, s, pp);
    hipLaunchKernelGGL(make_chunks_kernel, dim3(ch_blocks), dim3(256), 0, s, pp);
    hipLaunchKernelGGL(chunk_scan_kernel, dim3(1), dim3(scan_threads), 0, s, pp);
    hipLaunchKernelGGL(sched_scatter_kernel, dim3(ch_blocks), dim3(256), 0, s, pp);
    // n-polymer annotation + word packing: one wave per (chunk, sequence), registers only (annot_wave.hpp) -- the same
    // launch whether the GPU is empty or a fill kernel holds the CUs' LDS
    if (ctx->max_n == MAX_PERIOD) hipLaunchKernelGGL(annotate_wave_kernel<true>, dim3((unsigned)(2 * max_chunks)), dim3(64), 0, s, pp);
    else hipLaunchKernelGGL(annotate_wave_kernel<false>, dim3((unsigned)(2 * max_chunks)), dim3(64), 0, s, pp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w->ev[1], s));
    // ---- fill: behind this group's preparation.  Consecutive groups alternate between two streams: their fill
    // kernels share nothing, so the next one's persistent workgroups move onto the CUs that this one's leave as its
    // last chunks run out -- the tail of one launch is filled by the head of the next (C2, steps back to back:
    // 17.1 ms per step against the 18.0 ms one fill kernel takes alone; one stream: 18.1)
    s = ctx->s_fill[ctx->next_fill];
    if (ctx->fill_streams == 2) ctx->next_fill ^= 1;
    HIP_TRY(hipStreamWaitEvent(s, w->ev[1], 0));
    HIP_TRY(hipEventRecord(w->ev[2], s));

    KParams kp;
    kp.descs = pp.descs;
    kp.sched = pp.sched;
    kp.n_chunks = pp.counters;
    kp.queue = pp.counters + 2;
    kp.steps = pp.steps;
    kp.inss = pp.inss;
    kp.seqw = pp.seqw;
    kp.refw = pp.refw;
    kp.refl = pp.refl;
    kp.tb = w->tb.as<uint32_t>();
    kp.dbg = w->dbg.as<uint32_t>();
    kp.sub_scores = ctx->d_sub;
    kp.np_scores = ctx->d_np;
    kp.max_n = ctx->max_n;
    kp.max_l = ctx->max_l;
    kp.r = r;
    kp.tbstride = tbs;
    kp.indel_start = a.indel_start;
    kp.indel_extend = a.indel_extend;
    hipError_t e = hipSuccess;
    const int mc = (int)max_chunks;
    switch (shape) {
        case 1: e = launch_fill<1>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        case 2: e = launch_fill<2>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        case 3: e = launch_fill<3>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        case 4: e = launch_fill<4>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        case 5: e = launch_fill<5>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        case 6: e = launch_fill<6>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        case 7: e = launch_fill<7>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        case 8: e = launch_fill<8>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        case 9: case 10: case 11: case 12: case 13: case 14: case 15: case 16:
            e = launch_fill<0>(kp, mc, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room); break;
        default: return fail(NPORE_E_UNSUPPORTED, "unsupported waves-per-chunk count");
    }
    if (e != hipSuccess) return fail(NPORE_E_HIP, std::string("fill launch: ") + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(w->ev[3], s));
    // ---- traceback + gather: behind this group's fill, beside the next group's
    s = ctx->s_post;
    HIP_TRY(hipStreamWaitEvent(s, w->ev[3], 0));
    HIP_TRY(hipEventRecord(w->ev[4], s));

    TParams tp;
    tp.descs = pp.descs;
    tp.n_chunks = pp.counters;
    tp.tb = kp.tb;
    tp.inss = pp.inss;
    tp.chunk_runs = w->cout_.as<uint32_t>();
    tp.chunk_nruns = w->cnruns.as<int32_t>();
    tp.chunk_len = w->clen.as<int32_t>();
    tp.chunk_status = w->cstat.as<int32_t>();
    tp.r = r;
    tp.tbstride = tbs;
    // (10 kb reads: 0.53 ms at 500 chunk slots, 0.83 ms at 8 000)
    hipLaunchKernelGGL(traceback_rows_kernel, dim3((unsigned)max_chunks), dim3(64), 0, s, tp);
    HIP_TRY(hipGetLastError());

    GParams gp;
    gp.descs = pp.descs;
    gp.read_first_chunk = pp.rd_chunk_first;
    gp.chunk_runs = tp.chunk_runs;
    gp.chunk_nruns = tp.chunk_nruns;
    gp.chunk_len = tp.chunk_len;
    gp.chunk_status = tp.chunk_status;
    gp.read_status_in = pp.rd_status;
    gp.counters = pp.counters;
    gp.seqs = pp.seqs;
    gp.refs = pp.refs;
    gp.out = got.d_out;
    gp.out_off = got.d_out_off;
    gp.out_len = got.d_out_len;
    gp.status = got.d_status;
    gp.read_base = out_read_base;
    gp.n_reads = nr;
    gp.chunk_woff = w->cwoff.as<int64_t>();
    hipLaunchKernelGGL(gather_scan_kernel, dim3(rd_blocks), dim3(256), 0, s, gp);
    if (a.final_text) {
        StdKParams sp;
        sp.descs = pp.descs;
        sp.read_first_chunk = pp.rd_chunk_first;
        sp.chunk_runs = tp.chunk_runs;
        sp.chunk_nruns = tp.chunk_nruns;
        sp.refs = pp.refs; sp.ref_off = pp.ref_off;
        sp.seqs = pp.seqs; sp.seq_off = pp.seq_off;
        sp.out = got.d_out;
        sp.out_off = got.d_out_off;
        sp.out_len = got.d_out_len;
        sp.status = got.d_status;
        sp.read_base = out_read_base;
        sp.n_reads = nr;
        if (a.bam) hipLaunchKernelGGL(standardize_words_kernel, dim3((unsigned)nr), dim3(64), 0, s, sp);
        else hipLaunchKernelGGL(standardize_kernel, dim3((unsigned)nr), dim3(64), 0, s, sp);      // one wavefront per read
        if (a.bam) {            // the group's records behind those of the groups before it (bam_emit_kernels.hpp)
            if (!a.h_raw || !a.staged()) return fail(NPORE_E_INVALID, "internal: BAM records on the device need the device pack");
            if (int rc = w->rec_off.ensure((size_t)nr * 8 + 64)) return rc;
            if (int rc = w->rec_len.ensure((size_t)nr * 8 + 64)) return rc;
            if (g0 == 0) HIP_TRY(hipMemsetAsync(a.bam->d_cursor, 0, 8, s));
            const int64_t *d_off = w->in_off.as<int64_t>();
            BamEmitParams bp;
            bp.raw = w->in_raw.as<uint8_t>(); bp.raw_off = d_off + 4 * (nr + 1);
            bp.ref_off = d_off; bp.seq_off = d_off + (nr + 1);
            bp.hp = w->in_hp.as<int64_t>();
            bp.words = got.d_out; bp.words_off = got.d_out_off; bp.words_len = got.d_out_len; bp.status = got.d_status;
            bp.read_base = out_read_base; bp.n_reads = nr;
            bp.recs = a.bam->d_recs; bp.cap = a.bam->cap; bp.cursor = a.bam->d_cursor;
            bp.rec_off = w->rec_off.as<int64_t>(); bp.rec_len = w->rec_len.as<int64_t>();
            hipLaunchKernelGGL(place_bam_records_kernel, dim3(1), dim3(256), 0, s, bp);
            hipLaunchKernelGGL(emit_bam_records_kernel, dim3((unsigned)nr), dim3(64), 0, s, bp);
        } else if (a.compact) {        // the texts to the front of the batch's compact buffer (unpack_kernels.hpp)
            if (int rc = w->coff.ensure((size_t)nr * 8 + 64)) return rc;
            if (g0 == 0) HIP_TRY(hipMemsetAsync(a.compact->d_cursor, 0, 8, s));
            CompactParams cp;
            cp.out = got.d_out;
            cp.out_off = got.d_out_off;
            cp.out_len = got.d_out_len;
            cp.read_base = out_read_base;
            cp.n_reads = nr;
            cp.ctext = a.compact->d_ctext;
            cp.cursor = a.compact->d_cursor;
            cp.coff = w->coff.as<int64_t>();
            cp.cap = a.compact->cap;
            hipLaunchKernelGGL(compact_texts_kernel, dim3((unsigned)nr), dim3(64), 0, s, cp);
        }
    } else
    // LDS of gather_kernel: one tile of ops + (when a chunk's two base slices fit beside it) the slices
    {
        const int64_t rows_max = std::min<int64_t>(max_len, a.max_b_rows) + 1;    // longest slice of any chunk
        if (beside_fill) {
            gp.slice_cap = 0;
            hipLaunchKernelGGL(gather_kernel<false>, dim3((unsigned)max_chunks), dim3(256), 0, s, gp);
        } else {
            gp.slice_cap = rows_max <= 24 * 1024 ? (int)((rows_max + 15) & ~(int64_t)15) : 0;
            const size_t glds = (size_t)GATHER_TILE + 2 * (size_t)gp.slice_cap;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&gather_kernel<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)glds));
            hipLaunchKernelGGL(gather_kernel<true>, dim3((unsigned)max_chunks), dim3(256), glds, s, gp);
        }
    }
    HIP_TRY(hipGetLastError());
    if (a.staged()) {                   // download the group's slice of the results behind its gather
        HIP_TRY(hipEventRecord(w->evc[2], s));
        if (a.final_text && a.bam) {
            HIP_TRY(hipMemcpyAsync(a.bam->h_rec_len + g0, w->rec_len.p, (size_t)nr * 8, hipMemcpyDeviceToHost, s));
            if (g1 == a.n_reads) HIP_TRY(hipMemcpyAsync(a.bam->h_total, a.bam->d_cursor, 8, hipMemcpyDeviceToHost, s));
        } else if (a.final_text && a.compact) {
            HIP_TRY(hipMemcpyAsync(a.compact->h_coff + g0, w->coff.p, (size_t)nr * 8, hipMemcpyDeviceToHost, s));
            if (g1 == a.n_reads && a.compact->h_bytes > 0)       // the batch's last group: the front of the compact buffer
                HIP_TRY(hipMemcpyAsync(a.compact->h_ctext, a.compact->d_ctext, (size_t)a.compact->h_bytes, hipMemcpyDeviceToHost, s));
        } else {
            HIP_TRY(hipMemcpyAsync(a.h_out + a.h_out_off[g0], w->out.p, (size_t)(a.h_out_off[g1] - a.h_out_off[g0]), hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipMemcpyAsync(a.h_out_len + g0, w->out_len.p, (size_t)nr * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(a.h_status + g0, w->status.p, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(w->evc[3], s));
    }
    HIP_TRY(hipMemcpyAsync(w->h_cnt.p, w->counters.p, 8, hipMemcpyDeviceToHost, s));    // chunk count, overflow flag
    HIP_TRY(hipEventRecord(w->ev[5], s));
    return NPORE_OK;
}

// Wait for a group that was enqueued into `w`, add its stage times to the context's timing and check its counters.
int collect_group(npore_ctx *ctx, WorkSet *w)
{
    if (!w->busy) return NPORE_OK;
    w->busy = false;
    HIP_TRY(hipEventSynchronize(w->ev[5]));
    if (w->call_id != ctx->timing_call) {       // first group of a newer call: npore_last_timing starts over
        std::fill(ctx->timing, ctx->timing + 8, 0.0);
        ctx->timing_call = w->call_id;
    }
    float ms = 0;
    for (int k = 0; k < 3; k++) {
        HIP_TRY(hipEventElapsedTime(&ms, w->ev[2 * k], w->ev[2 * k + 1]));
        ctx->timing[k] += ms;
        ctx->totals[k] += ms;
    }
    if (w->staged)
        for (int k = 0; k < 2; k++) {
            HIP_TRY(hipEventElapsedTime(&ms, w->evc[2 * k], w->evc[2 * k + 1]));
            ctx->timing[3 + k] += ms;
            ctx->totals[3 + k] += ms;
        }
    ctx->timing[6] += (double)w->cells; ctx->totals[6] += (double)w->cells;
    ctx->timing[7] += 1; ctx->totals[7] += 1;
    if (w->h_cnt.as<int32_t>()[1]) return fail(NPORE_E_HIP, "internal: chunk bound exceeded");
    return NPORE_OK;
}

// Everything this context has in flight (asynchronous calls): collected oldest first.  Returns the first failure,
// including one found earlier while a work set was being recycled.
int quiesce(npore_ctx *ctx)
{
    int rc = ctx->deferred_rc;
    std::string err = ctx->deferred_err;
    for (int k = 0; k < N_SETS; k++) {
        WorkSet *w = &ctx->ws[(ctx->next_ws + k) % N_SETS];
        const int r2 = collect_group(ctx, w);
        if (r2 && !rc) { rc = r2; err = g_err; }
    }
    ctx->deferred_rc = 0;
    ctx->deferred_err.clear();
    return rc ? fail(rc, err) : NPORE_OK;
}

// The batch, group by group, through the three-stage pipeline: the groups rotate through the N_SETS work sets, so
// that group k+1 is prepared and group k-1 traced back while the fill kernel works on group k.  `user` (may be
// NULL) is the caller's stream: the batch is ordered behind what it holds now.  sync = false returns once the
// last group is enqueued (results complete when npore_ctx_wait returns, or for work put on `user` afterwards).
int run_core(npore_ctx *ctx, const AlignArgs &a, const OutTarget &ot, hipStream_t user, bool sync)
{
    if (a.n_reads < 0) return fail(NPORE_E_INVALID, "n_reads < 0");
    if (!ctx->d_sub || !ctx->d_np) return fail(NPORE_E_INVALID, "this context was created without penalty tables (annotation only)");
    if (a.r < 1) return fail(NPORE_E_INVALID, "r must be >= 1");
    if (!std::isfinite(a.indel_start) || !std::isfinite(a.indel_extend))
        return fail(NPORE_E_INVALID, "indel_start and indel_extend must be finite");
    if (a.max_b_rows < 2) return fail(NPORE_E_INVALID, "max_b_rows must be >= 2");
    if (a.max_b_rows > 60000)
        return fail(NPORE_E_UNSUPPORTED, "max_b_rows > 60000: run lengths are kept in 16 bits");
    const int shape = pick_shape(a.r);
    if (!shape) return fail(NPORE_E_UNSUPPORTED, "band half-width r > 511");
    if (a.n_reads == 0) return NPORE_OK;
    ctx->call_id++;
    if (user) {
        HIP_TRY(hipEventRecord(ctx->ev[0], user));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev[0], 0));
    }

    // groups of consecutive reads whose traceback words fit the budget.  The automatic budget is this context's
    // share of the device (contexts of one device run side by side: the file pipeline's peer, bench --inflight),
    // divided by its N_SETS work sets: 60 % of the memory divided by the live contexts, and never more than what is
    // free now plus what the context already holds.
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int live = std::max(1, g_live_ctx[ctx->device & 15].load());
    size_t held = 0;
    for (const auto &w0 : ctx->ws) held += w0.tb.cap;
    const int64_t budget = ctx->tb_budget_mb > 0
                               ? ctx->tb_budget_mb * (int64_t)1048576
                               : (int64_t)(std::min(0.6 * (double)total_b / live, 0.9 * (double)(free_b + held)) / N_SETS);
    const int tbs = tb_stride(a.r);
    int64_t g0 = 0;
    int64_t max_group = a.n_reads;       // halved when a group's buffers do not fit after all
    WorkSet *last = nullptr;
    while (g0 < a.n_reads) {
        int64_t g1 = g0, acc = 0, cells = 0;
        while (g1 < a.n_reads && g1 - g0 < max_group) {
            const int64_t cl = a.h_cig_off[g1 + 1] - a.h_cig_off[g1];
            // traceback words + the per-step / per-base side arrays (steps, inss, refw, refl, seqw, runs: < 48 B per op)
            const int64_t need = (2 * cl + chunk_bound(cl, a.max_b_rows)) * tbs * 4 + 48 * cl;
            if (g1 > g0 && acc + need > budget) break;
            acc += need;
            g1++;
        }
        // a group that is not the last one holds a whole number of launch-fulls of full-size chunks (about one per
        // read): its fill kernel then ends on full chains instead of a sparse tail
        if (g1 < a.n_reads) {
            FillGeom fg;
            if (fill_geometry(a.r, fg)) {
                const int64_t full = (int64_t)fill_round_workgroups(fg, fg.cmax, ctx->n_cus) * fg.cmax;
                if (g1 - g0 > full) g1 = g0 + (g1 - g0) / full * full;
            }
        }
        cells = (a.h_seq_off[g1] - a.h_seq_off[g0] + a.h_ref_off[g1] - a.h_ref_off[g0] + (g1 - g0)) * (2 * a.r + 1);
        WorkSet *w = &ctx->ws[ctx->next_ws];
        if (int rc = collect_group(ctx, w)) {        // the set's previous group (N_SETS groups back) has to be through
            if (!ctx->deferred_rc) { ctx->deferred_rc = rc; ctx->deferred_err = g_err; }
        }
        // (the other work set still busy: its group is in the fill or traceback stage while this one is prepared,
        // and this group's gather will most likely run while the next one's fill is on the GPU)
        bool beside = false;
        for (int k = 1; k < N_SETS; k++) beside |= ctx->coresident && ctx->ws[(ctx->next_ws + k) % N_SETS].busy;
        if (int rc = run_group(ctx, w, a, g0, g1, ot, shape, beside)) {
            // drain what is in flight; a failure found there (an earlier group of this call, or of a previous
            // sync = 0 call) is the older one and must not be lost: it stays deferred / is what the call returns
            const std::string this_err = g_err;
            const int older = quiesce(ctx);
            if (rc == NPORE_E_NOMEM && g1 - g0 > 1) {          // another context got there first: smaller groups
                if (older) { ctx->deferred_rc = older; ctx->deferred_err = g_err; }
                max_group = (g1 - g0) / 2;
                continue;
            }
            return older ? older : fail(rc, this_err);
        }
        for (auto &o : ctx->ws)
            if (&o != w && !o.busy && o.tb.cap < w->tb.cap) o.presize_like(*w);
        w->busy = true;
        w->cells = cells;
        w->call_id = ctx->call_id;
        ctx->last_ws = last = w;
        ctx->next_ws = (ctx->next_ws + 1) % N_SETS;
        g0 = g1;
    }
    if (sync) return quiesce(ctx);
    if (user && last) HIP_TRY(hipStreamWaitEvent(user, last->ev[5], 0));
    return NPORE_OK;
}

// A batch in host buffers (a.h_*: filled by the caller, the three public entry points and the file pipeline): what all
// of them refuse, then run_core.  Every group of reads uploads its own slice and downloads its own results (run_group):
// the copies of one group run beside the kernels of its neighbours, and the caller's arrays are used as they are.
// With a.h_raw, align()'s inputs are still inside BAM records: `h_raw` holds the heads of the records (fixed fields ...
// 4-bit bases) one after the other, h_raw_off[n + 1] where each starts, and the three offset arrays are the sizes
// pack_sizes_of found; every group unpacks its slice on the device (unpack_kernels.hpp) against the context's device
// copy of the FASTA (device_fasta).
int align_batch(npore_ctx *ctx, const AlignArgs &a, bool sync)
{
    if (!ctx) return fail(NPORE_E_INVALID, "null context");
    if (a.n_reads < 0) return fail(NPORE_E_INVALID, "n_reads < 0");
    if (a.n_reads == 0) return NPORE_OK;
    const bool inputs = a.h_raw ? a.h_raw_off && a.d_ctg : a.h_refs && a.h_seqs && a.h_cigs;
    if (!inputs || !a.h_out || !a.h_ref_off || !a.h_seq_off || !a.h_cig_off || !a.h_out_off || !a.h_out_len || !a.h_status)
        return fail(NPORE_E_INVALID, "null argument");
    if (!a.h_raw && a.h_out_off[a.n_reads] < a.h_out_off[0]) return fail(NPORE_E_INVALID, "out_off not ascending");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->deferred_rc) return quiesce(ctx);   // a group of an earlier asynchronous call failed
    return run_core(ctx, a, OutTarget{nullptr, nullptr, nullptr, nullptr}, nullptr, sync);
}

// AlignArgs of a batch whose offset arrays and output slots are the caller's (the inputs: h_refs ... or h_raw, by the caller)
AlignArgs host_batch_args(int64_t n_reads, const int64_t *ref_off, const int64_t *seq_off, const int64_t *cig_off, float indel_start,
                          float indel_extend, int max_b_rows, int r, char *out, const int64_t *out_off, int64_t *out_len, int32_t *status)
{
    AlignArgs a{n_reads, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ref_off, seq_off, cig_off,
                indel_start, indel_extend, max_b_rows, r};
    a.h_out = out; a.h_out_off = out_off; a.h_out_len = out_len; a.h_status = status;
    return a;
}

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
    if (tables) {
        ctx->h_sub.assign(sub_scores, sub_scores + 25);
        ctx->h_np.assign(np_scores, np_scores + np_elems);
        ok = ok && hipMalloc((void **)&ctx->d_sub, 25 * sizeof(float)) == hipSuccess &&
             hipMalloc((void **)&ctx->d_np, np_elems * sizeof(float)) == hipSuccess &&
             hipMemcpy(ctx->d_sub, sub_scores, 25 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(ctx->d_np, np_scores, np_elems * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    }
    for (auto &e : ctx->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
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
    npore_ctx_destroy(ctx->peer);
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();       // nothing of this context may still be running
    for (DevBuf *b : {&ctx->in_refs, &ctx->in_seqs, &ctx->in_cigs, &ctx->in_off, &ctx->out, &ctx->out_off, &ctx->out_len, &ctx->status,
                      &ctx->d_fasta, &ctx->d_ctg, &ctx->cms_raw, &ctx->cms_off, &ctx->cms_ranges, &ctx->cms_counts})
        b->release();
    for (auto &w : ctx->ws) {
        for (DevBuf *b : w.all) b->release();
        w.h_cnt.release();
        w.h_off.release();
        for (auto &e : w.ev)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : w.evc)
            if (e) (void)hipEventDestroy(e);
    }
    ctx->h_offs.release();
    if (ctx->d_sub) (void)hipFree(ctx->d_sub);
    if (ctx->d_np) (void)hipFree(ctx->d_np);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : {ctx->stream, ctx->s_fill[0], ctx->s_fill[1], ctx->s_post})
        if (st) (void)hipStreamDestroy(st);
    for (auto *sp : ctx->slots) delete sp;
    delete ctx;
}

// The FASTA on the device (once per FASTA and context) and, per BAM reference, where its contig lies there.
static int device_fasta(npore_ctx *ctx, const npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref)
{
    const size_t bytes = fa->off.empty() ? 0 : (size_t)fa->off.back();
    if (ctx->d_fasta_serial != fa->serial || ctx->d_fasta_bytes != bytes) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (int rc = ctx->d_fasta.ensure(bytes + 64)) return rc;
        HIP_TRY(hipMemcpy(ctx->d_fasta.p, fa->bases.p, bytes, hipMemcpyHostToDevice));
        ctx->d_fasta_serial = fa->serial;
        ctx->d_fasta_bytes = bytes;
    }
    const size_t nref = b->ref_names.size();
    std::vector<CtgEntry> tab(std::max<size_t>(1, nref), CtgEntry{nullptr, 0});
    for (size_t k = 0; k < nref; k++) {
        const int fi = fasta_of_ref[k];
        if (fi >= 0 && fi < (int)fa->names.size()) tab[k] = CtgEntry{ctx->d_fasta.as<char>() + fa->off[(size_t)fi], fa->len((size_t)fi)};
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));       // (no group of an earlier run still reads the table)
    if (int rc = ctx->d_ctg.ensure(tab.size() * sizeof(CtgEntry))) return rc;
    HIP_TRY(hipMemcpy(ctx->d_ctg.p, tab.data(), tab.size() * sizeof(CtgEntry), hipMemcpyHostToDevice));
    ctx->n_ctg = (int)nref;
    return NPORE_OK;
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
    AlignArgs a{n, d_refs, d_ref_off, d_seqs, d_seq_off, d_cigars, d_cig_off,
                offs, offs + (n + 1), offs + 2 * (n + 1),
                indel_start, indel_extend, max_b_rows, r};
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
    else if (k == "cms_batch_reads") { if (value < 1) return fail(NPORE_E_INVALID, "cms_batch_reads: at least 1"); ctx->cms_batch_reads = value; }
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
    std::unique_ptr<BamRecordWalker> walker;
    std::vector<int64_t> idx;
    int64_t idx_at = 0;
    if (one_pass) {
        if (int rc = one_pass_args_check(b, (int)h_rid.size(), h_rid.data(), 0)) return rc;
        walker.reset(new BamRecordWalker(b, (int)h_rid.size(), h_rid.data(), h_lo.data(), h_hi.data(), 0, threads, 0u));
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
                gate[(size_t)k] = cms_gate((uint32_t)r.flag(), r.pos(), r.l_seq(), r.cigar(), r.n_cigar(), exclude_flags, c.ranges.data(),
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
            const RecView r = rec_of(rf, k);
            kept.push_back(k);
            kept_rid.push_back(r.ref_id());
            rawo.push_back(rawo.back() + (((int64_t)(r.aux() - r.p) + 4 + 7) & ~7ll));
        }
        ht.t[CMS_T_BATCHES]++;
        const int64_t n = (int64_t)kept.size();
        if (n == 0) continue;
        if (!raw.ensure((size_t)rawo[(size_t)n] + 64) || !rawo_pin.ensure((size_t)(n + 1) * 8)) return fail(NPORE_E_NOMEM, "batch buffers");
        std::memcpy(rawo_pin.p, rawo.data(), (size_t)(n + 1) * 8);
        parallel_for((n + per - 1) / per, threads, [&](int64_t tix) {
            for (int64_t k = tix * per; k < std::min(n, (tix + 1) * per); k++) {
                const RecView r = rec_of(rf, kept[(size_t)k]);
                std::memcpy(raw.p + rawo[(size_t)k], rf.ptr[(size_t)kept[(size_t)k]], (size_t)(r.aux() - r.p) + 4);
            }
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
            HIP_TRY(hipEventRecord(ctx->ev[1], s));
            hipLaunchKernelGGL(confusion_records_kernel, dim3((unsigned)(k1 - k0)), dim3(256), 0, s, cp);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ctx->ev[2], s));
            HIP_TRY(hipStreamSynchronize(s));        // (the staging buffers and the planes are free again)
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
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

int64_t npore_debug_crc32(const uint8_t *p, int64_t n, uint32_t crc)
{
    if ((!p && n > 0) || n < 0) return fail(NPORE_E_INVALID, "null argument");
    return (int64_t)crc32_fast(crc, p, (size_t)n);
}

int npore_debug_dpp(uint32_t *out128)
{
    uint32_t *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, 128 * 4));
    hipLaunchKernelGGL(dpp_selftest_kernel, dim3(1), dim3(64), 0, 0, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out128, d, 128 * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipFree(d));
    return NPORE_OK;
}

int npore_debug_divcheck(int64_t *mismatches)
{
    unsigned long long *d = nullptr, h = 0;
    HIP_TRY(hipMalloc((void **)&d, 8));
    HIP_TRY(hipMemset(d, 0, 8));
    hipLaunchKernelGGL(divcheck_kernel, dim3(256), dim3(256), 0, 0, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipFree(d));
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
    pack_sizes_of(rf, n, ref_off, seq_off, cig_off, 0);
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
    return pack_records(b, rf, fa, fasta_of_ref, n, refs, ref_off, seqs, seq_off, cigs, cig_off, threads);
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
    const int rc = format_bam_into(b, b->api_fetch, n, finals, final_off, final_len, status, threads, b->recs, recs_len, nullptr);
    *recs = reinterpret_cast<const uint8_t *>(b->recs.p);
    return rc;
}
NPORE_CATCH_INT

int npore_bam_set_output(npore_bam *b, int format, const char *bai_path, int flags)
{
    if (!b || (format != NPORE_OUT_SAM && format != NPORE_OUT_BAM) || (flags & ~(NPORE_OUT_EOF | NPORE_OUT_PART))) return fail(NPORE_E_INVALID, "bad argument");
    b->out_format = format;
    b->out_bai = (format == NPORE_OUT_BAM && bai_path) ? bai_path : "";
    b->out_flags = flags;
    return NPORE_OK;
}

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
    const std::string bai = b->out_bai;
    const int flags = b->out_flags;
    b->out_format = NPORE_OUT_SAM;                   // (the setting holds for one run)
    b->out_bai.clear();
    b->out_flags = 0;
    std::fill(b->out_info, b->out_info + 4, 0);
    if (int rc = w.open(out_path, b->ref_names.size(), bai.empty() ? nullptr : bai.c_str(), (flags & NPORE_OUT_EOF) != 0, (flags & NPORE_OUT_PART) != 0)) return rc;
    std::vector<BamRecMeta> meta;
    for (int64_t k0 = 0; k0 < n; k0 += batch_reads) {
        const int64_t m = std::min(batch_reads, n - k0);
        if (int rc = fetch_records(b, idx + k0, m, threads, b->api_fetch)) return rc;
        int64_t len = 0;
        if (int rc = format_bam_into(b, b->api_fetch, m, finals, final_off + k0, final_len + k0, status + k0, threads, b->recs, &len, &meta)) return rc;
        if (int rc = w.add(reinterpret_cast<const uint8_t *>(b->recs.p), len, meta.data(), (int64_t)meta.size())) return rc;
    }
    return w.finish(b->out_info);
}
NPORE_CATCH_INT

namespace {
// pack the selected records into the slot (inputs of npore_align_batch) and size its output buffers
// (the records are in s.rf already)
int slot_pack_records(const npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, int64_t n, int threads, npore_batch_slot &s,
                      bool device_glue = false, bool compact = false)
{
    for (auto *v : {&s.ro, &s.so, &s.co, &s.oo, &s.fo}) v->assign((size_t)n + 1, 0);
    s.olen.assign((size_t)n, 0);
    s.flen.assign((size_t)n, 0);
    pack_sizes_of(s.rf, n, s.ro.data(), s.so.data(), s.co.data(), threads);
    if (!s.refs.ensure((size_t)s.ro[(size_t)n] + 64) || !s.seqs.ensure((size_t)s.so[(size_t)n] + 64) || !s.cigs.ensure((size_t)s.co[(size_t)n] + 64))
        return fail(NPORE_E_NOMEM, "batch buffers");
    if (!fa || !fasta_of_ref) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = pack_records(b, s.rf, fa, fasta_of_ref, n, reinterpret_cast<uint8_t *>(s.refs.p), s.ro.data(),
                              reinterpret_cast<uint8_t *>(s.seqs.p), s.so.data(), s.cigs.p, s.co.data(), threads, true))
        return rc;
    for (int64_t k = 0; k < n; k++) {
        const int64_t cap = (s.ro[(size_t)k + 1] - s.ro[(size_t)k]) + (s.so[(size_t)k + 1] - s.so[(size_t)k]);
        // (device glue: the slot receives the collapsed CIGAR text instead of the op string -- 2 bytes per op + 16 always suffice)
        s.oo[(size_t)k + 1] = s.oo[(size_t)k] + (device_glue ? 2 * cap + 16 : cap);
        s.fo[(size_t)k + 1] = s.fo[(size_t)k] + 2 * cap + 16;
    }
    // (compact: the texts come back compacted -- file_pipeline --, no page-locked copy of the slots is needed)
    if ((!compact && !s.alns.ensure((size_t)s.oo[(size_t)n] + 64)) || (!device_glue && !s.finals.ensure((size_t)s.fo[(size_t)n] + 64)))
        return fail(NPORE_E_NOMEM, "batch buffers");
    return NPORE_OK;
}
// device pack: the sizes as above, and instead of the three arrays the HEADS of the records (block_size word, fixed fields,
// name, CIGAR words, 4-bit bases -- about half of a record; qualities and tags are not needed on the device) copied one
// after the other into the slot's page-locked buffer; unpack_kernels.hpp does the rest per group.  Device glue only
// (the host glue reads the base arrays).
// as_bam (BAM mode): each record up to the end of its QUALITIES (the tags stay on the host), the reads' HP values, slots of
// 4 bytes per op + 16 (CIGAR words instead of text), and the bound of the batch's record bytes.
int slot_pack_raw(const npore_bam *b, const int32_t *fasta_of_ref, int n_fasta, int64_t n, int threads, npore_batch_slot &s, bool compact = false,
                  bool as_bam = false)
{
    if (as_bam && !s.hp_pin.ensure((size_t)n * 8 + 64)) return fail(NPORE_E_NOMEM, "batch buffers");
    s.rec_cap = 0;
    for (auto *v : {&s.ro, &s.so, &s.co, &s.oo, &s.fo}) v->assign((size_t)n + 1, 0);
    s.rawo.assign((size_t)n + 1, 0);
    s.olen.assign((size_t)n, 0);
    s.flen.assign((size_t)n, 0);
    pack_sizes_of(s.rf, n, s.ro.data(), s.so.data(), s.co.data(), threads);
    for (int64_t k = 0; k < n; k++) {
        const RecView r = rec_of(s.rf, k);
        const int32_t rid = r.ref_id();
        const int fi = (rid >= 0 && rid < (int32_t)b->ref_names.size()) ? fasta_of_ref[rid] : -1;
        if (fi < 0 || fi >= n_fasta) return fail(NPORE_E_INVALID, "a selected read lies on a contig that is not in the FASTA");
        s.rawo[(size_t)k + 1] = s.rawo[(size_t)k] + (int64_t)((as_bam ? r.aux() : r.qual()) - r.p) + 4;
        const int64_t cap = (s.ro[(size_t)k + 1] - s.ro[(size_t)k]) + (s.so[(size_t)k + 1] - s.so[(size_t)k]);
        s.oo[(size_t)k + 1] = s.oo[(size_t)k] + (as_bam ? 4 : 2) * cap + 16;
        if (as_bam) {
            const int64_t sl = s.so[(size_t)k + 1] - s.so[(size_t)k];
            reinterpret_cast<int64_t *>(s.hp_pin.p)[k] = rec_hp(r);
            s.rec_cap += 36 + r.l_read_name() + 4 * cap + 16 + (sl + 1) / 2 + sl + 7;
        }
    }
    if (!s.raw.ensure((size_t)s.rawo[(size_t)n] + 64) || (!compact && !s.alns.ensure((size_t)s.oo[(size_t)n] + 64))) return fail(NPORE_E_NOMEM, "batch buffers");
    const int64_t per = 16;
    parallel_for((n + per - 1) / per, threads, [&](int64_t t) {
        for (int64_t k = t * per; k < std::min(n, (t + 1) * per); k++) {
            char *dst = s.raw.p + s.rawo[(size_t)k];
            const size_t len = (size_t)(s.rawo[(size_t)k + 1] - s.rawo[(size_t)k]);
            std::memcpy(dst, s.rf.ptr[(size_t)k], len);
            cache_writeback(dst, len);         // page-locked staging about to cross PCIe: out of this core's cache first (hostio.hpp)
        }
    });
    return NPORE_OK;
}
int slot_pack(const npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx, int64_t n, int threads,
              npore_batch_slot &s)
{
    if (!pack_args_ok(b, idx, n)) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = fetch_records(b, idx, n, threads, s.rf)) return rc;
    return slot_pack_records(b, fa, fasta_of_ref, n, threads, s);
}
int slot_align(npore_ctx *ctx, int64_t n, float indel_start, float indel_extend, int max_b_rows, int r, int32_t *status,
               npore_batch_slot &s)
{
    return npore_align_batch(ctx, n, reinterpret_cast<uint8_t *>(s.refs.p), s.ro.data(), reinterpret_cast<uint8_t *>(s.seqs.p),
                             s.so.data(), s.cigs.p, s.co.data(), indel_start, indel_extend, max_b_rows, r, s.alns.p, s.oo.data(),
                             s.olen.data(), status);
}
// realign_read's glue (src/bam.pyx:65-78) and the SAM lines; reads refused by align() have no string and get an empty CIGAR
int slot_post(const npore_bam *b, const int64_t *idx, int64_t n, const int32_t *status, int threads, npore_batch_slot &s,
              double *ms_std = nullptr, bool device_glue = false, bool as_bam = false)
{
    // SAM text, or (a BAM-mode file run) the same reads' records
    auto format_into = [&](const char *finals, const int64_t *final_off) {
        return as_bam ? format_bam_into(b, s.rf, n, finals, final_off, s.flen.data(), status, threads, s.sam, &s.sam_len, &s.meta)
                      : format_sam_into(b, s.rf, n, finals, final_off, s.flen.data(), status, threads, s.sam, &s.sam_len);
    };
    if (device_glue) {          // the slots hold the final CIGAR text already (standardize_kernel)
        if (ms_std) *ms_std = 0.0;
        for (int64_t k = 0; k < n; k++) s.flen[(size_t)k] = s.olen[(size_t)k] > 0 ? s.olen[(size_t)k] : 0;
        if (s.ctext_copied > 0) {          // ... compacted (file_pipeline): the front of the compact buffer is here, the rest is fetched now
            const int64_t *coff = reinterpret_cast<const int64_t *>(s.coff_pin.p);
            int64_t extent = 0;
            for (int64_t k = 0; k < n; k++) {
                if (s.flen[(size_t)k] > 0 && coff[k] < 0) return fail(NPORE_E_HIP, "internal: compact text buffer overflow");
                if (s.flen[(size_t)k] > 0) extent = std::max(extent, coff[k] + s.flen[(size_t)k]);
            }
            if (extent > s.ctext_copied) {        // (texts far longer than usual: 0.5 bytes per base were sent with the batch)
                if (!s.ctext_pin.ensure((size_t)extent + 64)) return fail(NPORE_E_NOMEM, "batch buffers");
                HIP_TRY(hipMemcpy(s.ctext_pin.p, s.d_ctext.p, (size_t)extent, hipMemcpyDeviceToHost));
                s.ctext_copied = extent;
            }
            return format_into(s.ctext_pin.p, coff);
        }
        return format_into(s.alns.p, s.oo.data());
    }
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t *refs = reinterpret_cast<const uint8_t *>(s.refs.p), *seqs = reinterpret_cast<const uint8_t *>(s.seqs.p);
    parallel_for(n, threads, [&](int64_t k) {
        const int64_t l = s.olen[(size_t)k] > 0 ? s.olen[(size_t)k] : 0;
        s.flen[(size_t)k] = standardize_collapsed_into(s.alns.p + s.oo[(size_t)k], l, refs + s.ro[(size_t)k],     // 2 bytes per op + 16 always suffice
                                                       s.ro[(size_t)k + 1] - s.ro[(size_t)k], seqs + s.so[(size_t)k],
                                                       s.so[(size_t)k + 1] - s.so[(size_t)k], s.finals.p + s.fo[(size_t)k]);
    });
    if (ms_std) *ms_std = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    (void)idx;
    return format_into(s.finals.p, s.fo.data());
}
// BAM mode, records built on the device: nothing is formatted here -- the batch's bytes as they lie there, into page-locked
// memory, and from the records' lengths what the writer's index needs (reference, position and span are the input record's)
int slot_fetch_records(int64_t n, const int32_t *status, npore_batch_slot &s)
{
    const int64_t total = (int64_t)*reinterpret_cast<const unsigned long long *>(s.total_pin.p);
    const int64_t *len = reinterpret_cast<const int64_t *>(s.reclen_pin.p);
    if (total < 0 || total > s.rec_cap) return fail(NPORE_E_HIP, "internal: BAM record buffer overflow");
    s.meta.clear();
    int64_t sum = 0;
    for (int64_t k = 0; k < n; k++) {
        if (len[k] < 0) return fail(NPORE_E_HIP, "internal: BAM record buffer overflow");
        if (s.olen[(size_t)k] > 4 * 0xFFFF) return fail(NPORE_E_UNSUPPORTED, "a final CIGAR has more than 65535 operations (BAM output)");
        if ((len[k] == 0) != ((status[k] & NPORE_ST_BAD_INPUT) != 0)) return fail(NPORE_E_HIP, "internal: BAM records and status bits disagree");
        if (len[k] == 0) continue;
        const RecView r = rec_of(s.rf, k);
        s.meta.push_back(BamRecMeta{r.ref_id(), r.pos(), s.ro[(size_t)k + 1] - s.ro[(size_t)k], len[k]});
        sum += len[k];
    }
    if (sum != total) return fail(NPORE_E_HIP, "internal: BAM record sizes do not add up");
    if (!s.recs_pin.ensure((size_t)total + 64)) return fail(NPORE_E_NOMEM, "batch buffers");
    if (total > 0) HIP_TRY(hipMemcpy(s.recs_pin.p, s.d_recs.p, (size_t)total, hipMemcpyDeviceToHost));
    s.sam_len = total;
    return NPORE_OK;
}
}  // namespace


int npore_bam_realign_batch(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const int64_t *idx,
                            int64_t n, float indel_start, float indel_extend, int max_b_rows, int r, int threads,
                            const char **sam, int64_t *sam_len, int32_t *status)
try {
    if (!ctx || !b || !status || !sam || !sam_len) return fail(NPORE_E_INVALID, "null argument");
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->slots[0]) ctx->slots[0] = new npore_batch_slot();
    npore_batch_slot &s = *ctx->slots[0];
    auto t0 = clk::now();
    if (int rc = slot_pack(b, fa, fasta_of_ref, idx, n, threads, s)) return rc;
    b->stage_ms[0] = ms_since(t0);
    t0 = clk::now();
    if (int rc = slot_align(ctx, n, indel_start, indel_extend, max_b_rows, r, status, s)) return rc;
    b->stage_ms[1] = ms_since(t0);
    t0 = clk::now();
    double ms_std = 0.0;
    const int rc = slot_post(b, idx, n, status, threads, s, &ms_std);
    b->stage_ms[2] = ms_std;
    b->stage_ms[3] = ms_since(t0) - ms_std;
    *sam = s.sam.p;
    *sam_len = s.sam_len;
    return rc;
}
NPORE_CATCH_INT

}  // extern "C"

namespace {
// The BAM -> SAM pipeline over a stream of batches.  Stages: records + pack (helper threads, two batches ahead) | the
// device path of ONE context through its asynchronous entry point -- a batch is enqueued the moment it is packed and
// the call returns at once, so up to N_SETS batches are on the device, the upload / preparation of one and the
// traceback / download of another beside the fill kernel of a third (run_core) | standardise + SAM text + ordered write
// (helper threads, each behind the event recorded behind its batch's download).  A slot carries a batch through all
// stages; six slots cover two being packed, three on the device and one being written.
//   acquire(k, slot) -> the records of batch k in slot.rf: their number, 0 = no further batch, < 0 = failure (fail() called);
//     serial_acquire: called in batch order (the one-pass reader), else from the packing threads as they come;
//   on_status(k, m, status bits): in batch order, in front of the batch's text.
// Where a file run's output goes: the SAM text's FILE, or (npore_bam_set_output, which holds for one run) the BAM writer
struct RunOutput {
    FILE *fh = nullptr;
    std::unique_ptr<BgzfStoredWriter> bw;
    npore_bam *b = nullptr;
    int open(npore_bam *bam, const char *out_path)
    {
        b = bam;
        const int format = b->out_format, flags = b->out_flags;
        const std::string bai = b->out_bai;
        b->out_format = NPORE_OUT_SAM;
        b->out_flags = 0;
        b->out_bai.clear();
        std::fill(b->out_info, b->out_info + 4, 0);
        if (format == NPORE_OUT_BAM) {
            bw.reset(new BgzfStoredWriter());
            return bw->open(out_path, b->ref_names.size(), bai.empty() ? nullptr : bai.c_str(), (flags & NPORE_OUT_EOF) != 0, (flags & NPORE_OUT_PART) != 0);
        }
        fh = std::fopen(out_path, "ab");
        return fh ? NPORE_OK : fail(NPORE_E_INVALID, std::string("cannot open '") + out_path + "' for appending");
    }
    int close(int rc)
    {
        if (fh && std::fclose(fh) != 0 && rc == NPORE_OK) rc = fail(NPORE_E_INVALID, "close failed");
        fh = nullptr;
        if (bw && rc == NPORE_OK) rc = bw->finish(b->out_info);
        bw.reset();
        return rc;
    }
    ~RunOutput() { if (fh) std::fclose(fh); }
};

template <class Acquire, class OnStatus>
int file_pipeline(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, float indel_start, float indel_extend,
                  int max_b_rows, int r, int threads, FILE *fh, bool serial_acquire, Acquire acquire, OnStatus on_status,
                  BgzfStoredWriter *bw = nullptr)
{
    // (run_core refuses them too, but on a worker thread: refuse here, before a batch is read or a record written)
    if (!std::isfinite(indel_start) || !std::isfinite(indel_extend))
        return fail(NPORE_E_INVALID, "indel_start and indel_extend must be finite");
    for (auto &sp : ctx->slots)
        if (!sp) sp = new npore_batch_slot();
    const auto wall0 = std::chrono::steady_clock::now();
    for (auto &sp : ctx->slots) { std::fill(sp->t_ms, sp->t_ms + 6, 0.0); sp->rc = 0; sp->m = 0; }
    ctx->file_mark[0] = ctx->totals[0] + ctx->totals[1] + ctx->totals[2];
    ctx->file_mark[1] = ctx->totals[3] + ctx->totals[4];
    constexpr int S = npore_ctx::N_SLOTS;
    // Several batches are in the host stages at once (two being packed, up to two being written): each stage gets half
    // of the CPUs, so that the process does not run five times as many busy threads as it has CPUs -- under a cgroup quota
    // that ends in the whole process being throttled for the rest of the scheduling period
    const int half_threads = std::max(1, host_threads(threads) / 2);
    // (experiments: NPORE_PACK_THREADS / NPORE_POST_THREADS override the split)
    const int pack_threads = std::getenv("NPORE_PACK_THREADS") ? std::max(1, std::atoi(std::getenv("NPORE_PACK_THREADS"))) : half_threads;
    const int post_threads = std::getenv("NPORE_POST_THREADS") ? std::max(1, std::atoi(std::getenv("NPORE_POST_THREADS"))) : half_threads;
    const bool glue = ctx->device_glue != 0;      // realign_read's glue on the device: the slots receive the final CIGAR text
    // ... and align()'s inputs unpacked from the records on the device (the host glue needs the base arrays on the host)
    const bool dpack = glue && ctx->device_pack != 0 && !(std::getenv("NPORE_DEVICE_PACK") && std::atoi(std::getenv("NPORE_DEVICE_PACK")) == 0);
    if (dpack)
        if (int rc = device_fasta(ctx, b, fa, fasta_of_ref)) return rc;
    const int n_fasta = (int)fa->names.size();
    // BAM mode: the records are built on the device where the default pipeline runs (device pack + device glue:
    // bam_emit_kernels.hpp); with the host glue or the host pack the host twin makes them (format_bam_into)
    const bool dev_bam = bw != nullptr && dpack;
    // NPORE_PIPE_TRACE=1: one line per batch and stage boundary on stderr (ms since the call began)
    const bool trace = std::getenv("NPORE_PIPE_TRACE") != nullptr;
    std::mutex trace_m;
    auto mark = [&](const char *what, int64_t k) {
        if (!trace) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        std::lock_guard<std::mutex> lk(trace_m);
        std::fprintf(stderr, "pipe %8.2f ms  batch %3lld  %s\n", ms, (long long)k, what);
    };
    std::vector<std::future<void>> packed, posted;
    // batches leave in input order: `written` counts the batches that are through (written, or given up on);
    // `acquired` the batches whose records have been taken from a serial source
    std::mutex gate_m;
    std::condition_variable gate_cv;
    int64_t written = 0, acquired = 0;
    auto wait_for = [&](int64_t &counter, int64_t upto) {
        std::unique_lock<std::mutex> lk(gate_m);
        gate_cv.wait(lk, [&] { return counter >= upto; });
    };
    auto bump = [&](int64_t &counter) {
        { std::lock_guard<std::mutex> lk(gate_m); counter++; }
        gate_cv.notify_all();
    };
    auto start_pack = [&](int64_t k) {
        packed.push_back(std::async(std::launch::async, [&, k] {
            npore_batch_slot &s = *ctx->slots[(size_t)(k % S)];
            if (k >= S) wait_for(written, k - S + 1);          // the slot's previous batch has been written
            if (serial_acquire) wait_for(acquired, k);
            const auto t0 = std::chrono::steady_clock::now();
            mark("acquire begins", k);
            s.keep.clear();
            s.rc = 0;
            s.m = 0;
            bool bumped = !serial_acquire;
            try {                                       // (no exception may leave a task unseen: the batch fails instead)
                const int64_t m = acquire(k, s);
                mark("acquired", k);
                if (serial_acquire) { bump(acquired); bumped = true; }
                s.m = m > 0 ? m : 0;
                if (m < 0) s.rc = (int)m;
                else if (m > 0) s.rc = dpack ? slot_pack_raw(b, fasta_of_ref, n_fasta, m, pack_threads, s, glue, dev_bam)
                                             : slot_pack_records(b, fa, fasta_of_ref, m, pack_threads, s, glue, glue);
                if (s.rc) s.err = npore_last_error();
            } catch (const std::exception &e) {
                s.rc = NPORE_E_NOMEM;
                s.err = std::string("batch preparation: ") + e.what();
                s.m = 0;
            }
            if (!bumped) bump(acquired);                // (the batches behind this one must not wait for ever)
            s.t_ms[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            mark("packed", k);
        }));
    };
    auto start_post = [&](int64_t k) {
        posted.push_back(std::async(std::launch::async, [&, k] {
            npore_batch_slot &t = *ctx->slots[(size_t)(k % S)];
            struct Through { decltype(wait_for) &w; decltype(bump) &m; int64_t &c; int64_t k; ~Through() { w(c, k); m(c); } } through{wait_for, bump, written, k};
            if (t.rc) return;
            (void)hipSetDevice(ctx->device);
            auto t0 = std::chrono::steady_clock::now();
            if (hipEventSynchronize(t.done) != hipSuccess) { t.rc = NPORE_E_HIP; t.err = "waiting for a batch failed"; return; }
            mark("device done", k);
            t.t_ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            const int64_t m = t.m;
            std::memcpy(t.olen.data(), t.olen_pin.p, (size_t)m * 8);
            const int32_t *st = reinterpret_cast<const int32_t *>(t.st_pin.p);
            t0 = std::chrono::steady_clock::now();
            double ms_std = 0.0;
            try {
                t.rc = dev_bam ? slot_fetch_records(m, st, t) : slot_post(b, nullptr, m, st, post_threads, t, &ms_std, glue, bw != nullptr);
            } catch (const std::exception &e) {
                fail(NPORE_E_NOMEM, std::string("SAM text of a batch: ") + e.what());
                t.rc = NPORE_E_NOMEM;
            }
            const double ms_post = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            t.t_ms[2] += ms_std;
            t.t_ms[3] += ms_post - ms_std;
            if (t.rc) { t.err = npore_last_error(); return; }
            mark("text made", k);
            wait_for(written, k);                              // records in input order
            on_status(k, m, st);
            t0 = std::chrono::steady_clock::now();
            if (bw) {
                const char *bytes = dev_bam ? t.recs_pin.p : t.sam.p;
                if (bw->add(reinterpret_cast<const uint8_t *>(bytes), t.sam_len, t.meta.data(), (int64_t)t.meta.size())) { t.rc = NPORE_E_INVALID; t.err = npore_last_error(); }
            } else if (std::fwrite(t.sam.p, 1, (size_t)t.sam_len, fh) != (size_t)t.sam_len) { t.rc = NPORE_E_INVALID; t.err = "short write"; }
            t.t_ms[4] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            mark("written", k);
            t.keep.clear();
        }));
    };
    int rc = NPORE_OK;
    std::string err;
    start_pack(0);
    start_pack(1);
    for (int64_t k = 0; rc == NPORE_OK; k++) {
        npore_batch_slot &s = *ctx->slots[(size_t)(k % S)];
        packed[(size_t)k].wait();
        if (s.rc) { rc = s.rc; err = s.err; break; }
        if (s.m == 0) break;                                   // the source is exhausted
        start_pack(k + 2);
        const int64_t m = s.m;
        if (!s.olen_pin.ensure((size_t)m * 8 + 64) || !s.st_pin.ensure((size_t)m * 4 + 64)) { rc = NPORE_E_NOMEM; err = "batch buffers"; break; }
        if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) { rc = NPORE_E_HIP; err = "hipEventCreate"; break; }
        // (returns once the batch's groups are enqueued; waits only when all work sets of the context are still busy)
        mark("enqueue begins", k);
        // device glue: the texts come back compacted -- the front of the batch's compact buffer (0.5 bytes per base are
        // sent with the batch's last group; what usual reads need is a quarter of that) and the reads' offsets
        TextCompact cmp{};
        BamEmit emit{};
        s.ctext_copied = 0;
        if (dev_bam) {
            if (s.d_recs.ensure((size_t)s.rec_cap + 64) || s.d_cursor.ensure(64) || !s.ctext_pin.ensure(64) || !s.reclen_pin.ensure((size_t)m * 8 + 64) ||
                !s.total_pin.ensure(64)) { rc = NPORE_E_NOMEM; err = "batch buffers"; break; }
            emit = BamEmit{s.d_recs.as<uint8_t>(), s.rec_cap, s.d_cursor.as<unsigned long long>(), reinterpret_cast<const int64_t *>(s.hp_pin.p),
                           reinterpret_cast<int64_t *>(s.reclen_pin.p), reinterpret_cast<unsigned long long *>(s.total_pin.p)};
        } else if (glue) {
            // (a text takes whole 16-byte granules of the compact buffer: at most 15 bytes more than its slot)
            const int64_t slots = s.oo[(size_t)m] + 16 * m, bound = std::min(slots, slots / 4 + 4096);
            if (s.d_ctext.ensure((size_t)slots + 64) || s.d_cursor.ensure(64) || !s.ctext_pin.ensure((size_t)bound + 64) ||
                !s.coff_pin.ensure((size_t)m * 8 + 64)) { rc = NPORE_E_NOMEM; err = "batch buffers"; break; }
            cmp = TextCompact{s.d_ctext.as<uint8_t>(), s.d_cursor.as<unsigned long long>(), slots,
                              reinterpret_cast<int64_t *>(s.coff_pin.p), s.ctext_pin.p, bound};
            s.ctext_copied = bound;
        }
        char *const out_host = glue ? s.ctext_pin.p : s.alns.p;      // (with the compaction nothing is copied there)
        AlignArgs a = host_batch_args(m, s.ro.data(), s.so.data(), s.co.data(), indel_start, indel_extend, max_b_rows, r, out_host,
                                      s.oo.data(), reinterpret_cast<int64_t *>(s.olen_pin.p), reinterpret_cast<int32_t *>(s.st_pin.p));
        if (dpack) {
            a.h_raw = reinterpret_cast<uint8_t *>(s.raw.p); a.h_raw_off = s.rawo.data();
            a.d_ctg = ctx->d_ctg.as<CtgEntry>(); a.n_ctg = ctx->n_ctg;
        } else {
            a.h_refs = reinterpret_cast<uint8_t *>(s.refs.p); a.h_seqs = reinterpret_cast<uint8_t *>(s.seqs.p); a.h_cigs = s.cigs.p;
        }
        a.final_text = glue;
        if (dev_bam) a.bam = &emit;
        else if (glue) a.compact = &cmp;                             // (read while the groups are enqueued, not behind the call)
        s.rc = align_batch(ctx, a, false);
        if (s.rc) { rc = s.rc; err = npore_last_error(); s.err = err; break; }
        if (hipEventRecord(s.done, ctx->s_post) != hipSuccess) { rc = NPORE_E_HIP; err = "hipEventRecord"; s.rc = rc; s.err = err; break; }
        mark("enqueued", k);
        start_post(k);
    }
    for (auto &f : packed) if (f.valid()) f.wait();
    for (auto &f : posted) if (f.valid()) f.wait();
    {
        const int rcw = npore_ctx_wait(ctx);                   // stage clocks of every group; a failure found while a work set was recycled
        if (rcw && rc == NPORE_OK) { rc = rcw; err = npore_last_error(); }
    }
    for (auto &sp : ctx->slots) {
        if (rc == NPORE_OK && sp->rc) { rc = sp->rc; err = sp->err; }
        sp->keep.clear();
    }
    // stage clocks of this call: sums over the batches of the time each stage's thread spent (stages of
    // neighbouring batches overlap, so the sums exceed the wall time), the wall time, and the GPU's share
    std::fill(b->file_ms, b->file_ms + 8, 0.0);
    for (auto &sp : ctx->slots)
        for (int q = 0; q < 5; q++) b->file_ms[q] += sp->t_ms[q];
    b->file_ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    b->file_ms[6] = ctx->totals[0] + ctx->totals[1] + ctx->totals[2] - ctx->file_mark[0];     // stage clocks of the device path (prep + fill + traceback;
    b->file_ms[7] = ctx->totals[3] + ctx->totals[4] - ctx->file_mark[1];                     // H2D + D2H): SUMS over groups that run beside each other
    return rc == NPORE_OK ? NPORE_OK : fail(rc, err);
}
}  // namespace

extern "C" {

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
    if (!ctx || !b || !fa || !fasta_of_ref || !out_path || (n > 0 && (!idx || !status)) || batch_reads < 1) return fail(NPORE_E_INVALID, "bad argument");
    if (!pack_args_ok(b, idx, n)) return fail(NPORE_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    RunOutput out;
    if (int rco = out.open(b, out_path)) return rco;
    const int64_t nb = (n + batch_reads - 1) / batch_reads;
    int rc = file_pipeline(ctx, b, fa, fasta_of_ref, indel_start, indel_extend, max_b_rows, r, threads, out.fh, false,
                           [&](int64_t k, npore_batch_slot &s) -> int64_t {
                               if (k >= nb) return 0;
                               const int64_t m = std::min(batch_reads, n - k * batch_reads);
                               const int rcf = fetch_records(b, idx + k * batch_reads, m, threads, s.rf);
                               return rcf ? (int64_t)rcf : m;
                           },
                           [&](int64_t k, int64_t m, const int32_t *st) { std::memcpy(status + k * batch_reads, st, (size_t)m * 4); },
                           out.bw.get());
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
    BamRecordWalker walker(b, n_regions, ref_id, start, stop, max_reads, threads);
    RunOutput out;
    if (int rco = out.open(b, out_path)) return rco;
    int64_t n_bad = 0, ordinal0 = 0;
    auto on_status = [&](int64_t, int64_t m, const int32_t *st) {
        for (int64_t i = 0; i < m; i++)
            if (st[i]) {
                counts[(st[i] & NPORE_ST_BAD_INPUT) ? 1 : 2]++;
                if (n_bad < bad_cap) { bad_ord[n_bad] = ordinal0 + i; bad_status[n_bad] = st[i]; }
                n_bad++;
            }
        ordinal0 += m;
    };
    int rc = file_pipeline(ctx, b, fa, fasta_of_ref, indel_start, indel_extend, max_b_rows, r, threads, out.fh, true,
                           [&](int64_t, npore_batch_slot &s) { return walker.next_batch(s.rf, s.keep, batch_reads); }, on_status,
                           out.bw.get());
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
