// align_engine.hpp -- the device path of a batch of reads: a context's work sets, the geometry of a fill launch, and a
// group of reads through its stages (plan, reservation, upload, preparation, fill, traceback + output, download),
// group after group through the three-stage pipeline (run_core).  Included by npore_api.cpp, the only translation unit,
// in front of file_pipeline.hpp, which drives it batch by batch.
#pragma once
#include <atomic>
#include <cmath>

#include "devbuf.hpp"
#include "kernels.hpp"
#include "prep_kernels.hpp"
#include "annot_wave.hpp"
#include "unpack_kernels.hpp"
#include "bam_emit_kernels.hpp"
#include "bam_deflate_kernels.hpp"

using namespace npore;

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
    const int64_t *h_hp;         // [n_reads] page-locked: the reads' HP values (full: the bytes of kept aux in the staged heads)
    int64_t *h_rec_len;          // [n_reads] page-locked: bytes of every read's record (0: not written)
    unsigned long long *h_total; // page-locked: bytes of the batch's records
    // NPORE_OUT_DEFLATE (bam_deflate_kernels.hpp; deflate false: stored members, nothing more on the device): the three
    // kernels' arguments, and where the member-size table and the batch's four numbers come down with the last group
    bool deflate = false;
    DeflateParams dfl{};
    uint32_t *h_sizes = nullptr; // [dfl.max_members] page-locked
    int64_t *h_info = nullptr;   // [4] page-locked: DeflateParams::info
    RecSpec rec;                 // which records (hostio.hpp): FULL ones have their heads staged with STAGE_FULL, and NM, MD, cs and de
                                 // counted, sized and written on the device (nm_rec.hpp, md_rec.hpp, cs_rec.hpp)
};

struct npore_batch_slot;        // a batch of the BAM -> SAM pipeline (file_pipeline.hpp)

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
    DevBuf nm, md_len;                // ... FULL records: the group's NM counts; NPORE_OUT_MD: the bytes of its MD texts
    DevBuf cs_len, de_val;            // ... NPORE_TAG_*: the bytes of its cs texts, its de values
    DevBuf eqx_len;                   // ... NPORE_CIGAR_EQX: the words of its final CIGARs in =/X form
    DevBuf oc_len;                    // ... NPORE_TAG_OC: the bytes of its OC texts (0: the read did not change)
    HostBuf h_off;
    hipEvent_t evc[4] = {};      // H2D start / end, D2H start / end of a staged group
    bool staged = false;
    hipEvent_t ev[6] = {};       // prep start / end, fill start / end, traceback + gather start / end (= group done)
    bool busy = false;           // enqueued, not collected yet
    int64_t cells = 0, call_id = 0;
    ~WorkSet()
    {
        for (hipEvent_t e : {ev[0], ev[1], ev[2], ev[3], ev[4], ev[5], evc[0], evc[1], evc[2], evc[3]})
            if (e) (void)hipEventDestroy(e);
    }
    // An idle set takes the capacities of one that has just been given a group: the groups of a run are alike, so its
    // own first group then finds its buffers in place instead of allocating tens of GB in front of its kernels (with
    // three sets that was the THIRD step of a run -- 0.4 s in a timed region that had two warm-up steps)
    // The per-read arrays of the FULL records' tag kernels (nm, md_len, cs_len, de_val, eqx_len, oc_len) for nr reads of a run that writes `rec`
    int reserve_emit_tags(const RecSpec &rec, size_t nr)
    {
        if (int rc = rec.md ? md_len.ensure(nr * 4 + 64) : 0) return rc;
        if (int rc = rec.cs_de() ? cs_len.ensure(nr * 4 + 64) : 0) return rc;
        if (int rc = rec.cs_de() ? de_val.ensure(nr * 4 + 64) : 0) return rc;
        if (int rc = rec.eqx() ? eqx_len.ensure(nr * 4 + 64) : 0) return rc;
        if (int rc = rec.oc() ? oc_len.ensure(nr * 4 + 64) : 0) return rc;
        return rec.full ? nm.ensure(nr * 4 + 64) : NPORE_OK;
    }
    void presize_like(const WorkSet &o)
    {
        DevBuf WorkSet::*const all[] = {&WorkSet::rd_i32, &WorkSet::rd_i64, &WorkSet::steps, &WorkSet::inss, &WorkSet::descs, &WorkSet::sched,
                                        &WorkSet::hist, &WorkSet::counters, &WorkSet::tiles, &WorkSet::cwoff, &WorkSet::seqw, &WorkSet::refw,
                                        &WorkSet::refl, &WorkSet::seql, &WorkSet::tb, &WorkSet::cout_, &WorkSet::clen, &WorkSet::cstat,
                                        &WorkSet::cnruns, &WorkSet::in_refs, &WorkSet::in_seqs, &WorkSet::in_cigs, &WorkSet::in_off,
                                        &WorkSet::out, &WorkSet::out_len, &WorkSet::status, &WorkSet::in_raw, &WorkSet::coff,
                                        &WorkSet::in_hp, &WorkSet::rec_off, &WorkSet::rec_len, &WorkSet::nm, &WorkSet::md_len, &WorkSet::cs_len, &WorkSet::de_val,
                                        &WorkSet::eqx_len, &WorkSet::oc_len};
        for (auto m : all) (this->*m).match(o.*m);
    }
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
    hipEvent_t ev_user = nullptr;   // orders a batch behind what the caller's stream holds (run_core)
    hipEvent_t ev_cms[2] = {};      // around a confusion_records_kernel launch (npore_bam_confusion)
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
    int device_inflate = 0;     // one-pass BAM readers: the BGZF blocks inflated on the device (inflate_kernels.hpp), 0: on the host's threads
    // device pack: the FASTA of the current run on the device (uploaded once per FASTA), the contig of every BAM reference
    DevBuf d_fasta, d_ctg;
    DevBuf d_stream_pos;        // BAM out, NPORE_OUT_DEFLATE: where the next batch's records begin in the run's record stream (8 bytes)
    // recount of the confusion matrices from BAM records (npore_bam_confusion): the batch's record heads and their offsets,
    // the current contig's ranges, the counters
    DevBuf cms_raw, cms_off, cms_ranges, cms_counts;
    int64_t cms_batch_reads = 4000;
    // Gini purity of pileups from BAM records (npore_bam_purity; staging: the cms_ buffers): the window's counter planes and
    // sums of squares, the insertion events and their buckets, the scan's block sums, histograms | tallies | cursor, rows
    DevBuf pur_cnt, pur_v2, pur_ev, pur_sorted, pur_bsum, pur_out, pur_rows;
    int64_t purity_window = 1ll << 22;   // positions per counter window (npore_ctx_set "purity_window")
    uint64_t d_fasta_serial = 0;
    size_t d_fasta_bytes = 0;
    int n_ctg = 0;
    bool fill_has_room = false; // the last fill launch left LDS for such kernels on its CUs
    HostBuf h_offs;             // offset arrays of a device-resident batch (npore_align_batch_device)
    // annotation entry points (npore_get_np_info, npore_np_regions, npore_bam_confusion): bases, their offsets, the results
    DevBuf in_seqs, in_off, out;
    std::vector<int32_t> regions;                                    // npore_np_regions: positions, then repeat counts
    // host staging of the BAM -> SAM pipeline (npore_bam_realign_batch / _file): grow-only, reused across batches and files
    double file_mark[2] = {0, 0};      // totals at the start of npore_bam_realign_file (kernels, PCIe)
    static constexpr int N_SLOTS = 6;
    npore_batch_slot *slots[N_SLOTS] = {};       // made on first use, deleted by npore_ctx_destroy
    double timing[8] = {};
    // (npore_ctx_destroy has synchronised the device; the buffers and the work sets' events go with the members)
    ~npore_ctx()
    {
        if (d_sub) (void)hipFree(d_sub);
        if (d_np) (void)hipFree(d_np);
        for (hipEvent_t e : {ev_user, ev_cms[0], ev_cms[1]})
            if (e) (void)hipEventDestroy(e);
        for (hipStream_t st : {stream, s_fill[0], s_fill[1], s_post})
            if (st) (void)hipStreamDestroy(st);
    }
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
    int64_t read_base = 0;       // index of a group's first read in these arrays
};

// device pointers to the raw batch + host copies of the three offset arrays
struct AlignArgs {
    int64_t n_reads = 0;
    const uint8_t *d_refs = nullptr;
    const int64_t *d_ref_off = nullptr;
    const uint8_t *d_seqs = nullptr;
    const int64_t *d_seq_off = nullptr;
    const char *d_cigs = nullptr;
    const int64_t *d_cig_off = nullptr;
    const int64_t *h_ref_off = nullptr, *h_seq_off = nullptr, *h_cig_off = nullptr;
    float indel_start = 0.f, indel_extend = 0.f;
    int max_b_rows = 0, r = 0;
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

// How a group's results leave: chosen once (plan_group), acted on by reserve_group, post_group and download_group
enum class OutMode {
    OpStrings,     // align()'s op string of every read in its slot
    FinalText,     // the collapsed, standardised CIGAR text in the slots (AlignArgs::final_text)
    CompactText,   // ... compacted to the front of the batch's compact buffer (AlignArgs::compact)
    BamRecords     // the final CIGARs as words, the batch's BAM records built from them (AlignArgs::bam)
};

// What follows for reads [g0, g1) from the host offset arrays and the arguments (plan_group: no HIP call)
struct GroupPlan {
    int64_t g0 = 0, g1 = 0, nr = 0;
    int tbs = 0;                                    // traceback words per anti-diagonal
    int64_t cig_bytes = 0, S_tot = 0, R_tot = 0;
    int64_t max_len = 0;                            // longest chunk slice: never beyond its sequence, nor max_b_rows + 1 bases
    int64_t max_chunks = 0, max_tiles = 0;          // upper bounds; CIGAR tiles (prep_kernels.hpp): every read has at least one
    int64_t steps_cap = 0, tb_words = 0, raw_bytes = 0, out_bytes = 0;   // (the last two: a staged group's record heads and output slots)
    bool staged = false, raw = false;               // uploads and downloads its own slice; ... of record heads, unpacked here
    OutMode mode = OutMode::OpStrings;
};

int plan_group(const AlignArgs &a, int64_t g0, int64_t g1, GroupPlan &p)
{
    p.g0 = g0; p.g1 = g1; p.nr = g1 - g0;
    p.tbs = tb_stride(a.r);
    p.staged = a.staged(); p.raw = p.staged && a.h_raw;
    p.mode = !a.final_text ? OutMode::OpStrings : a.bam ? OutMode::BamRecords : a.compact ? OutMode::CompactText : OutMode::FinalText;
    if (p.mode == OutMode::BamRecords && !p.raw) return fail(NPORE_E_INVALID, "internal: BAM records on the device need the device pack");
    p.cig_bytes = a.h_cig_off[g1] - a.h_cig_off[g0];
    p.S_tot = a.h_seq_off[g1] - a.h_seq_off[g0]; p.R_tot = a.h_ref_off[g1] - a.h_ref_off[g0];
    for (int64_t k = g0; k < g1; k++) {
        const int64_t cl = a.h_cig_off[k + 1] - a.h_cig_off[k];
        p.max_len = std::max({p.max_len, a.h_seq_off[k + 1] - a.h_seq_off[k], a.h_ref_off[k + 1] - a.h_ref_off[k]});
        p.max_chunks += chunk_bound(cl, a.max_b_rows);
        p.max_tiles += std::max<int64_t>(1, (cl + CIGAR_TILE - 1) / CIGAR_TILE);
    }
    if (p.max_chunks > (1ll << 30)) return fail(NPORE_E_UNSUPPORTED, "too many chunks in one group");
    if (p.max_tiles > (1ll << 30)) return fail(NPORE_E_UNSUPPORTED, "too many CIGAR tiles in one group");
    p.steps_cap = 2 * p.cig_bytes + 512;
    p.tb_words = (2 * p.cig_bytes + p.max_chunks) * p.tbs;
    p.raw_bytes = p.raw ? a.h_raw_off[g1] - a.h_raw_off[g0] : 0;
    p.out_bytes = p.staged ? a.h_out_off[g1] - a.h_out_off[g0] : 0;
    return NPORE_OK;
}

// A staged group's offset block (h_off here, in_off on the device): five arrays of nr + 1 offsets behind each other, in this
// order -- of the refs, the seqs, the CIGARs, the output slots (BAM records: the final's words) and the record heads
enum GroupOff : int { OFF_REF = 0, OFF_SEQ, OFF_CIG, OFF_OUT, OFF_RAW, OFF_ARRAYS };
template <class T> T *group_off(T *block, int which, int64_t nr) { return block + which * (nr + 1); }

// Every buffer of the work set the group's stages use, each under the condition of its use, before the first enqueue
// (a buffer that grows is a hipFree, which synchronises the device)
int reserve_group(WorkSet *w, const GroupPlan &p, const AlignArgs &a)
{
    const size_t nr = (size_t)p.nr, mc = (size_t)p.max_chunks;
    if (int rc = w->rd_i32.ensure((5 * nr + 16) * 4)) return rc;
    if (int rc = w->tiles.ensure((size_t)p.max_tiles * 24 + 64)) return rc;
    if (int rc = w->cwoff.ensure(mc * 8 + 64)) return rc;
    if (int rc = w->rd_i64.ensure((nr + 2) * 8)) return rc;
    if (int rc = w->steps.ensure((size_t)p.steps_cap)) return rc;
    if (int rc = w->inss.ensure((size_t)(2 * p.cig_bytes + p.nr + 16) * 4)) return rc;
    if (int rc = w->descs.ensure(mc * sizeof(ChunkDesc))) return rc;
    if (int rc = w->sched.ensure(mc * 4)) return rc;
    if (int rc = w->hist.ensure((size_t)(a.max_b_rows + 2) * 4)) return rc;
    if (int rc = w->counters.ensure(64)) return rc;
    if (int rc = w->seqw.ensure((size_t)(p.S_tot + p.max_chunks + 16) * 4)) return rc;
    if (int rc = w->refw.ensure((size_t)(p.R_tot + p.max_chunks + 16) * 16)) return rc;
    if (int rc = w->refl.ensure((size_t)(p.R_tot + p.max_chunks + 16) * 8)) return rc;
    if (int rc = w->tb.ensure((size_t)p.tb_words * 4 + 64)) return rc;
#if defined(NPORE_EXPERIMENTS)
    if (const char *e = std::getenv("NPORE_DBGMAT"))
        if (int rc = w->dbg.ensure((size_t)p.tb_words * 4 * (size_t)std::max(1, std::atoi(e)) + 64)) return rc;
#endif
    if (int rc = w->cout_.ensure(((size_t)(p.S_tot + p.R_tot) + 64) * 4)) return rc;
    for (DevBuf *b : {&w->cnruns, &w->clen, &w->cstat})
        if (int rc = b->ensure(mc * 4 + 64)) return rc;
    if (int rc = w->h_cnt.ensure(64)) return rc;
    if (!p.staged) return NPORE_OK;
    if (int rc = w->h_off.ensure(OFF_ARRAYS * (nr + 1) * 8)) return rc;
    if (int rc = w->in_refs.ensure((size_t)p.R_tot + 64)) return rc;
    if (int rc = w->in_seqs.ensure((size_t)p.S_tot + 64)) return rc;
    if (int rc = w->in_cigs.ensure((size_t)p.cig_bytes + 64)) return rc;
    if (int rc = w->in_off.ensure(OFF_ARRAYS * (nr + 1) * 8)) return rc;
    if (int rc = w->out.ensure((size_t)p.out_bytes + 64)) return rc;
    if (int rc = w->out_len.ensure(nr * 8)) return rc;
    if (int rc = w->status.ensure(nr * 4)) return rc;
    if (p.raw)
        if (int rc = w->in_raw.ensure((size_t)p.raw_bytes + 64)) return rc;
    if (p.mode == OutMode::CompactText) return w->coff.ensure(nr * 8 + 64);
    if (p.mode != OutMode::BamRecords) return NPORE_OK;
    for (DevBuf *b : {&w->in_hp, &w->rec_off, &w->rec_len})
        if (int rc = b->ensure(nr * 8 + 64)) return rc;
    return w->reserve_emit_tags(a.bam->rec, nr);
}

// The device addresses of a group whose buffers are reserved: the preparation's arrays (the later stages read them from
// here) and, in `out` (on entry the caller's device arrays), where the output tail writes.  A staged group has its own slice
// in the work set (in_off: GroupOff), any other the caller's arrays.
PrepParams wire_group(const npore_ctx *ctx, WorkSet *w, const GroupPlan &p, const AlignArgs &a, OutTarget &out)
{
    const int64_t nr = p.nr;
    PrepParams pp;
    pp.n_reads = nr;
    if (p.staged) {
        const int64_t *d_off = w->in_off.as<int64_t>();
        pp.refs = w->in_refs.as<uint8_t>(); pp.ref_off = group_off(d_off, OFF_REF, nr);
        pp.seqs = w->in_seqs.as<uint8_t>(); pp.seq_off = group_off(d_off, OFF_SEQ, nr);
        pp.cigs = w->in_cigs.as<char>(); pp.cig_off = group_off(d_off, OFF_CIG, nr);
        out = OutTarget{w->out.as<uint8_t>(), group_off(d_off, OFF_OUT, nr), w->out_len.as<int64_t>(), w->status.as<int32_t>(), 0};
    } else {
        pp.refs = a.d_refs; pp.ref_off = a.d_ref_off + p.g0;
        pp.seqs = a.d_seqs; pp.seq_off = a.d_seq_off + p.g0;
        pp.cigs = a.d_cigs; pp.cig_off = a.d_cig_off + p.g0;
        out.read_base = p.g0;
    }
    pp.max_b_rows = a.max_b_rows; pp.r = a.r; pp.tbstride = p.tbs; pp.max_n = ctx->max_n; pp.max_l = ctx->max_l;
    pp.max_chunks = (int)p.max_chunks;
    int32_t *i32 = w->rd_i32.as<int32_t>();
    pp.rd_nsteps = i32; pp.rd_nchunks = i32 + nr; pp.rd_status = i32 + 2 * nr;
    pp.rd_chunk_first = i32 + 3 * nr;      // nr + 1 entries
    pp.rd_tile_first = i32 + 4 * nr + 4;   // nr + 1 entries
    pp.tile_cnt = w->tiles.as<int4>();
    pp.tile_base = reinterpret_cast<int2 *>(w->tiles.as<char>() + (size_t)p.max_tiles * 16);
    pp.rd_steps_off = w->rd_i64.as<int64_t>();
    pp.steps = w->steps.as<uint8_t>(); pp.inss = w->inss.as<int32_t>();
    pp.descs = w->descs.as<ChunkDesc>(); pp.sched = w->sched.as<int32_t>();
    pp.hist = w->hist.as<int32_t>(); pp.counters = w->counters.as<int32_t>();
    pp.seqw = w->seqw.as<uint32_t>(); pp.refw = w->refw.as<uint4>(); pp.refl = w->refl.as<uint2>();
    return pp;
}

// The unpack of a staged group's nr record heads into the work set's three arrays (pass_mask: these stay as they are)
UnpackParams wire_unpack(WorkSet *w, int64_t nr, const CtgEntry *ctg, int n_ctg, uint32_t pass_mask)
{
    const int64_t *d_off = w->in_off.as<int64_t>();
    UnpackParams up;
    up.raw = w->in_raw.as<uint8_t>(); up.raw_off = group_off(d_off, OFF_RAW, nr);
    up.ctg = ctg; up.n_ctg = n_ctg;
    up.refs = w->in_refs.as<uint8_t>(); up.ref_off = group_off(d_off, OFF_REF, nr);
    up.seqs = w->in_seqs.as<uint8_t>(); up.seq_off = group_off(d_off, OFF_SEQ, nr);
    up.cigs = w->in_cigs.as<char>(); up.cig_off = group_off(d_off, OFF_CIG, nr);
    up.n_reads = nr;
    up.pass_mask = pass_mask;
    return up;
}
// The emit launch of a staged group of nr reads whose final CIGARs lie as words in the work set's output slots (the group's
// own slice: read_base 0), for the records `rec` names, into the record buffer recs / cap / cursor
BamEmitParams wire_bam_emit(WorkSet *w, int64_t nr, uint8_t *recs, int64_t cap, unsigned long long *cursor, const RecSpec &rec)
{
    const int64_t *d_off = w->in_off.as<int64_t>();
    BamEmitParams bp;
    bp.raw = w->in_raw.as<uint8_t>(); bp.raw_off = group_off(d_off, OFF_RAW, nr);
    bp.ref_off = group_off(d_off, OFF_REF, nr); bp.seq_off = group_off(d_off, OFF_SEQ, nr);
    bp.hp = w->in_hp.as<int64_t>();
    bp.words = w->out.as<uint8_t>(); bp.words_off = group_off(d_off, OFF_OUT, nr); bp.words_len = w->out_len.as<int64_t>(); bp.status = w->status.as<int32_t>();
    bp.read_base = 0; bp.n_reads = nr;
    bp.recs = recs; bp.cap = cap; bp.cursor = cursor;
    bp.rec_off = w->rec_off.as<int64_t>(); bp.rec_len = w->rec_len.as<int64_t>();
    if (rec.full) {                       // FULL records: NM from the group's code arrays, then the same two steps
        bp.refs = w->in_refs.as<uint8_t>(); bp.seqs = w->in_seqs.as<uint8_t>(); bp.nm = w->nm.as<int32_t>();
        bp.pass_mask = rec.pass_mask;
        if (rec.md) bp.md_len = w->md_len.as<int32_t>();      // (MD: its size in front of the placement, its text behind the record)
        if (rec.cs_de()) { bp.tags = rec.cs_de(); bp.cs_len = w->cs_len.as<int32_t>(); bp.de = w->de_val.as<float>(); }      // (cs / de: the same)
        if (rec.eqx()) bp.eqx_len = w->eqx_len.as<int32_t>();      // (=/X: the count of its words in front of the placement, the words behind the record)
        if (rec.oc()) bp.oc_len = w->oc_len.as<int32_t>();         // (OC: changed or not and its size in front of the placement, its text behind the record)
    }
    return bp;
}

// ---- the stages of a group.  Each enqueues, none waits for the device.

// A staged group's slice to the device: bases + CIGAR ops as they lie (or the record heads, unpacked there into the same
// three arrays: unpack_kernels.hpp), the offset arrays rebased to the slice, BAM mode's HP values
int upload_group(npore_ctx *ctx, WorkSet *w, const GroupPlan &p, const AlignArgs &a)
{
    hipStream_t s = ctx->stream;
    const int64_t nr = p.nr, g0 = p.g0;
    int64_t *ho = w->h_off.as<int64_t>(), *hro = group_off(ho, OFF_REF, nr), *hso = group_off(ho, OFF_SEQ, nr), *hco = group_off(ho, OFF_CIG, nr),
            *hoo = group_off(ho, OFF_OUT, nr), *hraw = group_off(ho, OFF_RAW, nr);
    for (int64_t i = 0; i <= nr; i++) {
        hro[i] = a.h_ref_off[g0 + i] - a.h_ref_off[g0]; hso[i] = a.h_seq_off[g0 + i] - a.h_seq_off[g0];
        hco[i] = a.h_cig_off[g0 + i] - a.h_cig_off[g0]; hoo[i] = a.h_out_off[g0 + i] - a.h_out_off[g0];
    }
    for (int64_t i = 0; p.raw && i <= nr; i++) hraw[i] = a.h_raw_off[g0 + i] - a.h_raw_off[g0];
    HIP_TRY(hipEventRecord(w->evc[0], s));
    if (p.raw) {
        HIP_TRY(hipMemcpyAsync(w->in_raw.p, a.h_raw + a.h_raw_off[g0], (size_t)p.raw_bytes, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(hipMemcpyAsync(w->in_refs.p, a.h_refs + a.h_ref_off[g0], (size_t)p.R_tot, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(w->in_seqs.p, a.h_seqs + a.h_seq_off[g0], (size_t)p.S_tot, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(w->in_cigs.p, a.h_cigs + a.h_cig_off[g0], (size_t)p.cig_bytes, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(w->in_off.p, ho, (size_t)(group_off(ho, OFF_ARRAYS, nr) - ho) * 8, hipMemcpyHostToDevice, s));
    if (p.mode == OutMode::BamRecords)
        HIP_TRY(hipMemcpyAsync(w->in_hp.p, a.bam->h_hp + g0, (size_t)nr * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(w->evc[1], s));
    if (p.raw) {
        hipLaunchKernelGGL(unpack_records_kernel, dim3((unsigned)nr), dim3(256), 0, s,
                           wire_unpack(w, nr, a.d_ctg, a.n_ctg, a.bam ? a.bam->rec.pass_mask : PASS_NONE));
        HIP_TRY(hipGetLastError());
    }
    return NPORE_OK;
}

// CIGAR -> path -> chunks -> schedule, and the chunks' annotated words (prep_kernels.hpp, annot_wave.hpp)
int prep_group(npore_ctx *ctx, WorkSet *w, const GroupPlan &p, const PrepParams &pp, bool beside_fill)
{
    hipStream_t s = ctx->stream;
    const unsigned scan_threads = beside_fill ? 256 : 1024;
#if defined(NPORE_EXPERIMENTS)
    if (std::getenv("NPORE_DBGMAT") && w->dbg.p) (void)hipMemsetAsync(w->dbg.p, 0, w->dbg.cap, s);     // (steps of the compiled path leave zeros)
#endif
    HIP_TRY(hipEventRecord(w->ev[0], s));
    HIP_TRY(hipMemsetAsync(pp.hist, 0, (size_t)(pp.max_b_rows + 2) * 4, s));
    const unsigned rd_blocks = (unsigned)((p.nr + 3) / 4), ch_blocks = (unsigned)((p.max_chunks + 255) / 256);
    const unsigned tile_blocks = (unsigned)((p.max_tiles + 3) / 4);
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
    if (ctx->max_n == MAX_PERIOD) hipLaunchKernelGGL(annotate_wave_kernel<true>, dim3((unsigned)(2 * p.max_chunks)), dim3(64), 0, s, pp);
    else hipLaunchKernelGGL(annotate_wave_kernel<false>, dim3((unsigned)(2 * p.max_chunks)), dim3(64), 0, s, pp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w->ev[1], s));
    return NPORE_OK;
}

// The fill kernel, behind this group's preparation.  Consecutive groups alternate between two streams: their fill
// kernels share nothing, so the next one's persistent workgroups move onto the CUs that this one's leave as its
// last chunks run out -- the tail of one launch is filled by the head of the next (C2, steps back to back:
// 17.1 ms per step against the 18.0 ms one fill kernel takes alone; one stream: 18.1)
int fill_group(npore_ctx *ctx, WorkSet *w, const GroupPlan &p, const AlignArgs &a, const PrepParams &pp, int shape, bool overlapping)
{
    hipStream_t s = ctx->s_fill[ctx->next_fill];
    if (ctx->fill_streams == 2) ctx->next_fill ^= 1;
    HIP_TRY(hipStreamWaitEvent(s, w->ev[1], 0));
    HIP_TRY(hipEventRecord(w->ev[2], s));
    KParams kp;
    kp.descs = pp.descs; kp.sched = pp.sched;
    kp.n_chunks = pp.counters; kp.queue = pp.counters + 2;
    kp.steps = pp.steps; kp.inss = pp.inss;
    kp.seqw = pp.seqw; kp.refw = pp.refw; kp.refl = pp.refl;
    kp.tb = w->tb.as<uint32_t>(); kp.dbg = w->dbg.as<uint32_t>();
    kp.sub_scores = ctx->d_sub; kp.np_scores = ctx->d_np; kp.max_n = ctx->max_n; kp.max_l = ctx->max_l;
    kp.r = a.r; kp.tbstride = p.tbs; kp.indel_start = a.indel_start; kp.indel_extend = a.indel_extend;
    // by waves per chunk: 1 ... 8 compiled for their count, 9 ... 16 the instantiation that takes it from the launch
    static constexpr decltype(&launch_fill<0>) by_shape[9] = {launch_fill<1>, launch_fill<2>, launch_fill<3>, launch_fill<4>, launch_fill<5>,
                                                              launch_fill<6>, launch_fill<7>, launch_fill<8>, launch_fill<0>};
    if (shape < 1 || shape > MAX_WAVES_PER_CHUNK) return fail(NPORE_E_UNSUPPORTED, "unsupported waves-per-chunk count");
    const hipError_t e = by_shape[std::min(shape, 9) - 1](kp, (int)p.max_chunks, ctx->force_chunks, ctx->n_cus, s, overlapping, &ctx->fill_has_room);
    if (e != hipSuccess) return fail(NPORE_E_HIP, std::string("fill launch: ") + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(w->ev[3], s));
    return NPORE_OK;
}

// NPORE_OUT_DEFLATE: the whole members inside a batch's record bytes, coded (bam_deflate_kernels.hpp).  The grids cover the
// most members the record buffer can hold; the kernels find on the device how many there are.
inline void launch_deflate(const DeflateParams &dp, hipStream_t s)
{
    if (dp.max_members <= 0) return;
    const bool match = dp.mode == DEFLATE_MODE_MATCH;           // (NPORE_OUT_MATCH: the planning and the emitting kernel with matches)
    hipLaunchKernelGGL(match ? plan_match_kernel : plan_deflate_kernel, dim3((unsigned)dp.max_members), dim3(64), 0, s, dp);
    hipLaunchKernelGGL(place_deflate_kernel, dim3(1), dim3(256), 0, s, dp);
    hipLaunchKernelGGL(match ? emit_match_kernel : emit_deflate_kernel, dim3((unsigned)dp.max_members + 2), dim3(64), 0, s, dp);      // (+ 2: the fragments)
}

// Traceback + output, behind this group's fill and beside the next group's; the tail is chosen by the plan's OutMode
int post_group(npore_ctx *ctx, WorkSet *w, const GroupPlan &p, const AlignArgs &a, const PrepParams &pp, const OutTarget &out, bool beside_fill)
{
    hipStream_t s = ctx->s_post;
    const int64_t nr = p.nr;
    HIP_TRY(hipStreamWaitEvent(s, w->ev[3], 0));
    HIP_TRY(hipEventRecord(w->ev[4], s));
    TParams tp;
    tp.descs = pp.descs; tp.n_chunks = pp.counters;
    tp.tb = w->tb.as<uint32_t>(); tp.inss = pp.inss;
    tp.chunk_runs = w->cout_.as<uint32_t>(); tp.chunk_nruns = w->cnruns.as<int32_t>();
    tp.chunk_len = w->clen.as<int32_t>(); tp.chunk_status = w->cstat.as<int32_t>(); tp.r = a.r; tp.tbstride = p.tbs;
    // (10 kb reads: 0.53 ms at 500 chunk slots, 0.83 ms at 8 000)
    hipLaunchKernelGGL(traceback_rows_kernel, dim3((unsigned)p.max_chunks), dim3(64), 0, s, tp);
    HIP_TRY(hipGetLastError());

    GParams gp;
    gp.descs = pp.descs; gp.read_first_chunk = pp.rd_chunk_first;
    gp.chunk_runs = tp.chunk_runs; gp.chunk_nruns = tp.chunk_nruns;
    gp.chunk_len = tp.chunk_len; gp.chunk_status = tp.chunk_status;
    gp.read_status_in = pp.rd_status; gp.counters = pp.counters;
    gp.seqs = pp.seqs; gp.refs = pp.refs;
    gp.out = out.d_out; gp.out_off = out.d_out_off; gp.out_len = out.d_out_len; gp.status = out.d_status;
    gp.read_base = out.read_base; gp.n_reads = nr;
    gp.chunk_woff = w->cwoff.as<int64_t>();
    hipLaunchKernelGGL(gather_scan_kernel, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, s, gp);
    if (p.mode == OutMode::OpStrings) {
        // LDS of gather_kernel: one tile of ops + (when a chunk's two base slices fit beside it) the slices
        const int64_t rows_max = std::min<int64_t>(p.max_len, a.max_b_rows) + 1;    // longest slice of any chunk
        if (beside_fill) {
            gp.slice_cap = 0;
            hipLaunchKernelGGL(gather_kernel<false>, dim3((unsigned)p.max_chunks), dim3(256), 0, s, gp);
        } else {
            gp.slice_cap = rows_max <= 24 * 1024 ? (int)((rows_max + 15) & ~(int64_t)15) : 0;
            const size_t glds = (size_t)GATHER_TILE + 2 * (size_t)gp.slice_cap;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&gather_kernel<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)glds));
            hipLaunchKernelGGL(gather_kernel<true>, dim3((unsigned)p.max_chunks), dim3(256), glds, s, gp);
        }
        HIP_TRY(hipGetLastError());
        return NPORE_OK;
    }
    StdKParams sp;                       // realign_read's glue, one wavefront per read: text, or (BAM mode) CIGAR words
    sp.descs = pp.descs; sp.read_first_chunk = pp.rd_chunk_first;
    sp.chunk_runs = tp.chunk_runs; sp.chunk_nruns = tp.chunk_nruns;
    sp.refs = pp.refs; sp.ref_off = pp.ref_off;
    sp.seqs = pp.seqs; sp.seq_off = pp.seq_off;
    sp.out = gp.out; sp.out_off = gp.out_off; sp.out_len = gp.out_len; sp.status = gp.status;
    sp.read_base = out.read_base; sp.n_reads = nr;
    if (p.mode == OutMode::BamRecords) hipLaunchKernelGGL(standardize_words_kernel, dim3((unsigned)nr), dim3(64), 0, s, sp);
    else hipLaunchKernelGGL(standardize_kernel, dim3((unsigned)nr), dim3(64), 0, s, sp);
    if (p.mode == OutMode::BamRecords) {          // the group's records behind those of the groups before it (bam_emit_kernels.hpp)
        if (p.g0 == 0) HIP_TRY(hipMemsetAsync(a.bam->d_cursor, 0, 8, s));
        launch_bam_emit(wire_bam_emit(w, nr, a.bam->d_recs, a.bam->cap, a.bam->d_cursor, a.bam->rec), a.bam->rec.full, s);
        if (a.bam->deflate && p.g1 == a.n_reads) launch_deflate(a.bam->dfl, s);      // the batch's records are complete
    } else if (p.mode == OutMode::CompactText) {  // the texts to the front of the batch's compact buffer (unpack_kernels.hpp)
        if (p.g0 == 0) HIP_TRY(hipMemsetAsync(a.compact->d_cursor, 0, 8, s));
        CompactParams cp;
        cp.out = sp.out; cp.out_off = sp.out_off; cp.out_len = sp.out_len;
        cp.read_base = out.read_base; cp.n_reads = nr;
        cp.ctext = a.compact->d_ctext; cp.cap = a.compact->cap; cp.cursor = a.compact->d_cursor;
        cp.coff = w->coff.as<int64_t>();
        hipLaunchKernelGGL(compact_texts_kernel, dim3((unsigned)nr), dim3(64), 0, s, cp);
    }
    HIP_TRY(hipGetLastError());
    return NPORE_OK;
}

// A staged group's slice of the results to the host; of every group the chunk count, the overflow flag and the last event
int download_group(npore_ctx *ctx, WorkSet *w, const GroupPlan &p, const AlignArgs &a)
{
    hipStream_t s = ctx->s_post;
    const int64_t nr = p.nr, g0 = p.g0;
    if (p.staged) {
        HIP_TRY(hipEventRecord(w->evc[2], s));
        if (p.mode == OutMode::BamRecords) {
            HIP_TRY(hipMemcpyAsync(a.bam->h_rec_len + g0, w->rec_len.p, (size_t)nr * 8, hipMemcpyDeviceToHost, s));
            if (p.g1 == a.n_reads) HIP_TRY(hipMemcpyAsync(a.bam->h_total, a.bam->d_cursor, 8, hipMemcpyDeviceToHost, s));
            if (p.g1 == a.n_reads && a.bam->deflate) {
                HIP_TRY(hipMemcpyAsync(a.bam->h_info, a.bam->dfl.info, 32, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(a.bam->h_sizes, a.bam->dfl.sizes, (size_t)a.bam->dfl.max_members * 4, hipMemcpyDeviceToHost, s));
            }
        } else if (p.mode == OutMode::CompactText) {
            HIP_TRY(hipMemcpyAsync(a.compact->h_coff + g0, w->coff.p, (size_t)nr * 8, hipMemcpyDeviceToHost, s));
            if (p.g1 == a.n_reads && a.compact->h_bytes > 0)       // the batch's last group: the front of the compact buffer
                HIP_TRY(hipMemcpyAsync(a.compact->h_ctext, a.compact->d_ctext, (size_t)a.compact->h_bytes, hipMemcpyDeviceToHost, s));
        } else {
            HIP_TRY(hipMemcpyAsync(a.h_out + a.h_out_off[g0], w->out.p, (size_t)p.out_bytes, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipMemcpyAsync(a.h_out_len + g0, w->out_len.p, (size_t)nr * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(a.h_status + g0, w->status.p, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(w->evc[3], s));
    }
    HIP_TRY(hipMemcpyAsync(w->h_cnt.p, w->counters.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(w->ev[5], s));
    return NPORE_OK;
}

// Reads [g0,g1): everything from the raw bytes to the gathered output, without host synchronisation.
// overlapping: another group of this context is on the device, most likely in its fill kernel, whose persistent
// workgroups hold nearly all the LDS and most of the vector registers of every CU until they have emptied their queue.
// beside_fill: ... and that fill launch left room on its CUs (launch_fill).  The preparation and gather kernels of THIS
// group then run in shapes that find room beside a fill workgroup instead of waiting for it to leave: 256-thread scans
// (one wave per SIMD), the LDS-free annotation (prep_kernels.hpp) and the gather without its LDS tile (kernels.hpp).
int run_group(npore_ctx *ctx, WorkSet *w, const AlignArgs &a, int64_t g0, int64_t g1, const OutTarget &ot, int shape, bool overlapping)
{
    const bool beside_fill = overlapping && ctx->fill_has_room;
    GroupPlan p;
    if (int rc = plan_group(a, g0, g1, p)) return rc;
    if (int rc = reserve_group(w, p, a)) return rc;
    OutTarget out = ot;
    const PrepParams pp = wire_group(ctx, w, p, a, out);
    w->staged = p.staged;
    if (p.staged)
        if (int rc = upload_group(ctx, w, p, a)) return rc;
    if (int rc = prep_group(ctx, w, p, pp, beside_fill)) return rc;
    if (int rc = fill_group(ctx, w, p, a, pp, shape, overlapping)) return rc;
    if (int rc = post_group(ctx, w, p, a, pp, out, beside_fill)) return rc;
    return download_group(ctx, w, p, a);
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
        HIP_TRY(hipEventRecord(ctx->ev_user, user));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_user, 0));
    }

    // groups of consecutive reads whose traceback words fit the budget.  The automatic budget is this context's
    // share of the device (contexts of one device run side by side: bench --inflight),
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
    AlignArgs a;
    a.n_reads = n_reads;
    a.h_ref_off = ref_off; a.h_seq_off = seq_off; a.h_cig_off = cig_off;
    a.indel_start = indel_start; a.indel_extend = indel_extend; a.max_b_rows = max_b_rows; a.r = r;
    a.h_out = out; a.h_out_off = out_off; a.h_out_len = out_len; a.h_status = status;
    return a;
}

}  // namespace
