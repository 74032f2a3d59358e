// tests/model/bam_walk.cpp -- TEST INFRASTRUCTURE.
// The product's BAM reader (npore_amd/csrc/bam_reader.hpp) built with plain g++, no GPU and no HIP header in reach: the
// one-pass record walker (BamRecordWalker over BamWindowSource, what npore_bam_realign_sequential feeds its batches from)
// beside selection on an indexed, resident handle (bam_select) of the same file.  Both answers are lists of offsets
// into the inflated stream; the CPU tests compare them.
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../npore_amd/csrc/bam_reader.hpp"

using namespace npore;

extern "C" {

const char *bam_walk_last_error(void) { return g_err.c_str(); }

// Offsets (of the block_size fields) of the records bam_select keeps on a resident handle.  Returns their number (the
// first `cap` are written), or a negative code.
int64_t bam_walk_select(const char *path, int n_regions, const int32_t *ref_id, const int64_t *start, const int64_t *stop,
                        int64_t max_reads, int64_t *out, int64_t cap)
try {
    std::unique_ptr<npore_bam> b(bam_open(path, 2, 1, nullptr));
    if (!b) return NPORE_E_INVALID;
    const int64_t n = bam_select(b.get(), n_regions, ref_id, start, stop, max_reads, nullptr, 0);
    if (n < 0) return n;
    std::vector<int64_t> idx((size_t)n + 1);
    if (bam_select(b.get(), n_regions, ref_id, start, stop, max_reads, idx.data(), n) != n) return fail(NPORE_E_INVALID, "select is not repeatable");
    for (int64_t k = 0; k < n && k < cap; k++) out[k] = b->rec_off[(size_t)idx[(size_t)k]];
    return n;
} catch (const std::exception &e) {
    return fail(NPORE_E_NOMEM, e.what());
}

// The same for the one-pass walk of process `rank` of `world` (world > 1: the share cuts come from the .bai at `bai`),
// in batches of `batch_reads`.  The walker hands out pointers into its windows; a record's offset is found by looking
// its BYTES up in the resident stream, front to back -- so a record that was carried from one window into the next and
// put together wrongly has no offset (the walk fails here).  The windows are NPORE_BAM_WINDOW_BLOCKS blocks long.
int64_t bam_walk_one_pass(const char *path, int n_regions, const int32_t *ref_id, const int64_t *start, const int64_t *stop,
                          int64_t max_reads, int rank, int world, const char *bai, int64_t batch_reads, int64_t *out, int64_t cap)
try {
    std::unique_ptr<npore_bam> b(bam_open(path, 2, 3, nullptr));
    if (!b) return NPORE_E_INVALID;
    if (int rc = bam_set_share(b.get(), rank, world, bai)) return rc;
    if (int rc = one_pass_args_check(b.get(), n_regions, ref_id, max_reads)) return rc;
    std::vector<const uint8_t *> recs;
    std::vector<std::shared_ptr<RawBuf>> keep;           // (every window of the walk: the files of the tests are small)
    {
        BamRecordWalker walker(b.get(), n_regions, ref_id, start, stop, max_reads, 2);
        RecFetch rf;
        for (;;) {
            const int64_t m = walker.next_batch(rf, keep, batch_reads);
            if (m < 0) return m;
            if (m == 0) break;
            if (m > batch_reads || m != (int64_t)rf.ptr.size()) return fail(NPORE_E_INVALID, "a batch of the wrong size");
            recs.insert(recs.end(), rf.ptr.begin(), rf.ptr.end());
        }
        if (walker.next_batch(rf, keep, batch_reads) != 0) return fail(NPORE_E_INVALID, "the walk goes on behind its end");
    }
    std::unique_ptr<npore_bam> res(bam_open(path, 2, 1, nullptr));
    if (!res) return NPORE_E_INVALID;
    size_t at = 0;
    for (size_t k = 0; k < recs.size(); k++) {
        const size_t len = 4 + (size_t)rdi32(recs[k]);
        for (;; at++) {
            if (at == res->rec_off.size()) return fail(NPORE_E_INVALID, "a record of the walk is not in the stream (or not in file order)");
            const size_t o = (size_t)res->rec_off[at];
            if (o + len <= res->data_size && std::memcmp(res->data + o, recs[k], len) == 0) break;
        }
        if ((int64_t)k < cap) out[k] = res->rec_off[at];
        at++;
    }
    return (int64_t)recs.size();
} catch (const std::exception &e) {
    return fail(NPORE_E_NOMEM, e.what());
}

// What bam_set_share decides for EVERY rank of `world` on one one-pass handle, without a walk: rc[rank] is its return
// code, span[2 * rank] / span[2 * rank + 1] the stretch it leaves in the handle (offsets into the inflated stream; -1:
// the end of the file).  Returns 0, or a negative code when the BAM itself does not open.
int bam_walk_shares(const char *path, const char *bai, int world, int32_t *rc, int64_t *span)
try {
    std::unique_ptr<npore_bam> b(bam_open(path, 2, 3, nullptr));
    if (!b) return NPORE_E_INVALID;
    for (int rank = 0; rank < world; rank++) {
        rc[rank] = bam_set_share(b.get(), rank, world, bai);
        span[2 * rank] = b->share_begin == UINT64_MAX ? -1 : (int64_t)b->share_begin;
        span[2 * rank + 1] = b->share_end == UINT64_MAX ? -1 : (int64_t)b->share_end;
        if (rc[rank] == NPORE_OK && !b->has_share) return fail(NPORE_E_INVALID, "a share that the handle does not have");
    }
    return 0;
} catch (const std::exception &e) {
    return fail(NPORE_E_NOMEM, e.what());
}

// has[k] = 1 where a one-pass handle on `path` says that contig k has reads (from the .bai beside the file, or, with
// none that it trusts, every contig).  Returns the number of contigs (the first `cap` are written), or a negative code.
int bam_walk_refs_with_reads(const char *path, uint8_t *has, int cap)
try {
    std::unique_ptr<npore_bam> b(bam_open(path, 2, 3, nullptr));
    if (!b) return NPORE_E_INVALID;
    for (int k = 0; k < (int)b->ref_has_reads.size() && k < cap; k++) has[k] = b->ref_has_reads[(size_t)k];
    return (int)b->ref_has_reads.size();
} catch (const std::exception &e) {
    return fail(NPORE_E_NOMEM, e.what());
}

}  // extern "C"
