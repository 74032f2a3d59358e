// bam_reader.hpp -- the BAM reader and the SAM writer of the BAM -> SAM pipeline, host side: opening a BAM (resident,
// streamed, header only), the record index and selection by region, the .bai share cuts, the one-pass window reader,
// record packing, SAM text.  Everything here parses untrusted files and none of it touches the GPU: this header and
// what it includes (hostio.hpp) compile with any C++17 compiler, no HIP header in reach.  The C ABI's entry points
// (npore_api.cpp) are thin wrappers around these bodies.
#pragma once
#include "../../include/npore_amd.h"
#include "hostio.hpp"
#include "deflate_code.hpp"
#include "cs_rec.hpp"
#include "eqx_rec.hpp"
#include "md_rec.hpp"
#include "nm_rec.hpp"
#include "oc_rec.hpp"

#include <sys/uio.h>

#include <cerrno>
#include <condition_variable>
#include <deque>
#include <map>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace npore {

// header of a BAM stream at d[0 .. N): text, references; *hdr_end = offset of the first record.  -1: more bytes needed
// (streamed mode reads on), 0: corrupt, 1: ok
inline int bam_parse_header(npore_bam *b, const uint8_t *d, size_t N, size_t *hdr_end)
{
    if (N < 12) return -1;
    if (std::memcmp(d, "BAM\1", 4) != 0) return 0;
    size_t p = 4;
    const int64_t l_text = rdi32(&d[p]);
    p += 4;
    if (l_text < 0) return 0;
    if (p + (size_t)l_text + 4 > N) return -1;
    b->text.assign(reinterpret_cast<const char *>(&d[p]), (size_t)l_text);
    while (!b->text.empty() && b->text.back() == '\0') b->text.pop_back();
    p += (size_t)l_text;
    const int32_t n_ref = rdi32(&d[p]);
    p += 4;
    if (n_ref < 0) return 0;
    b->ref_names.clear();
    b->ref_lens.clear();
    for (int32_t k = 0; k < n_ref; k++) {
        if (p + 4 > N) return -1;
        const int32_t l_name = rdi32(&d[p]);
        if (l_name < 1) return 0;
        if (p + 8 + (size_t)l_name > N) return -1;
        b->ref_names.emplace_back(reinterpret_cast<const char *>(&d[p + 4]), (size_t)l_name - 1);
        b->ref_lens.push_back(rdi32(&d[p + 4 + (size_t)l_name]));
        p += 8 + (size_t)l_name;
    }
    *hdr_end = p;
    return 1;
}

// the variable-length parts the record accessors will walk lie inside the record
inline bool record_is_sound(const uint8_t *q)
{
    const int32_t bs = rdi32(q);
    const uint8_t *f = q + 4;
    const int64_t l_rn = f[8], n_cig = rd16(f + 12), l_seq = rdi32(f + 16);
    return !(l_rn < 1 || l_seq < 0 || 32 + l_rn + 4 * n_cig + (l_seq + 1) / 2 + l_seq > bs || f[32 + l_rn - 1] != 0);
}

// The framing step of every walk over a record stream: is the record whose block_size field lies at d[p] whole within
// the N bytes at hand?  WHOLE: yes, the next record begins at `next`; MORE: its end (or its block_size field) lies
// beyond d[N) -- what that means is the caller's business (the end of a resident stream, a tail to carry into the next
// window); CORRUPT: a block_size smaller than the fixed fields.
enum class Frame { WHOLE, MORE, CORRUPT };
inline Frame frame_record(const uint8_t *d, size_t N, size_t p, size_t &next)
{
    if (p + 4 > N) return Frame::MORE;
    const int32_t bs = rdi32(d + p);
    if (bs < 32) return Frame::CORRUPT;
    if (p + 4 + (size_t)bs > N) return Frame::MORE;
    next = p + 4 + (size_t)bs;
    return Frame::WHOLE;
}

// what selection needs of the records in d[first record .. ): validation + metadata on all cores.  `offs` = offsets of
// the records' block_size fields relative to d; the metadata is appended to the handle's arrays.
inline bool bam_index_records(npore_bam *b, const uint8_t *d, const std::vector<int64_t> &offs, int64_t global_base, int threads)
{
    const int64_t n = (int64_t)offs.size(), at = (int64_t)b->rec_off.size();
    b->rec_off.resize((size_t)(at + n));
    b->m_ref.resize((size_t)(at + n));
    b->m_pos.resize((size_t)(at + n));
    b->m_span.resize((size_t)(at + n));
    b->m_flag.resize((size_t)(at + n));
    std::atomic<int> corrupt{0};
    const int64_t per = 256;
    parallel_for((n + per - 1) / per, threads, [&](int64_t blk) {
        for (int64_t i = blk * per; i < std::min(n, (blk + 1) * per); i++) {
            const uint8_t *q = d + offs[(size_t)i];
            if (!record_is_sound(q)) { corrupt++; return; }
            const RecView r = rec_view(q);
            const int64_t span = rec_ref_len(r);
            b->rec_off[(size_t)(at + i)] = global_base + offs[(size_t)i];
            b->m_ref[(size_t)(at + i)] = r.ref_id();
            b->m_pos[(size_t)(at + i)] = r.pos();
            b->m_span[(size_t)(at + i)] = (int32_t)std::min<int64_t>(span, INT32_MAX);
            b->m_flag[(size_t)(at + i)] = (uint16_t)r.flag();
        }
    });
    return corrupt == 0;
}

// per-reference record lists and the shortcuts of npore_bam_select, from the per-record metadata
inline void bam_finish_index(npore_bam *b)
{
    const int32_t n_ref = (int32_t)b->ref_names.size();
    b->ref_has_reads.assign((size_t)n_ref, 0);
    b->by_ref.assign((size_t)n_ref, {});
    b->ref_sorted.assign((size_t)n_ref, 1);
    b->ref_max_len.assign((size_t)n_ref, 0);
    std::vector<int64_t> last_pos((size_t)n_ref, -1);
    const int64_t n_rec = (int64_t)b->rec_off.size();
    for (int64_t i = 0; i < n_rec; i++) {
        const int32_t rid = b->m_ref[(size_t)i];
        if (rid >= 0 && rid < n_ref) {
            const int64_t pos = b->m_pos[(size_t)i];
            b->ref_has_reads[(size_t)rid] = 1;
            b->by_ref[(size_t)rid].push_back(i);
            if (pos < last_pos[(size_t)rid]) b->ref_sorted[(size_t)rid] = 0;
            last_pos[(size_t)rid] = pos;
            b->ref_max_len[(size_t)rid] = std::max<int64_t>(b->ref_max_len[(size_t)rid], b->m_span[(size_t)i]);
        }
    }
}

// STREAMED open: block table, then the stream in windows of `win_blocks` BGZF blocks (inflated on all cores, walked,
// dropped); a record that straddles two windows is carried over.  Resident: one window + 22 bytes per record.
inline npore_bam *bam_open_streamed(const char *path, int threads, std::unique_ptr<PreadFile> file, const char *index_path)
{
    std::unique_ptr<npore_bam> hold(new npore_bam());
    npore_bam *b = hold.get();
    b->streamed = true;
    b->file = std::move(file);
    uint64_t total = 0;
    if (!bgzf_scan(*b->file, b->blocks, total)) { fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BGZF file"); return nullptr; }
    b->data_size = (size_t)total;
    if (index_path && *index_path) {        // another process of this node has made the record index already
        MappedFile ix;
        const uint8_t *q = nullptr;
        if (ix.open(index_path) && ix.n >= 32 && std::memcmp(ix.p, "NPOREIX1", 8) == 0) q = ix.p;
        if (q) {
            uint64_t n_rec, hdr_len, tot;
            std::memcpy(&n_rec, q + 8, 8); std::memcpy(&hdr_len, q + 16, 8); std::memcpy(&tot, q + 24, 8);
            size_t hdr_end = 0;
            const size_t need = 32 + hdr_len + n_rec * 22;
            if (tot == total && ix.n >= need && bam_parse_header(b, q + 32, (size_t)hdr_len, &hdr_end) == 1) {
                const uint8_t *a = q + 32 + hdr_len;
                b->rec_off.resize(n_rec); b->m_ref.resize(n_rec); b->m_pos.resize(n_rec); b->m_span.resize(n_rec); b->m_flag.resize(n_rec);
                std::memcpy(b->rec_off.data(), a, n_rec * 8); a += n_rec * 8;
                std::memcpy(b->m_ref.data(), a, n_rec * 4); a += n_rec * 4;
                std::memcpy(b->m_pos.data(), a, n_rec * 4); a += n_rec * 4;
                std::memcpy(b->m_span.data(), a, n_rec * 4); a += n_rec * 4;
                std::memcpy(b->m_flag.data(), a, n_rec * 2);
                bam_finish_index(b);
                return hold.release();
            }
        }
        // (an unusable index file: fall through and index the file here)
    }
    size_t win_blocks = 4096;               // <= 256 MB of inflated stream per window
    if (const char *e = std::getenv("NPORE_BAM_WINDOW_BLOCKS")) win_blocks = (size_t)std::max(1, std::atoi(e));
    RawBuf win;
    std::vector<uint8_t> carry;             // the incomplete tail of the previous window
    uint64_t carry_at = 0;                  // stream offset of carry[0]
    bool have_header = false;
    std::vector<int64_t> offs;
    for (size_t b0 = 0; b0 < b->blocks.size();) {
        const size_t b1 = std::min(b->blocks.size(), b0 + win_blocks);
        const uint64_t w0 = b->blocks[b0].out_off, w1 = b->blocks[b1 - 1].out_off + b->blocks[b1 - 1].out_len;
        if (!win.ensure(carry.size() + (size_t)(w1 - w0) + 8)) { fail(NPORE_E_NOMEM, "BAM window"); return nullptr; }
        uint8_t *d = reinterpret_cast<uint8_t *>(win.p);
        if (!carry.empty()) std::memcpy(d, carry.data(), carry.size());
        if (!bgzf_inflate_range(*b->file, b->blocks, b0, b1, d + carry.size(), threads)) {
            fail(NPORE_E_INVALID, std::string("'") + path + "': corrupt BGZF block");
            return nullptr;
        }
        const uint64_t base = carry.empty() ? w0 : carry_at;      // stream offset of d[0]
        const size_t N = carry.size() + (size_t)(w1 - w0);
        size_t p = 0;
        if (!have_header) {
            size_t hdr_end = 0;
            const int rc = bam_parse_header(b, d, N, &hdr_end);
            if (rc == 0) { fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BAM file"); return nullptr; }
            if (rc < 0) {                                         // the header does not end in this window: read on
                if (b1 == b->blocks.size()) { fail(NPORE_E_INVALID, "truncated BAM header"); return nullptr; }
                carry.assign(d, d + N);
                carry_at = base;
                b0 = b1;
                continue;
            }
            have_header = true;
            p = hdr_end;
            b->first_record = base + hdr_end;
        }
        offs.clear();
        for (size_t nx = 0;; p = nx) {
            const Frame f = frame_record(d, N, p, nx);
            if (f == Frame::CORRUPT) { fail(NPORE_E_INVALID, "truncated BAM record"); return nullptr; }
            if (f == Frame::MORE) break;                          // the tail is carried into the next window
            offs.push_back((int64_t)p);
        }
        if (!bam_index_records(b, d, offs, (int64_t)base, threads)) { fail(NPORE_E_INVALID, "corrupt BAM record"); return nullptr; }
        carry.assign(d + p, d + N);
        carry_at = base + p;
        b0 = b1;
    }
    if (!have_header) { fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BAM file"); return nullptr; }
    if (!carry.empty()) { fail(NPORE_E_INVALID, "truncated BAM record"); return nullptr; }
    bam_finish_index(b);
    return hold.release();
}

// ONE-PASS open (mode 3): the BGZF block table and the BAM header, nothing else -- no record is looked at until
// npore_bam_realign_sequential walks the stream.  Such a handle has no record index: npore_bam_select finds nothing.
inline npore_bam *bam_open_header_only(const char *path, int threads, std::unique_ptr<PreadFile> file)
{
    std::unique_ptr<npore_bam> hold(new npore_bam());
    npore_bam *b = hold.get();
    b->streamed = true;
    b->file = std::move(file);
    uint64_t total = 0;
    if (!bgzf_scan(*b->file, b->blocks, total)) { fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BGZF file"); return nullptr; }
    b->data_size = (size_t)total;
    RawBuf head;
    for (size_t b1 = std::min<size_t>(b->blocks.size(), 16);; b1 = std::min(b->blocks.size(), b1 * 4)) {
        if (b1 == 0) { fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BAM file"); return nullptr; }
        const size_t n = (size_t)(b->blocks[b1 - 1].out_off + b->blocks[b1 - 1].out_len);
        if (!head.ensure(n + 8) || !bgzf_inflate_range(*b->file, b->blocks, 0, b1, reinterpret_cast<uint8_t *>(head.p), threads)) {
            fail(NPORE_E_INVALID, std::string("'") + path + "': corrupt BGZF block");
            return nullptr;
        }
        size_t hdr_end = 0;
        const int rc = bam_parse_header(b, reinterpret_cast<const uint8_t *>(head.p), n, &hdr_end);
        if (rc == 1) { b->first_record = hdr_end; break; }
        if (rc == 0 || b1 == b->blocks.size()) { fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BAM file"); return nullptr; }
    }
    bam_finish_index(b);                                 // (empty per-reference lists)
    // which contigs have reads (get_bam_regions' default keeps only those, src/util.py:16-93 with bam.count() > 0): from
    // the file's .bai when there is one (a reference with bins or linear-index entries has records) -- otherwise unknown
    // without a pass over the records: every contig is assumed to have some.  What the index says is a claim that the
    // one-pass walk checks against the records it meets (has_reads_index): a stale index ends the run, it drops nothing
    b->ref_has_reads.assign(b->ref_names.size(), 1);
    {
        const std::string p0 = std::string(path) + ".bai";
        std::string p1 = path;
        const size_t dot = p1.rfind('.');
        if (dot != std::string::npos) p1 = p1.substr(0, dot) + ".bai";
        std::vector<uint64_t> offs;
        std::vector<uint8_t> has;
        for (const std::string &cand : {p0, p1})
            if (bai_linear_offsets(cand.c_str(), offs, &has) && has.size() == b->ref_names.size()) { b->ref_has_reads = has; b->has_reads_index = cand; break; }
    }
    return hold.release();
}

// mode 0: automatic (streamed when the file is BGZF and larger than NPORE_BAM_STREAM_MB, default 1024 MB), 1: whole file
// resident, 2: streamed, 3: one-pass (header only; the reads through npore_bam_realign_sequential).  index_path (may be NULL): a record index saved by npore_bam_save_index for this very file --
// a streamed handle then skips its indexing pass (one process of a node indexes, the others load).
inline npore_bam *bam_open(const char *path, int threads, int mode, const char *index_path)
{
    if (!path) { fail(NPORE_E_INVALID, "null path"); return nullptr; }
    if (mode != 1) {
        std::unique_ptr<PreadFile> pf(new PreadFile());
        if (!pf->open(path)) { fail(NPORE_E_INVALID, std::string("BAM file '") + path + "' not found"); return nullptr; }
        uint8_t magic[4] = {0, 0, 0, 0};
        const bool gz = pf->size >= 28 && pf->read(0, magic, 4) && magic[0] == 31 && magic[1] == 139;
        uint64_t limit_mb = 1024;
        if (const char *e = std::getenv("NPORE_BAM_STREAM_MB")) limit_mb = (uint64_t)std::max(0ll, std::atoll(e));
        if (gz && mode == 3) return bam_open_header_only(path, threads, std::move(pf));
        if (mode == 3) { fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BGZF file (one-pass mode)"); return nullptr; }
        if (gz && (mode == 2 || pf->size > limit_mb * 1048576ull)) return bam_open_streamed(path, threads, std::move(pf), index_path);
        if (mode == 2) { fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BGZF file (streamed mode)"); return nullptr; }
    }
    std::unique_ptr<MappedFile> mfp(new MappedFile());
    MappedFile &mf = *mfp;
    if (!mf.open(path)) { fail(NPORE_E_INVALID, std::string("BAM file '") + path + "' not found"); return nullptr; }
    const ByteSpan raw{mf.p, mf.n};
    std::unique_ptr<npore_bam> hold(new npore_bam());
    npore_bam *b = hold.get();
    std::string err;
    if (mf.n >= 12 && std::memcmp(mf.p, "BAM\1", 4) == 0) {
        // an inflated BAM stream (npore_bam_dump_inflated: one rank of a node inflates, the others map its copy)
        b->data = mf.p;
        b->data_size = mf.n;
        b->raw_map = std::move(mfp);
    } else {
        if (!bgzf_inflate(raw, threads, b->data_buf, b->data_size, err) || b->data_size < 12 || std::memcmp(b->data_buf.p, "BAM\1", 4) != 0) {
            fail(NPORE_E_INVALID, std::string("'") + path + "' is not a BAM file" + (err.empty() ? "" : " (" + err + ")"));
            return nullptr;
        }
        b->data = reinterpret_cast<const uint8_t *>(b->data_buf.p);
    }
    const uint8_t *d = b->data;
    const size_t N = b->data_size;
    size_t p = 0;
    if (bam_parse_header(b, d, N, &p) != 1) { fail(NPORE_E_INVALID, "truncated BAM header"); return nullptr; }
    // records: offsets (one hop per record), then validation + metadata on all cores, then the per-reference lists
    std::vector<int64_t> offs;
    while (p + 4 <= N) {                                          // (fewer than four bytes behind the last record are let be)
        size_t nx = 0;
        if (frame_record(d, N, p, nx) != Frame::WHOLE) { fail(NPORE_E_INVALID, "truncated BAM record"); return nullptr; }
        offs.push_back((int64_t)p);
        p = nx;
    }
    if (!bam_index_records(b, d, offs, 0, threads)) { fail(NPORE_E_INVALID, "corrupt BAM record"); return nullptr; }
    bam_finish_index(b);
    return hold.release();
}

// The record index of a handle (header + per-record offsets and metadata: 22 bytes per record), complete or not there
// at all, for npore_bam_open_mode(..., index_path) in the other processes of a node.
inline int bam_save_index(const npore_bam *b, const char *path)
{
    if (!b || !path) return fail(NPORE_E_INVALID, "null argument");
    // the header as a BAM stream prefix, so that the loader parses it with the same code
    std::string hdr("BAM\1", 4);
    auto put32 = [&](int32_t v) { hdr.append(reinterpret_cast<const char *>(&v), 4); };
    put32((int32_t)b->text.size());
    hdr += b->text;
    put32((int32_t)b->ref_names.size());
    for (size_t k = 0; k < b->ref_names.size(); k++) {
        put32((int32_t)b->ref_names[k].size() + 1);
        hdr.append(b->ref_names[k].c_str(), b->ref_names[k].size() + 1);
        put32((int32_t)b->ref_lens[k]);
    }
    const std::string tmp = std::string(path) + ".tmp" + std::to_string((long long)::getpid());
    FILE *fh = std::fopen(tmp.c_str(), "wb");
    if (!fh) return fail(NPORE_E_INVALID, "cannot create '" + tmp + "'");
    const uint64_t n_rec = b->rec_off.size(), hdr_len = hdr.size(), tot = b->data_size;
    bool ok = std::fwrite("NPOREIX1", 1, 8, fh) == 8 && std::fwrite(&n_rec, 8, 1, fh) == 1 && std::fwrite(&hdr_len, 8, 1, fh) == 1 &&
              std::fwrite(&tot, 8, 1, fh) == 1 && std::fwrite(hdr.data(), 1, hdr.size(), fh) == hdr.size();
    auto put = [&](const void *p, size_t bytes) { if (ok && bytes) ok = std::fwrite(p, 1, bytes, fh) == bytes; };
    put(b->rec_off.data(), n_rec * 8); put(b->m_ref.data(), n_rec * 4); put(b->m_pos.data(), n_rec * 4);
    put(b->m_span.data(), n_rec * 4); put(b->m_flag.data(), n_rec * 2);
    if (std::fclose(fh) != 0 || !ok || std::rename(tmp.c_str(), path) != 0) {
        std::remove(tmp.c_str());
        return fail(NPORE_E_INVALID, std::string("cannot write '") + path + "'");
    }
    return NPORE_OK;
}

inline int bam_dump_inflated(const npore_bam *b, const char *path)
{
    if (!b || !path) return fail(NPORE_E_INVALID, "null argument");
    if (b->streamed) return fail(NPORE_E_UNSUPPORTED, "a streamed BAM handle holds no inflated stream (share its index: npore_bam_save_index)");
    const std::string tmp = std::string(path) + ".tmp" + std::to_string((long long)::getpid());
    FILE *fh = std::fopen(tmp.c_str(), "wb");
    if (!fh) return fail(NPORE_E_INVALID, "cannot create '" + tmp + "'");
    const bool ok = std::fwrite(b->data, 1, b->data_size, fh) == b->data_size;
    if (std::fclose(fh) != 0 || !ok || std::rename(tmp.c_str(), path) != 0) {       // complete, or not there at all
        std::remove(tmp.c_str());
        return fail(NPORE_E_INVALID, std::string("cannot write '") + path + "'");
    }
    return NPORE_OK;
}

inline int64_t bam_select(const npore_bam *b, int n_regions, const int32_t *ref_id, const int64_t *start, const int64_t *stop,
                          int64_t max_reads, int64_t *out_idx, int64_t cap, uint32_t drop_flags = PASS_FLAGS, uint32_t pass_mask = PASS_NONE)
{
    // pass_mask (staged_head.hpp): records with one of these flag bits are kept, to pass through; such a record without a
    // reference length (a placed, unmapped one has no CIGAR) overlaps as if its length were 1, as htslib has it
    drop_flags &= ~pass_mask;
    if (!b || (n_regions > 0 && (!ref_id || !start || !stop)) || (cap > 0 && !out_idx)) return fail(NPORE_E_INVALID, "null argument");
    int64_t kept = 0;
    for (int g = 0; g < n_regions; g++) {
        if (ref_id[g] < 0 || ref_id[g] >= (int32_t)b->by_ref.size()) continue;
        const std::vector<int64_t> &recs = b->by_ref[(size_t)ref_id[g]];     // file order
        size_t first = 0;
        if (b->ref_sorted[(size_t)ref_id[g]]) {
            // coordinate-sorted (the usual case): skip everything that ends before the region can start
            const int64_t lo = start[g] - b->ref_max_len[(size_t)ref_id[g]];
            first = (size_t)(std::lower_bound(recs.begin(), recs.end(), lo,
                                              [&](int64_t i, int64_t v) { return (int64_t)b->m_pos[(size_t)i] < v; }) - recs.begin());
        }
        for (size_t q = first; q < recs.size(); q++) {
            const int64_t i = recs[q];
            int64_t pos = b->m_pos[(size_t)i], rl = b->m_span[(size_t)i];
            if (rl == 0 && record_passes(b->m_flag[(size_t)i], pass_mask)) rl = 1;
            if (b->ref_sorted[(size_t)ref_id[g]] && pos >= stop[g]) break;
            if (!(pos < stop[g] && pos + rl > start[g])) continue;                 // overlaps [start, stop)
            if (max_reads > 0 && kept >= max_reads) return kept;                   // src/bam.pyx:29-30
            if (b->m_flag[(size_t)i] & drop_flags) continue;                      // secondary / supplementary / unmapped, :31-32
            if (kept < cap) out_idx[kept] = i;
            kept++;
        }
    }
    return kept;
}

// Does a record start at offset `abs` of the inflated stream, which lies in member `blk`?  What a cut of a share must
// be: the record there is framed WHOLE within the stream and sound, lies on a contig of the header (or on none) at a
// position within it, and behind it the stream ends or another such record follows.  Inflates `blk` and, where the two
// records reach further, the members behind it; a block_size that points beyond the stream's end inflates nothing more.
inline bool share_cut_is_record_start(const npore_bam *b, size_t blk, uint64_t abs)
{
    const uint64_t base = b->blocks[blk].out_off;
    std::vector<uint8_t> buf;
    size_t have = 0, b1 = blk;                               // members [blk, b1) inflated: buf[0 .. have) = stream[base ..)
    auto more = [&]() -> bool {                              // the next member that holds anything
        for (; b1 < b->blocks.size(); b1++) {
            const size_t len = (size_t)b->blocks[b1].out_len;
            if (!len) continue;
            buf.resize(have + len + 8);
            if (!bgzf_inflate_range(*b->file, b->blocks, b1, b1 + 1, buf.data() + have, 1)) return false;
            have += len;
            b1++;
            return true;
        }
        return false;
    };
    const int64_t n_ref = (int64_t)b->ref_names.size();
    auto record_at = [&](size_t p, size_t &next) -> bool {
        for (;;) {
            const Frame f = frame_record(buf.data(), have, p, next);
            if (f == Frame::WHOLE) break;
            if (f == Frame::CORRUPT) return false;
            if (p + 4 <= have && base + p + 4 + (uint64_t)rdi32(buf.data() + p) > b->data_size) return false;
            if (!more()) return false;
        }
        const uint8_t *q = buf.data() + p;
        if (!record_is_sound(q)) return false;
        const int64_t rid = rdi32(q + 4), pos = rdi32(q + 8);
        return rid >= -1 && rid < n_ref && (rid < 0 || (pos >= 0 && pos < b->ref_lens[(size_t)rid]));
    };
    size_t nx = 0, nx2 = 0;
    if (!more() || !record_at((size_t)(abs - base), nx)) return false;
    return base + nx == b->data_size || record_at(nx, nx2);
}

// ONE-PASS handle, several processes: the stretch of the record stream that `rank` of `world` walks (npore_bam.share_*).
// The index is another file and may be stale or somebody else's, so EVERY rank locates and checks ALL world + 1 cuts:
// whether the ranks walk shares or take the indexed reader depends on the two files and on `world`, never on `rank` --
// a rank that decided for itself would deal the reads differently from the rest (records twice, records missing).
inline int bam_set_share(npore_bam *b, int rank, int world, const char *bai_path)
{
    if (!b || world < 1 || rank < 0 || rank >= world) return fail(NPORE_E_INVALID, "bad argument");
    if (!b->file || b->blocks.empty()) return fail(NPORE_E_INVALID, "a share needs a handle opened on a BGZF file (modes 2 and 3)");
    b->has_share = false;
    b->share_begin = 0;
    b->share_end = UINT64_MAX;
    b->share_block = 0;
    if (world == 1) return NPORE_OK;
    std::vector<uint64_t> cuts;
    std::vector<uint8_t> has;
    if (!bai_path || !bai_linear_offsets(bai_path, cuts, &has) || has.size() != b->ref_names.size() || cuts.empty())
        return fail(NPORE_E_UNSUPPORTED, "no usable .bai linear index: the record stream cannot be dealt without a pass over it");
    const std::string foreign = std::string("the index '") + bai_path + "' does not belong to this BAM file (is it stale?)";
    // the first record of the stretch whose compressed offset lies at or behind k / world of the file
    const uint64_t c0 = b->blocks.front().in_off, c1 = b->blocks.back().in_off + b->blocks.back().in_len;
    auto cut_of = [&](int k) -> uint64_t {
        if (k <= 0) return 0;
        if (k >= world) return UINT64_MAX;
        const uint64_t target = c0 + (uint64_t)((long double)(c1 - c0) * k / world);
        auto it = std::lower_bound(cuts.begin(), cuts.end(), target << 16);
        return it == cuts.end() ? UINT64_MAX : *it;
    };
    // virtual offset -> block of the table and offset in the inflated stream (false: the index is not this file's): the
    // compressed half is where a member begins, exactly, the other half lies inside what that member inflates to
    auto locate = [&](uint64_t v, size_t &blk, uint64_t &abs) -> bool {
        const uint64_t coff = v >> 16, uoff = v & 0xFFFFu;
        auto it = std::lower_bound(b->blocks.begin(), b->blocks.end(), coff, [](const BgzfBlock &k, uint64_t c) { return k.mem_off < c; });
        if (it == b->blocks.end() || it->mem_off != coff || uoff >= it->out_len) return false;
        blk = (size_t)(it - b->blocks.begin());
        abs = it->out_off + uoff;
        return abs >= b->first_record;
    };
    // EVERY offset of the index lies in this file's block table (a search each, nothing inflated): the answer is then the
    // same at every `world`, also at one whose own cuts happen to be among the offsets that still fit
    size_t blk = 0;
    uint64_t abs = 0, seen = 0;                              // (neighbouring cuts are often the same entry: checked once)
    for (const uint64_t v : cuts)
        if (!locate(v, blk, abs)) return fail(NPORE_E_UNSUPPORTED, foreign);
    for (int k = 1; k < world; k++) {
        const uint64_t v = cut_of(k);
        if (v == UINT64_MAX) break;                          // nothing left from here on
        if (v != seen && (!locate(v, blk, abs) || !share_cut_is_record_start(b, blk, abs))) return fail(NPORE_E_UNSUPPORTED, foreign);
        seen = v;
        if (k == rank) { b->share_block = blk; b->share_begin = abs; }
        if (k == rank + 1) b->share_end = abs;
    }
    if (cut_of(rank) == UINT64_MAX) b->share_begin = b->share_end = UINT64_MAX;       // nothing left for this rank
    b->has_share = true;
    return NPORE_OK;
}

inline bool pack_args_ok(const npore_bam *b, const int64_t *idx, int64_t n)
{
    if (!b || n < 0 || (n > 0 && !idx)) return false;
    for (int64_t k = 0; k < n; k++)
        if (idx[k] < 0 || idx[k] >= (int64_t)b->rec_off.size()) return false;
    return true;
}

inline int fetch_records(const npore_bam *b, const int64_t *idx, int64_t n, int threads, RecFetch &rf)
{
    std::string err;
    if (!bam_fetch(*b, idx, n, threads, rf, err)) return fail(NPORE_E_INVALID, "BAM records: " + err);
    return NPORE_OK;
}
// pass_mask: a record that passes (staged_head.hpp) gives align() nothing -- its three slices are empty
inline void pack_sizes_of(const RecFetch &rf, int64_t n, int64_t *ref_off, int64_t *seq_off, int64_t *cig_off, int threads, uint32_t pass_mask)
{
    // per read (a 10 kb read has thousands of CIGAR operations: all cores), then the prefix sums
    ref_off[0] = seq_off[0] = cig_off[0] = 0;
    const int64_t per = 64;
    parallel_for((n + per - 1) / per, threads, [&](int64_t t) {
        for (int64_t k = t * per; k < std::min(n, (t + 1) * per); k++) {
            const RecView r = rec_of(rf, k);
            if (staged_passes(r.p, pass_mask)) { ref_off[k + 1] = seq_off[k + 1] = cig_off[k + 1] = 0; continue; }
            const RecCigar cg = rec_cigar(r);
            int64_t lead, trail, ops = 0, rl = 0;
            rec_clips(cg, lead, trail);
            for (uint32_t c = 0; c < cg.n; c++) {
                const uint32_t w = cg.op(c), op = w & 15u, len = w >> 4;
                if (op != 4 && op != 5) ops += len;
                if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += len;      // (rec_ref_len: M D N = X)
            }
            ref_off[k + 1] = rl;
            seq_off[k + 1] = std::max<int64_t>(0, (int64_t)r.l_seq() - lead - trail);
            cig_off[k + 1] = ops;
        }
    });
    for (int64_t k = 0; k < n; k++) { ref_off[k + 1] += ref_off[k]; seq_off[k + 1] += seq_off[k]; cig_off[k + 1] += cig_off[k]; }
}

inline int pack_records(const npore_bam *b, const RecFetch &rf, const npore_fasta *fa, const int32_t *fasta_of_ref, int64_t n,
                 uint8_t *refs, const int64_t *ref_off, uint8_t *seqs, const int64_t *seq_off, char *cigs,
                 const int64_t *cig_off, int threads, bool for_upload, uint32_t pass_mask)
{
    std::atomic<int> bad{0};
    parallel_for(n, threads, [&](int64_t k) {
        const RecView r = rec_of(rf, k);
        const int32_t rid = r.ref_id();
        const int fi = (rid >= 0 && rid < (int32_t)b->ref_names.size()) ? fasta_of_ref[rid] : -1;
        if (fi < 0 || fi >= (int)fa->names.size()) { bad++; return; }
        if (staged_passes(r.p, pass_mask)) return;      // (its slices are empty: pack_sizes_of)
        // reference bases: FASTA slice [pos, pos + reference_length), what pysam rebuilds from MD (src/bam.pyx:45)
        const char *ctg = fa->seq((size_t)fi);
        const int64_t ctg_len = fa->len((size_t)fi);
        const int64_t rl = ref_off[k + 1] - ref_off[k], pos = r.pos();
        uint8_t *ro = refs + ref_off[k];
        {
            const int64_t q0 = std::min(rl, std::max<int64_t>(0, -pos)), q1 = std::max(q0, std::min(rl, ctg_len - pos));
            std::memset(ro, 0, (size_t)q0);
            base_codes(ctg + pos + q0, ro + q0, q1 - q0);
            std::memset(ro + q1, 0, (size_t)(rl - q1));
        }
        // query bases without the soft clips (src/bam.pyx:42)
        const RecCigar cg = rec_cigar(r);
        int64_t lead, trail;
        rec_clips(cg, lead, trail);
        uint8_t *so = seqs + seq_off[k];
        const int64_t sl = seq_off[k + 1] - seq_off[k];
        nibble_codes(r.seq(), lead, so, sl);
        // expanded CIGAR without S and H (src/bam.pyx:59)
        char *co = cigs + cig_off[k];
        for (uint32_t c = 0; c < cg.n; c++) {
            const uint32_t w = cg.op(c), op = w & 15u, len = w >> 4;
            if (op == 4 || op == 5) continue;
            const char ch = op < 10 ? CIGOPS[op] : '?';
            if (len <= 8) { for (uint32_t q = 0; q < len; q++) co[q] = ch; }      // (most runs are a few ops long)
            else std::memset(co, ch, len);
            co += len;
        }
        if (for_upload) {       // page-locked staging about to cross PCIe: out of this core's cache first (hostio.hpp)
            cache_writeback(ro, (size_t)rl);
            cache_writeback(so, (size_t)sl);
            cache_writeback(cigs + cig_off[k], (size_t)(cig_off[k + 1] - cig_off[k]));
        }
    });
    return bad ? fail(NPORE_E_INVALID, "a selected read lies on a contig that is not in the FASTA") : NPORE_OK;
}

#if defined(__x86_64__)
// "=ACMGRSVTWYHKDBN"[nibble] for 16 packed bytes at a time (high nibble first); returns the packed bytes done (a multiple of 16)
__attribute__((target("ssse3"))) inline int64_t nibbles_to_text_ssse3(const uint8_t *src, char *dst, int64_t n_bytes)
{
    const __m128i lut = _mm_loadu_si128(reinterpret_cast<const __m128i *>(SEQ16));
    const __m128i low = _mm_set1_epi8(0x0F);
    int64_t j = 0;
    for (; j + 16 <= n_bytes; j += 16) {
        const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + j));
        const __m128i hi = _mm_shuffle_epi8(lut, _mm_and_si128(_mm_srli_epi16(v, 4), low));
        const __m128i lo = _mm_shuffle_epi8(lut, _mm_and_si128(v, low));
        _mm_storeu_si128(reinterpret_cast<__m128i *>(dst + 2 * j), _mm_unpacklo_epi8(hi, lo));
        _mm_storeu_si128(reinterpret_cast<__m128i *>(dst + 2 * j + 16), _mm_unpackhi_epi8(hi, lo));
    }
    return j;
}
#endif

inline int format_sam_into(const npore_bam *b, const RecFetch &rf, int64_t n, const char *finals, const int64_t *final_off,
                    const int64_t *final_len, const int32_t *status, int threads, RawBuf &out, int64_t *sam_len)
{
    if (!b || n < 0 || !sam_len || (n > 0 && (!finals || !final_off || !final_len || !status)))
        return fail(NPORE_E_INVALID, "bad argument");
    // pass 1: line sizes; pass 2: fill (both parallel over reads)
    std::vector<int64_t> off((size_t)n + 1, 0);
    // decimal text of v at dst (dst == nullptr: only the length), no terminator
    auto put_int = [](char *dst, long long v) -> int {
        char tmp[24];
        int nd = 0;
        unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        do { tmp[nd++] = (char)('0' + u % 10); u /= 10; } while (u);
        const int neg = v < 0;
        if (dst) {
            if (neg) *dst++ = '-';
            for (int q = 0; q < nd; q++) dst[q] = tmp[nd - 1 - q];
        }
        return nd + neg;
    };
#if defined(__x86_64__)
    static const bool have_ssse3 = __builtin_cpu_supports("ssse3");
#endif
    static const struct PairTab {      // two bases of the 4-bit packed sequence per lookup
        uint16_t pair[256];
        PairTab() { for (int v = 0; v < 256; v++) pair[v] = (uint16_t)((uint8_t)SEQ16[v >> 4] | ((uint8_t)SEQ16[v & 15] << 8)); }
    } seqtab;
    auto line = [&](int64_t k, char *dst) -> int64_t {    // returns the length; writes when dst != nullptr
        if (status[k] & NPORE_ST_BAD_INPUT) return 0;    // refused reads are not written
        const RecView r = rec_of(rf, k);
        const RecCigar cg = rec_cigar(r);
        int64_t lead, trail;
        rec_clips(cg, lead, trail);
        const int64_t sl = std::max<int64_t>(0, (int64_t)r.l_seq() - lead - trail);
        const int32_t rid = r.ref_id();
        const std::string &rn = (rid >= 0 && rid < (int32_t)b->ref_names.size()) ? b->ref_names[(size_t)rid] : std::string("*");
        const bool noq = r.l_seq() == 0 || r.qual()[0] == 0xFF;
        const size_t nl = std::strlen(r.name());
        const long long flag = r.flag(), pos1 = (long long)r.pos() + 1, mapq = r.mapq(), hp = (long long)rec_hp(r),
                        reflen = (long long)rec_ref_len(cg);
        if (!dst)       // name \t flag \t rname \t pos \t mapq \t cigar \t * \t 0 \t tlen \t seq \t qual \t HP:i:n \n
            return (int64_t)nl + 1 + put_int(nullptr, flag) + 1 + (int64_t)rn.size() + 1 + put_int(nullptr, pos1) + 1 +
                   put_int(nullptr, mapq) + 1 + final_len[k] + 5 + put_int(nullptr, reflen) + 1 + sl + 1 + (noq ? 1 : sl) + 6 +
                   put_int(nullptr, hp) + 1;
        char *o = dst;
        std::memcpy(o, r.name(), nl); o += nl;
        *o++ = '\t'; o += put_int(o, flag); *o++ = '\t';
        std::memcpy(o, rn.data(), rn.size()); o += rn.size();
        *o++ = '\t'; o += put_int(o, pos1); *o++ = '\t'; o += put_int(o, mapq); *o++ = '\t';
        std::memcpy(o, finals + final_off[k], (size_t)final_len[k]); o += final_len[k];
        std::memcpy(o, "\t*\t0\t", 5); o += 5;
        o += put_int(o, reflen); *o++ = '\t';
        {
            const uint8_t *sq = r.seq();
            int64_t q = 0, t = lead;
            if (q < sl && (t & 1)) { o[q++] = SEQ16[sq[t >> 1] & 15]; t++; }
            const uint8_t *src = sq + (t >> 1);
            const int64_t pairs = (sl - q) >> 1;
            char *po = o + q;
            int64_t j = 0;
#if defined(__x86_64__)
            if (have_ssse3) j = nibbles_to_text_ssse3(src, po, pairs);          // 16 packed bytes -> 32 letters per step
#endif
            for (; j < pairs; j++) { const uint16_t v = seqtab.pair[src[j]]; std::memcpy(po + 2 * j, &v, 2); }
            q += 2 * pairs;
            if (q < sl) { o[q] = SEQ16[src[pairs] >> 4]; q++; }
            o += sl;
        }
        *o++ = '\t';
        if (noq) *o++ = '*';
        else {
            const uint8_t *__restrict ql = r.qual() + lead;
            char *__restrict qo = o;
            for (int64_t q = 0; q < sl; q++) qo[q] = (char)(33 + ql[q]);
            o += sl;
        }
        std::memcpy(o, "\tHP:i:", 6); o += 6;
        o += put_int(o, hp); *o++ = '\n';
        return (int64_t)(o - dst);
    };
    parallel_for(n, threads, [&](int64_t k) { off[(size_t)k + 1] = line(k, nullptr); });
    for (int64_t k = 0; k < n; k++) off[(size_t)k + 1] += off[(size_t)k];
    if (!out.ensure((size_t)off[(size_t)n] + 1)) return fail(NPORE_E_NOMEM, "SAM text buffer");
    parallel_for(n, threads, [&](int64_t k) { if (off[(size_t)k + 1] > off[(size_t)k]) line(k, out.p + off[(size_t)k]); });
    *sam_len = off[(size_t)n];
    return NPORE_OK;
}

// ---- BAM out: records and file, stated once -----------------------------------------------------------------------
// RECORD.  One per read that format_sam_into would write (reads with NPORE_ST_BAD_INPUT are left out), carrying what
// the SAM line of src/bam.pyx:83 carries:
//   block_size | refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen | read_name\0 |
//   CIGAR words | 4-bit bases | qualities | the HP tag
//   - refID, pos, mapq, flag and the name are the input record's; bin = reg2bin(pos, pos + max(1, reflen)), reflen the
//     input record's reference length;
//   - the CIGAR words `len << 4 | op` are the final standardised CIGAR (M / I / D, no clips);
//   - l_seq counts the bases without the soft clips; the 4-bit bases are the input's from the leading clip on (an odd
//     clip moves every nibble), the low nibble of an odd last byte is 0; the qualities are the same slice, a read
//     without qualities (first byte 0xFF) gets 0xFF x l_seq;
//   - next_refID = next_pos = -1 (SAM's `*` and `0`), tlen = reflen (SAM's `stop - start`);
//   - one tag, HP, as the smallest integer type that holds it in htslib's order: C, S, I from 0 up, c, s, i below; 0 when
//     the input has none.
//   A record's size is 36 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq + 3 + {1, 2, 4}.
//   - a final CIGAR of n > 65 535 operations does not fit n_cigar_op; it is written as htslib writes it (SAM specification
//     4.2.2): n_cigar_op = 2, the CIGAR field holds the placeholder `l_seq << 4 | 4`, `reflen << 4 | 3`, and a second tag
//     BEHIND HP carries the words: 'C' 'G' 'B' 'I', the 32-bit count n, the n words.  Size: 36 + l_read_name + 8 +
//     (l_seq + 1) / 2 + l_seq + 3 + {1, 2, 4} + 8 + 4 * n.  bin, tlen and the index entry come from the real reference
//     length as always.  (The input side of the same rule: hostio.hpp rec_cigar.)
// FULL RECORD (NPORE_OUT_FULL, `--records full`; RECORD above stays the default and its bytes do not change).  The input
//   record with only what the realignment changes replaced:
//   - refID, pos, mapq, flag, the name, l_seq, next_refID, next_pos and tlen are the input's; bin as above;
//   - the 4-bit bases and the qualities are the input's, whole: clips included, no nibble moves, copied verbatim (a
//     leading 0xFF included);
//   - the CIGAR is the input's leading clip words, the final standardised CIGAR, the input's trailing clip words, not
//     merged.  The clip words are those of the record's real CIGAR (rec_cigar).  Lead: word 0 if it is H, then the next
//     word if it is S; trail: the mirror image at the end, over the words the lead left (full_clip_words) -- rec_clips'
//     recognition plus the H words it steps over; an H with no S beside it is kept too;
//   - the tags are the input's aux bytes in input order minus NM MD cs de dv CG (hostio.hpp filter_aux); HP stays where
//     and as it was, none is made when the input has none;
//   - a recomputed NM (nm_rec.hpp) follows them as the smallest unsigned type: C, S, I (bam_hp_tag_bytes);
//   - with NPORE_OUT_MD (`--md`) the MD tag (md_rec.hpp) follows NM: 'M' 'D' 'Z', the text, NUL -- 4 + its length bytes.  It is
//     `samtools calmd`'s text but for what NM already differs in: an IUPAC letter other than N counts as a mismatch and
//     prints as N.  Without the flag no MD is written (the input's is stale and dropped);
//   - more than 65 535 operations, clips included: the CIGAR field holds the placeholder `l_seq << 4 | 4`,
//     `reflen << 4 | 3` with the full l_seq, and CG:B,I with ALL the words goes behind NM (behind MD where there is one:
//     kept aux, NM, MD, CG).
//   - with NPORE_TAG_CS / NPORE_TAG_DE (`--cs`, `--de`, npore_bam_set_output_tags) cs and de (cs_rec.hpp) follow MD: 'c' 's' 'Z',
//     the text, NUL -- 4 + its length bytes -- and 'd' 'e' 'f' and a float -- 7 bytes: kept aux, NM, MD, cs, de, CG.  They are
//     minimap2's but for what NM already differs in: an IUPAC letter other than N counts as a mismatch.
//   - with NPORE_CIGAR_EQX (`--eqx`, the same setter's word) the final standardised CIGAR stands between the clip words in its
//     =/X form (eqx_rec.hpp): every compared position = or X by NM's predicate, run-length coded through neighbouring compared
//     words.  n_cigar counts the split words, so the placeholder + CG form begins several times sooner; the tags do not change.
//   - with NPORE_TAG_OC (`--oc`, the same setter's word) a read whose alignment CHANGED (oc_rec.hpp: the canonical M form of its
//     input CIGAR between the clip words is not its final CIGAR) carries its input's real CIGAR as OC:Z behind de: kept aux, NM,
//     MD, cs, de, OC, CG.  The kept aux then leaves an input's OC out as well, so an unchanged read has none.
//   Size: 36 + l_read_name + 4 * n_cigar (8 when long) + (l_seq + 1) / 2 + l_seq + kept aux + 3 + {1, 2, 4} (+ 4 + MD text)
//   (+ 8 + 4 * n when long).
// FILE.  BGZF with STORED deflate members (level 0, what `samtools view -u` writes): 18 bytes of gzip header with the BC
//   field, one stored block (01 LEN NLEN), the payload, CRC-32 and ISIZE -- payload + 31 bytes.  The header (text +
//   reference list) lies in members of its own; the record stream is cut every 65 280 payload bytes counted from the
//   first record of the file (or of a rank's part), whatever the batches were; the 28-byte EOF member ends the file.
// INDEX.  <out>.bam.bai from the same pass: per reference the bins with their chunks (neighbouring records of a bin
//   merged into one chunk), and the 16 kb linear index with empty windows filled forward -- from (refID, pos, reflen,
//   record bytes) and the virtual offsets the framing implies.  Written only when the records came in coordinate order.
constexpr size_t BGZF_STORED_PAYLOAD = 0xFF00, BGZF_STORED_OVERHEAD = 31;
static const uint8_t BGZF_EOF_MEMBER[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

inline uint32_t bam_reg2bin(int64_t beg, int64_t end)      // SAM specification 5.3
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
inline int bam_hp_tag_bytes(int64_t hp)      // the value's bytes (type letter: bam_record_into)
{
    if (hp >= 0) return hp <= 0xFF ? 1 : hp <= 0xFFFF ? 2 : 4;
    return hp >= -128 ? 1 : hp >= -32768 ? 2 : 4;
}
// operations of a collapsed CIGAR text ("12M3I..."); -1: not such a text
inline int64_t cigar_text_ops(const char *t, int64_t n)
{
    int64_t ops = 0;
    bool digits = false;
    for (int64_t q = 0; q < n; q++) {
        if (t[q] >= '0' && t[q] <= '9') digits = true;
        else { if (!digits) return -1; digits = false; ops++; }
    }
    return digits ? -1 : ops;
}
// The BAM record of read `r` with its final CIGAR text: its size (dst == nullptr) or its bytes at dst; 0 = the read is
// not written, < 0 = it cannot be (a final text that is no CIGAR).  `meta`: what the index needs.
inline int64_t bam_record_into(const RecView &r, const char *final_text, int64_t final_len, int32_t status, uint8_t *dst,
                               BamRecMeta *meta = nullptr)
{
    if (status & NPORE_ST_BAD_INPUT) return 0;
    const RecCigar in_cg = rec_cigar(r);
    int64_t lead, trail;
    rec_clips(in_cg, lead, trail);
    const int64_t sl = std::max<int64_t>(0, (int64_t)r.l_seq() - lead - trail);
    const int64_t n_cig = cigar_text_ops(final_text, final_len);
    if (n_cig < 0) return -1;
    const bool lng = n_cig > 0xFFFF;                 // placeholder + CG tag
    const int64_t hp = rec_hp(r);
    const int l_rn = r.l_read_name(), hb = bam_hp_tag_bytes(hp);
    const int64_t size = 36 + l_rn + 4 * n_cig + (sl + 1) / 2 + sl + 3 + hb + (lng ? 16 : 0);
    if (!dst) return size;
    const int64_t reflen = rec_ref_len(in_cg);
    auto w32 = [](uint8_t *o, uint32_t v) { std::memcpy(o, &v, 4); };
    auto w16 = [](uint8_t *o, uint16_t v) { std::memcpy(o, &v, 2); };
    uint8_t *o = dst;
    w32(o, (uint32_t)(size - 4));
    w32(o + 4, (uint32_t)r.ref_id());
    w32(o + 8, (uint32_t)r.pos());
    o[12] = (uint8_t)l_rn;
    o[13] = (uint8_t)r.mapq();
    w16(o + 14, (uint16_t)bam_reg2bin(r.pos(), (int64_t)r.pos() + std::max<int64_t>(1, reflen)));
    w16(o + 16, (uint16_t)(lng ? 2 : n_cig));
    w16(o + 18, (uint16_t)r.flag());
    w32(o + 20, (uint32_t)sl);
    w32(o + 24, 0xFFFFFFFFu);
    w32(o + 28, 0xFFFFFFFFu);
    w32(o + 32, (uint32_t)reflen);
    o += 36;
    std::memcpy(o, r.name(), (size_t)l_rn);
    o += l_rn;
    uint8_t *const seq_at = lng ? o + 8 : o + 4 * n_cig;
    if (lng) {                                       // the words go behind HP
        w32(o, (uint32_t)sl << 4 | 4u);
        w32(o + 4, (uint32_t)reflen << 4 | 3u);
        o = seq_at + (sl + 1) / 2 + sl + 3 + hb;
        std::memcpy(o, "CGBI", 4);
        w32(o + 4, (uint32_t)n_cig);
        o += 8;
    }
    {
        uint32_t len = 0;
        for (int64_t q = 0; q < final_len; q++) {
            const char c = final_text[q];
            if (c >= '0' && c <= '9') { len = len * 10 + (uint32_t)(c - '0'); continue; }
            const uint32_t op = c == 'M' ? 0 : c == 'I' ? 1 : c == 'D' ? 2 : c == 'N' ? 3 : c == 'S' ? 4 : c == 'H' ? 5 : c == 'P' ? 6 : c == '=' ? 7 : 8;
            w32(o, len << 4 | op);
            o += 4;
            len = 0;
        }
    }
    o = seq_at;
    {
        const uint8_t *sq = r.seq() + (lead >> 1);
        const int64_t nb = (sl + 1) / 2;
        if (!(lead & 1)) std::memcpy(o, sq, (size_t)nb);
        else for (int64_t j = 0; j < nb; j++) o[j] = (uint8_t)(sq[j] << 4 | sq[j + 1] >> 4);      // (sq[nb] is a byte of the record: the trailing clip or the qualities)
        if (sl & 1) o[nb - 1] &= 0xF0;
        o += nb;
    }
    if (r.l_seq() == 0 || r.qual()[0] == 0xFF) std::memset(o, 0xFF, (size_t)sl);
    else std::memcpy(o, r.qual() + lead, (size_t)sl);
    o += sl;
    o[0] = 'H'; o[1] = 'P';
    o[2] = (uint8_t)(hp >= 0 ? (hb == 1 ? 'C' : hb == 2 ? 'S' : 'I') : (hb == 1 ? 'c' : hb == 2 ? 's' : 'i'));
    { const uint32_t v = (uint32_t)(int32_t)hp; std::memcpy(o + 3, &v, (size_t)hb); }
    if (meta) *meta = BamRecMeta{r.ref_id(), r.pos(), reflen, size};
    return size;
}

// FULL RECORD's clip words of a real CIGAR: the lead is words [0, i), the trail words [j, n)
inline void full_clip_words(const RecCigar &cg, uint32_t &i, uint32_t &j)
{
    i = 0;
    j = cg.n;
    if (i < j && (cg.op(i) & 15u) == 5) i++;
    if (i < j && (cg.op(i) & 15u) == 4) i++;
    if (j > i && (cg.op(j - 1) & 15u) == 5) j--;
    if (j > i && (cg.op(j - 1) & 15u) == 4) j--;
}
inline uint32_t cigar_op_code(char c)
{
    return c == 'M' ? 0 : c == 'I' ? 1 : c == 'D' ? 2 : c == 'N' ? 3 : c == 'S' ? 4 : c == 'H' ? 5 : c == 'P' ? 6 : c == '=' ? 7 : 8;
}
// the words `len << 4 | op` of a final CIGAR text of `ops` operations (cigar_text_ops)
inline std::vector<uint8_t> cigar_text_words(const char *t, int64_t n, int64_t ops)
{
    std::vector<uint8_t> words((size_t)ops * 4 + 4);
    uint32_t len = 0;
    uint8_t *o = words.data();
    for (int64_t q = 0; q < n; q++) {
        if (t[q] >= '0' && t[q] <= '9') { len = len * 10 + (uint32_t)(t[q] - '0'); continue; }
        const uint32_t w = len << 4 | cigar_op_code(t[q]);
        std::memcpy(o, &w, 4);
        o += 4;
        len = 0;
    }
    return words;
}
// NM (nm_rec.hpp) of a final CIGAR text over the read's code arrays; -1: no CIGAR text
inline int64_t nm_of_text(const char *t, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl)
{
    const int64_t ops = cigar_text_ops(t, n);
    if (ops < 0) return -1;
    return nm_of_words(cigar_text_words(t, n, ops).data(), ops, ref, rl, seq, sl);
}
// MD (md_rec.hpp) of a final CIGAR's `ops` words over the read's code arrays, sized and then written
inline void md_of_words(const uint8_t *w, int64_t ops, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl, std::string &md)
{
    md.assign((size_t)md_size_of_words(w, ops, ref, rl, seq, sl), '\0');
    md_into_words(w, ops, ref, rl, seq, sl, reinterpret_cast<uint8_t *>(&md[0]), (int64_t)md.size());
}
// the bytes of the cs and de tags (NPORE_TAG_*; cs_rec.hpp) of the same as they follow MD in a FULL record: cs sized and then
// written, de from the size pass's counts
inline void cs_de_tags_of_words(int tags, const uint8_t *w, int64_t ops, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl, std::string &out)
{
    out.clear();
    if (tags & NPORE_TAG_CS) {
        const bool lng = (tags & NPORE_TAG_CS_LONG) != 0;
        const int64_t size = cs_size_of_words(w, ops, ref, rl, seq, sl, lng);
        out.assign("csZ").append((size_t)size + 1, '\0');
        cs_into_words(w, ops, ref, rl, seq, sl, lng, reinterpret_cast<uint8_t *>(&out[3]), size);
    }
    if (tags & NPORE_TAG_DE) {
        CsCounts c;
        cs_size_of_words(w, ops, ref, rl, seq, sl, false, &c);
        const float de = de_of_counts(c.e, c.x, c.g);
        char v[4];
        std::memcpy(v, &de, 4);
        out.append("def").append(v, 4);
    }
}
// bam_record_into's twin for the FULL RECORD over the final CIGAR's n_fin words (< 0: the text was no CIGAR); nm: the read's NM
// (nm_of_words); md: its MD text (md_of_words), or none; more: the bytes of its cs, de and OC tags (cs_de_tags_of_words,
// oc_tag_of_words), or none; drop_oc: filter_aux's -- the run writes OC (RecSpec::oc())
inline int64_t bam_record_full_words_into(const RecView &r, const uint8_t *fin_words, int64_t n_fin, int32_t status, int64_t nm, uint8_t *dst,
                                          BamRecMeta *meta = nullptr, const std::string *md = nullptr, const std::string *more = nullptr,
                                          bool drop_oc = false)
{
    if (status & NPORE_ST_BAD_INPUT) return 0;
    const RecCigar in_cg = rec_cigar(r);
    if (n_fin < 0 || nm < 0) return -1;
    uint32_t ci, cj;
    full_clip_words(in_cg, ci, cj);
    const int64_t n_cig = (int64_t)ci + n_fin + (int64_t)(in_cg.n - cj);
    const bool lng = n_cig > 0xFFFF;
    const int64_t l_seq = r.l_seq(), nb = (l_seq + 1) / 2, aux = filter_aux(r.aux(), r.end(), nullptr, drop_oc);
    const int l_rn = r.l_read_name(), nmb = bam_hp_tag_bytes(nm);
    const int64_t mdb = (md ? 4 + (int64_t)md->size() : 0) + (more ? (int64_t)more->size() : 0);      // (MD, cs, de, OC)
    const int64_t size = 36 + l_rn + (lng ? 8 : 4 * n_cig) + nb + l_seq + aux + 3 + nmb + mdb + (lng ? 8 + 4 * n_cig : 0);
    if (!dst) return size;
    const int64_t reflen = rec_ref_len(in_cg);
    auto w32 = [](uint8_t *o, uint32_t v) { std::memcpy(o, &v, 4); };
    auto w16 = [](uint8_t *o, uint16_t v) { std::memcpy(o, &v, 2); };
    uint8_t *o = dst;
    w32(o, (uint32_t)(size - 4));
    std::memcpy(o + 4, r.p, 32);                     // the input's fixed fields; bin and n_cigar_op are this record's
    w16(o + 14, (uint16_t)bam_reg2bin(r.pos(), (int64_t)r.pos() + std::max<int64_t>(1, reflen)));
    w16(o + 16, (uint16_t)(lng ? 2 : n_cig));
    o += 36;
    std::memcpy(o, r.name(), (size_t)l_rn);
    o += l_rn;
    uint8_t *const seq_at = lng ? o + 8 : o + 4 * n_cig;
    if (lng) {                                       // the words go behind NM (and MD, cs, de)
        w32(o, (uint32_t)l_seq << 4 | 4u);
        w32(o + 4, (uint32_t)reflen << 4 | 3u);
        o = seq_at + nb + l_seq + aux + 3 + nmb + mdb;
        std::memcpy(o, "CGBI", 4);
        w32(o + 4, (uint32_t)n_cig);
        o += 8;
    }
    std::memcpy(o, in_cg.w, 4 * (size_t)ci);
    o += 4 * (size_t)ci;
    std::memcpy(o, fin_words, 4 * (size_t)n_fin);
    o += 4 * (size_t)n_fin;
    std::memcpy(o, in_cg.w + 4 * (size_t)cj, 4 * (size_t)(in_cg.n - cj));
    o = seq_at;
    std::memcpy(o, r.seq(), (size_t)(nb + l_seq));
    o += nb + l_seq;
    filter_aux(r.aux(), r.end(), o, drop_oc);
    o += aux;
    o[0] = 'N'; o[1] = 'M';
    o[2] = (uint8_t)(nmb == 1 ? 'C' : nmb == 2 ? 'S' : 'I');
    { const uint32_t v = (uint32_t)nm; std::memcpy(o + 3, &v, (size_t)nmb); }
    o += 3 + nmb;
    if (md) {
        std::memcpy(o, "MDZ", 3);
        std::memcpy(o + 3, md->c_str(), md->size() + 1);
        o += 4 + md->size();
    }
    if (more) std::memcpy(o, more->data(), more->size());
    if (meta) *meta = BamRecMeta{r.ref_id(), r.pos(), reflen, size};
    return size;
}
// ... of a single read's final CIGAR TEXT (one tag or one record is wanted: the sanitizer programs; a batch goes through
// format_bam_into, which parses each text once)
inline int64_t bam_record_full_into(const RecView &r, const char *final_text, int64_t final_len, int32_t status, int64_t nm, uint8_t *dst)
{
    const int64_t n_fin = cigar_text_ops(final_text, final_len);
    if ((status & NPORE_ST_BAD_INPUT) || n_fin < 0) return (status & NPORE_ST_BAD_INPUT) ? 0 : -1;
    return bam_record_full_words_into(r, cigar_text_words(final_text, final_len, n_fin).data(), n_fin, status, nm, dst);
}
// The records a batch writes (rec), and for FULL records the code arrays of its reads (what align() got): NM is counted from
// them, MD and cs / de written from them; the slices of a record that passes are empty
struct ReadCodes {
    RecSpec rec;
    const uint8_t *refs = nullptr; const int64_t *ref_off = nullptr;
    const uint8_t *seqs = nullptr; const int64_t *seq_off = nullptr;
};

// format_sam_into's twin for BAM records: the kept reads' records one after the other in `out`, *out_len bytes;
// meta (may be null): one entry per WRITTEN record, in order
inline int format_bam_into(const npore_bam *b, const RecFetch &rf, int64_t n, const char *finals, const int64_t *final_off,
                           const int64_t *final_len, const int32_t *status, int threads, RawBuf &out, int64_t *out_len,
                           std::vector<BamRecMeta> *meta, const ReadCodes &codes)
{
    if (!b || n < 0 || !out_len || (n > 0 && (!finals || !final_off || !final_len || !status)))
        return fail(NPORE_E_INVALID, "bad argument");
    const RecSpec &rec = codes.rec;
    std::vector<int64_t> off((size_t)n + 1, 0), nm(rec.full ? (size_t)n : 0, 0);
    // (FULL records: a read's final CIGAR text becomes words ONCE -- NM, MD, cs, de and the record all take the words, counted
    // and written between the two passes; a text that is no CIGAR leaves the read's vector empty: -1 words)
    std::vector<std::vector<uint8_t>> words(rec.full ? (size_t)n : 0);
    auto n_words = [&](int64_t k) { return (int64_t)words[(size_t)k].size() / 4 - 1; };
    const int cs_de = rec.cs_de();
    const bool oc = rec.oc(), has_more = cs_de || oc;
    std::vector<std::string> md(rec.md ? (size_t)n : 0), more(has_more ? (size_t)n : 0);
    std::atomic<int> bad{0};
    const uint32_t pass_mask = rec.pass_mask;
    // a record that passes: the input's bytes; the index gets the input record's own reference length
    auto passed = [&](int64_t k, uint8_t *dst, BamRecMeta *m) -> int64_t {
        const RecView r = rec_of(rf, k);
        const int64_t size = staged_pass_bytes(r.p);
        if (dst) std::memcpy(dst, rf.ptr[(size_t)k], (size_t)size);
        if (dst && m) *m = BamRecMeta{r.ref_id(), r.pos(), rec_ref_len(r), size};
        return size;
    };
    auto record = [&](int64_t k, uint8_t *dst, BamRecMeta *m) {
        if (staged_passes(rec_of(rf, k).p, pass_mask)) return passed(k, dst, m);
        return rec.full ? bam_record_full_words_into(rec_of(rf, k), words[(size_t)k].data(), n_words(k), status[k], nm[(size_t)k], dst, m,
                                                     rec.md ? &md[(size_t)k] : nullptr, has_more ? &more[(size_t)k] : nullptr, oc)
                        : bam_record_into(rec_of(rf, k), finals + final_off[k], final_len[k], status[k], dst, m);
    };
    parallel_for(n, threads, [&](int64_t k) {
        const int64_t ops = rec.full && !(status[k] & NPORE_ST_BAD_INPUT) && !staged_passes(rec_of(rf, k).p, pass_mask)
                                ? cigar_text_ops(finals + final_off[k], final_len[k]) : -1;
        if (ops >= 0) {
            const uint8_t *w = (words[(size_t)k] = cigar_text_words(finals + final_off[k], final_len[k], ops)).data();
            const uint8_t *ref = codes.refs + codes.ref_off[k], *seq = codes.seqs + codes.seq_off[k];
            const int64_t rl = codes.ref_off[k + 1] - codes.ref_off[k], sl = codes.seq_off[k + 1] - codes.seq_off[k];
            nm[(size_t)k] = nm_of_words(w, ops, ref, rl, seq, sl);
            if (rec.md) md_of_words(w, ops, ref, rl, seq, sl, md[(size_t)k]);
            if (cs_de) cs_de_tags_of_words(cs_de, w, ops, ref, rl, seq, sl, more[(size_t)k]);
            if (oc) {              // OC behind them, on a read whose final words are not its input's canonical form (oc_rec.hpp)
                const RecCigar in_cg = rec_cigar(rec_of(rf, k));
                uint32_t ci, cj;
                full_clip_words(in_cg, ci, cj);
                if (oc_changed_words(in_cg.w, ci, cj, w, ops)) oc_tag_of_words(in_cg.w, in_cg.n, more[(size_t)k]);
            }
            // (NPORE_CIGAR_EQX: the record takes the split words; NM, MD, cs and de are the same on either form)
            if (rec.eqx()) words[(size_t)k] = eqx_of_words(w, ops, ref, rl, seq, sl);
        }
        const int64_t sz = record(k, nullptr, nullptr);
        if (sz < 0) bad++;
        off[(size_t)k + 1] = std::max<int64_t>(sz, 0);
    });
    if (bad) return fail(NPORE_E_UNSUPPORTED, "a final CIGAR is no CIGAR text (BAM output)");
    for (int64_t k = 0; k < n; k++) off[(size_t)k + 1] += off[(size_t)k];
    if (!out.ensure((size_t)off[(size_t)n] + 8)) return fail(NPORE_E_NOMEM, "BAM record buffer");
    std::vector<BamRecMeta> all;
    if (meta) all.resize((size_t)n);
    parallel_for(n, threads, [&](int64_t k) {
        if (off[(size_t)k + 1] > off[(size_t)k])
            record(k, reinterpret_cast<uint8_t *>(out.p) + off[(size_t)k], meta ? &all[(size_t)k] : nullptr);
    });
    if (meta) {
        meta->clear();
        for (int64_t k = 0; k < n; k++)
            if (off[(size_t)k + 1] > off[(size_t)k]) meta->push_back(all[(size_t)k]);
    }
    *out_len = off[(size_t)n];
    return NPORE_OK;
}

// The BAM index of a record stream cut into members every BGZF_STORED_PAYLOAD bytes: a record's virtual offset follows
// from its offset u in the stream and the file offset of member u / BGZF_STORED_PAYLOAD.  The members may differ in size
// (stored or Huffman-coded), so the builder keeps stream offsets and a table of the members' places, which the writer
// fills as it writes them (member_at); write() maps the one to the other.  An offset on a cut is the next member's first
// byte; behind the last member that is where the writer says the next one would lie (end_at: finish()).
class BaiBuilder {
public:
    void reset(size_t n_ref, uint64_t base)
    {
        refs_.assign(n_ref, Ref{});
        base_ = end_ = base;
        member_off_.clear();
        sorted_ = true; last_ref_ = -1; last_pos_ = INT64_MIN;
    }
    uint64_t base() const { return base_; }
    void member_at(uint64_t off) { member_off_.push_back(off); }      // in the index's coordinates (base() + bytes written)
    void end_at(uint64_t off) { end_ = off; }
    uint64_t voffset(uint64_t u) const
    {
        const size_t k = (size_t)(u / BGZF_STORED_PAYLOAD);
        return (k < member_off_.size() ? member_off_[k] : end_) << 16 | (u % BGZF_STORED_PAYLOAD);
    }
    void add(const BamRecMeta &m, uint64_t u)         // the record at stream offset u
    {
        if (m.ref < last_ref_ || (m.ref == last_ref_ && m.pos < last_pos_)) sorted_ = false;
        last_ref_ = m.ref;
        last_pos_ = m.pos;
        if (m.ref < 0 || (size_t)m.ref >= refs_.size() || !sorted_) return;
        Ref &r = refs_[(size_t)m.ref];
        const uint64_t v0 = u, v1 = u + (uint64_t)m.bytes;           // (stream offsets: write() maps them)
        const int64_t end = (int64_t)m.pos + std::max<int64_t>(1, m.span);
        auto &chunks = r.bins[bam_reg2bin(m.pos, end)];
        if (!chunks.empty() && chunks.back().second == v0) chunks.back().second = v1;
        else chunks.emplace_back(v0, v1);
        const size_t w0 = (size_t)(std::max<int64_t>(0, m.pos) >> 14), w1 = (size_t)(std::max<int64_t>(0, end - 1) >> 14);
        if (r.lin.size() <= w1) r.lin.resize(w1 + 1, 0);
        for (size_t w = w0; w <= w1; w++)
            if (!r.lin[w]) r.lin[w] = v0 + 1;                        // (0: no record in this window)
    }
    bool sorted() const { return sorted_; }
    bool write(const char *path) const                // complete, or not there at all
    {
        std::string out("BAI\1", 4);
        auto p32 = [&](uint32_t v) { out.append(reinterpret_cast<const char *>(&v), 4); };
        auto p64 = [&](uint64_t v) { out.append(reinterpret_cast<const char *>(&v), 8); };
        p32((uint32_t)refs_.size());
        for (const Ref &r : refs_) {
            p32((uint32_t)r.bins.size());
            for (const auto &bn : r.bins) {
                p32(bn.first);
                p32((uint32_t)bn.second.size());
                for (const auto &c : bn.second) { p64(voffset(c.first)); p64(voffset(c.second)); }
            }
            p32((uint32_t)r.lin.size());
            uint64_t last = 0;
            for (uint64_t v : r.lin) { if (v) last = voffset(v - 1); p64(last); }       // (windows without a record: the entry before)
        }
        const std::string tmp = std::string(path) + ".tmp" + std::to_string((long long)::getpid());
        FILE *fh = std::fopen(tmp.c_str(), "wb");
        if (!fh) return false;
        const bool ok = std::fwrite(out.data(), 1, out.size(), fh) == out.size();
        if (std::fclose(fh) != 0 || !ok || std::rename(tmp.c_str(), path) != 0) { std::remove(tmp.c_str()); return false; }
        return true;
    }

private:
    struct Ref {
        std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
        std::vector<uint64_t> lin;
    };
    std::vector<Ref> refs_;
    uint64_t base_ = 0, end_ = 0;
    std::vector<uint64_t> member_off_;       // where member k of the record stream lies
    bool sorted_ = true;
    int32_t last_ref_ = -1;
    int64_t last_pos_ = INT64_MIN;
};

// Appends a record stream to a file as BGZF members (the FILE rules above): add() takes a batch's record bytes as
// they lie -- stored members' payload goes out from the caller's buffer (writev), only the tail that does not fill a
// member is kept for the next batch -- and does the index bookkeeping; finish() writes the last member, the EOF member if
// asked for, and the index.  deflate (NPORE_OUT_DEFLATE, with NPORE_OUT_MATCH: the match mode): every member is coded by deflate_code.hpp's host twin, on
// `threads` threads -- or comes ready-made from the device (add_coded), which codes the whole members that lie inside a
// batch; the one member that straddles two batches is joined and coded here.  One thread at a time (the file pipeline's
// ordered write step).
class BgzfStoredWriter {
public:
    BgzfStoredWriter() = default;
    BgzfStoredWriter(const BgzfStoredWriter &) = delete;
    BgzfStoredWriter &operator=(const BgzfStoredWriter &) = delete;
    ~BgzfStoredWriter() { if (fd_ >= 0) ::close(fd_); }
    // the file is appended to: what lies there already (the header's members) stays
    // part: a rank's part of a file -- the index counts its offsets from a nominal first member at NPORE_PART_BASE, so
    // that none is 0, which a .bai takes for "no record in this window"; whoever appends the part shifts them
    int open(const char *path, size_t n_ref, const char *bai_path, bool eof_member, bool part = false, int deflate = 0, int threads = 1)
    {
        fd_ = ::open(path, O_WRONLY | O_CREAT | O_APPEND, 0666);
        if (fd_ < 0) return fail(NPORE_E_INVALID, std::string("cannot open '") + path + "' for appending");
        struct stat st;
        if (::fstat(fd_, &st) != 0) return fail(NPORE_E_INVALID, std::string("cannot stat '") + path + "'");
        base_ = (uint64_t)st.st_size;
        bai_path_ = bai_path ? bai_path : "";
        eof_ = eof_member;
        deflate_ = deflate;
        threads_ = threads;
        index_.reset(n_ref, part ? (uint64_t)NPORE_PART_BASE : base_);
        carry_.reserve(BGZF_STORED_PAYLOAD);
        return NPORE_OK;
    }
    bool deflate() const { return deflate_ != 0; }
    int deflate_mode() const { return deflate_; }     // 0, DEFLATE_MODE_HUFFMAN or DEFLATE_MODE_MATCH
    uint64_t stream_bytes() const { return stream_; }
    int add(const uint8_t *bytes, int64_t len, const BamRecMeta *meta, int64_t n_rec)
    {
        if (int rc = index_records(len, meta, n_rec)) return rc;
        size_t at = 0;
        const size_t N = (size_t)len;
        begin_members();
        if (!carry_.empty() && carry_.size() + N >= BGZF_STORED_PAYLOAD) {      // the member begun by the batch before
            const size_t take = BGZF_STORED_PAYLOAD - carry_.size();
            member(carry_.data(), carry_.size(), bytes, take);
            at = take;
        }
        const bool carried = at > 0;
        if (carry_.empty() || carried)
            for (; N - at >= BGZF_STORED_PAYLOAD; at += BGZF_STORED_PAYLOAD) member(bytes + at, BGZF_STORED_PAYLOAD, nullptr, 0);
        if (int rc = flush_members()) return rc;
        if (carried) carry_.clear();
        carry_.insert(carry_.end(), bytes + at, bytes + N);
        return NPORE_OK;
    }
    // A batch from the device (deflate mode): the bytes in front of the stream's first cut inside the batch (head: they
    // end the member begun by the batches before, or are all the batch has), the whole members behind it ready-made, one
    // after the other, member k of sizes[k] bytes, and the bytes behind the last cut (tail).
    int add_coded(const uint8_t *head, int64_t head_len, const uint8_t *members, const uint32_t *sizes, int64_t n_members,
                  const uint8_t *tail, int64_t tail_len, const BamRecMeta *meta, int64_t n_rec)
    {
        const size_t want = (BGZF_STORED_PAYLOAD - carry_.size() % BGZF_STORED_PAYLOAD) % BGZF_STORED_PAYLOAD;
        if (head_len < 0 || tail_len < 0 || n_members < 0 || tail_len >= (int64_t)BGZF_STORED_PAYLOAD ||
            ((n_members > 0 || tail_len > 0) ? (size_t)head_len != want : (size_t)head_len > want) )
            return fail(NPORE_E_INVALID, "internal: a batch's coded members do not fit the stream's cuts");
        if (int rc = index_records(head_len + n_members * (int64_t)BGZF_STORED_PAYLOAD + tail_len, meta, n_rec)) return rc;
        begin_members();
        carry_.insert(carry_.end(), head, head + head_len);
        const bool joined = carry_.size() == BGZF_STORED_PAYLOAD;
        if (joined) member(carry_.data(), carry_.size(), nullptr, 0);
        size_t at = 0;
        for (int64_t k = 0; k < n_members; k++) {
            if (sizes[k] < 28 || sizes[k] > BGZF_STORED_PAYLOAD + BGZF_STORED_OVERHEAD) return fail(NPORE_E_INVALID, "internal: bad size of a coded member");
            jobs_.push_back(Job{nullptr, 0, nullptr, 0, members + at, sizes[k]});
            at += sizes[k];
        }
        if (int rc = flush_members()) return rc;
        if (joined) carry_.clear();
        carry_.insert(carry_.end(), tail, tail + tail_len);
        return NPORE_OK;
    }
    // info[4]: records, payload bytes, 1 = an index was written / 0 = none asked for / -1 = not in coordinate order, file size
    int finish(int64_t *info)
    {
        begin_members();
        if (!carry_.empty()) member(carry_.data(), carry_.size(), nullptr, 0);
        if (int rc = flush_members()) return rc;
        index_.end_at(index_.base() + file_bytes_);
        if (eof_) {
            iov_.push_back(iovec{const_cast<uint8_t *>(BGZF_EOF_MEMBER), 28});
            file_bytes_ += 28;
            if (int rc = flush_iov()) return rc;
        }
        carry_.clear();
        const int rcc = ::close(fd_);
        fd_ = -1;
        if (rcc != 0) return fail(NPORE_E_INVALID, "close failed");
        int indexed = 0;
        if (!bai_path_.empty()) {
            if (!index_.sorted()) { indexed = -1; std::remove(bai_path_.c_str()); }
            else if (!index_.write(bai_path_.c_str())) return fail(NPORE_E_INVALID, "cannot write '" + bai_path_ + "'");
            else indexed = 1;
        }
        if (info) { info[0] = n_rec_; info[1] = (int64_t)stream_; info[2] = indexed; info[3] = (int64_t)(base_ + file_bytes_); }
        return NPORE_OK;
    }

private:
    struct Head { uint8_t h[23], t[8]; };
    // a member to be written: the payload a + b (b may be empty), or (ready != null) a member as it is
    struct Job { const uint8_t *a; size_t na; const uint8_t *b; size_t nb; const uint8_t *ready; size_t n_ready; };
    int index_records(int64_t len, const BamRecMeta *meta, int64_t n_rec)
    {
        uint64_t u = stream_;
        for (int64_t k = 0; k < n_rec; k++) { index_.add(meta[k], u); u += (uint64_t)meta[k].bytes; }
        if (u != stream_ + (uint64_t)len) return fail(NPORE_E_INVALID, "internal: record sizes do not add up to the batch's bytes");
        n_rec_ += n_rec;
        stream_ = u;
        return NPORE_OK;
    }
    void begin_members() { heads_.clear(); iov_.clear(); jobs_.clear(); }
    void member(const uint8_t *a, size_t na, const uint8_t *b, size_t nb) { jobs_.push_back(Job{a, na, b, nb, nullptr, 0}); }
    // the queued members, in order, to the file; their places to the index
    int flush_members()
    {
        if (deflate_) {                                 // code the payloads (a ready-made member needs nothing)
            const size_t slot = BGZF_STORED_PAYLOAD + BGZF_STORED_OVERHEAD + BGZF_STORED_PAYLOAD;     // member, and a joined payload behind it
            slot_of_.assign(jobs_.size(), 0);           // (only what is coded here takes a slot: a device batch has one such member at most)
            size_t n_coded = 0;
            for (size_t k = 0; k < jobs_.size(); k++)
                if (!jobs_[k].ready) slot_of_[k] = n_coded++;
            if (coded_.size() < n_coded * slot) coded_.resize(n_coded * slot);
            coded_len_.assign(jobs_.size(), 0);
            parallel_for((int64_t)jobs_.size(), n_coded > 1 ? threads_ : 1, [&](int64_t k) {
                const Job &j = jobs_[(size_t)k];
                if (j.ready) return;
                uint8_t *out = coded_.data() + slot_of_[(size_t)k] * slot;
                const uint8_t *in = j.a;
                if (j.nb) {
                    uint8_t *joined = out + BGZF_STORED_PAYLOAD + BGZF_STORED_OVERHEAD;
                    std::memcpy(joined, j.a, j.na);
                    std::memcpy(joined + j.na, j.b, j.nb);
                    in = joined;
                }
                coded_len_[(size_t)k] = deflate_member_host(in, j.na + j.nb, crc32_fast(0, in, j.na + j.nb), out, deflate_);
            });
            for (size_t k = 0; k < jobs_.size(); k++) {
                const Job &j = jobs_[k];
                index_.member_at(index_.base() + file_bytes_);
                if (j.ready) { iov_.push_back(iovec{const_cast<uint8_t *>(j.ready), j.n_ready}); file_bytes_ += j.n_ready; }
                else { iov_.push_back(iovec{coded_.data() + slot_of_[k] * slot, coded_len_[k]}); file_bytes_ += coded_len_[k]; }
            }
            return flush_iov();
        }
        for (const Job &j : jobs_) {
            if (j.ready) return fail(NPORE_E_INVALID, "internal: a coded member for a stored file");
            index_.member_at(index_.base() + file_bytes_);
            stored_member(j.a, j.na, j.b, j.nb);
        }
        return flush_iov();
    }
    // one stored member of a + b bytes (b may be empty) queued for the next writev
    void stored_member(const uint8_t *a, size_t na, const uint8_t *b, size_t nb)
    {
        const size_t n = na + nb, bsize = n + BGZF_STORED_OVERHEAD;
        heads_.emplace_back();
        Head &hd = heads_.back();
        const uint8_t h[23] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, (uint8_t)((bsize - 1) & 0xFF), (uint8_t)((bsize - 1) >> 8),
                               1, (uint8_t)(n & 0xFF), (uint8_t)(n >> 8), (uint8_t)(~n & 0xFF), (uint8_t)((~n >> 8) & 0xFF)};
        std::memcpy(hd.h, h, 23);
        uint32_t crc = crc32_fast(0, a, na);
        if (nb) crc = crc32_fast(crc, b, nb);
        const uint32_t isize = (uint32_t)n;
        std::memcpy(hd.t, &crc, 4);
        std::memcpy(hd.t + 4, &isize, 4);
        // (heads_ is a deque: the addresses stay while members are added)
        iov_.push_back(iovec{hd.h, 23});
        iov_.push_back(iovec{const_cast<uint8_t *>(a), na});
        if (nb) iov_.push_back(iovec{const_cast<uint8_t *>(b), nb});
        iov_.push_back(iovec{hd.t, 8});
        file_bytes_ += bsize;
    }
    int flush_iov()
    {
        size_t k = 0;
        while (k < iov_.size()) {
            const int cnt = (int)std::min<size_t>(iov_.size() - k, 512);
            ssize_t w = ::writev(fd_, iov_.data() + k, cnt);
            if (w < 0) { if (errno == EINTR) continue; return fail(NPORE_E_INVALID, "short write"); }
            while (w > 0 && k < iov_.size()) {                  // (a partial write: go on behind it)
                if ((size_t)w >= iov_[k].iov_len) { w -= (ssize_t)iov_[k].iov_len; k++; }
                else { iov_[k].iov_base = static_cast<uint8_t *>(iov_[k].iov_base) + w; iov_[k].iov_len -= (size_t)w; w = 0; }
            }
            while (k < iov_.size() && iov_[k].iov_len == 0) k++;
        }
        iov_.clear();
        return NPORE_OK;
    }
    int fd_ = -1;
    uint64_t base_ = 0, stream_ = 0, file_bytes_ = 0;
    int64_t n_rec_ = 0;
    bool eof_ = false;
    int deflate_ = 0;                        // 0: stored members; DEFLATE_MODE_HUFFMAN / DEFLATE_MODE_MATCH
    int threads_ = 1;
    std::string bai_path_;
    std::vector<uint8_t> carry_;             // the tail of the stream that does not fill a member yet (< 65 280 bytes)
    std::deque<Head> heads_;
    std::vector<iovec> iov_;
    std::vector<Job> jobs_;
    std::vector<uint8_t> coded_;             // deflate: the members coded here, a slot each
    std::vector<size_t> coded_len_, slot_of_;
    BaiBuilder index_;
};

// ---- the one-pass reader: the record stream walked once, front to back, no record index ------------------------
// A stretch of the inflated stream in one buffer: d[0 .. n) lies at offset abs0 of the stream.  The buffer lives as
// long as somebody points into it (a batch's records).
struct BamWindow {
    std::shared_ptr<RawBuf> buf;
    const uint8_t *d = nullptr;
    size_t n = 0;
    uint64_t abs0 = 0;
};

// The inflated stream of a BGZF file from one block on, in windows of NPORE_BAM_WINDOW_BLOCKS consecutive blocks (1024:
// <= 64 MB of stream), each inflated ONCE.  ONE inflater thread takes the windows in file order, each on all cores
// (bgzf_inflate_range; NPORE_INFLATE_THREADS: how many it may take at once), and keeps up to NPORE_BAM_WINDOWS_AHEAD (3)
// of them ready -- the inflation then runs whenever CPUs are free instead of one window ahead of the walk (the
// acquisitions of consecutive batches took 12 ... 72 ms that way, the long ones waiting for a window that the SAM text
// and packing threads had slowed down).  A window is inflated behind HEAD bytes of room, where next() puts the tail the
// reader carries over from the window before; so every record lies in one buffer.  The thread starts with the first
// next() and is stopped and joined by the destructor: a reader that ends early (the end of its share, max_reads, a
// failure) leaves at most that many windows inflated for nothing.
class BamWindowSource {
public:
    static constexpr size_t HEAD = 4u << 20;
    // inflate: who inflates a window's blocks in place of bgzf_inflate_range (empty: nobody).  With one, a window is 4096
    // blocks by default: the device decoder (inflate_kernels.hpp) runs one wave per block, and 1024 of them are one wave
    // per SIMD -- a dependent chain with nobody to hide it
    BamWindowSource(const npore_bam *b, int threads, BgzfInflateFn inflate = nullptr) : b_(b), inflate_threads_(threads), inflate_(std::move(inflate))
    {
        if (inflate_) win_blocks_ = 4096;
        if (const char *e = std::getenv("NPORE_BAM_WINDOW_BLOCKS")) win_blocks_ = (size_t)std::max(1, std::atoi(e));
        if (const char *e = std::getenv("NPORE_BAM_WINDOWS_AHEAD")) depth_ = std::max(1, std::atoi(e));
        if (const char *e = std::getenv("NPORE_INFLATE_THREADS")) inflate_threads_ = std::max(1, std::atoi(e));
    }
    BamWindowSource(const BamWindowSource &) = delete;
    BamWindowSource &operator=(const BamWindowSource &) = delete;
    ~BamWindowSource()
    {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_.notify_all();
        if (thread_.joinable()) thread_.join();
    }
    void start_at(size_t block) { next_block_ = block; }         // (before the first next(): a share that begins mid-file)
    // Replaces w by the next window, the unread tail w.d[from .. w.n) carried in front of it.  1: in place; 0: no block
    // is left (w stays as it is); -1: failure (fail() called)
    int next(BamWindow &w, size_t from)
    {
        if (next_block_ >= b_->blocks.size()) return 0;
        if (!thread_.joinable()) thread_ = std::thread([this, first = next_block_] { inflate_ahead(first); });
        const size_t c = (w.buf && from < w.n) ? w.n - from : 0;
        const uint64_t win_off = b_->blocks[next_block_].out_off;
        Pending pd;
        {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return !ready_.empty() || ended_; });
            if (ready_.empty()) { fail(NPORE_E_INVALID, "BAM window reader ended early"); return -1; }
            pd = std::move(ready_.front());
            ready_.pop_front();
        }
        cv_.notify_all();
        if (!pd.ok || pd.b0 != next_block_) {
            fail(NPORE_E_INVALID, pd.err.empty() ? std::string("corrupt BGZF block (or out of memory)") : pd.err);
            return -1;
        }
        std::shared_ptr<RawBuf> nw = pd.buf;
        uint8_t *d0 = reinterpret_cast<uint8_t *>(nw->p) + HEAD;
        if (c > HEAD) {                                          // a record longer than the room in front: copy once
            auto big = std::make_shared<RawBuf>();
            if (!big->ensure(c + pd.bytes + 8)) { fail(NPORE_E_NOMEM, "BAM window"); return -1; }
            std::memcpy(big->p + c, d0, pd.bytes);
            nw = big;
            d0 = reinterpret_cast<uint8_t *>(nw->p) + c;
        }
        if (c) std::memcpy(d0 - c, w.d + from, c);
        w.buf = nw;
        w.d = d0 - c;
        w.abs0 = win_off - c;
        w.n = c + pd.bytes;
        next_block_ = pd.b1;
        return 1;
    }

private:
    struct Pending { std::shared_ptr<RawBuf> buf; size_t bytes = 0, b0 = 0, b1 = 0; bool ok = false; std::string err; };
    void inflate_ahead(size_t b0)                                // the inflater thread
    {
        const size_t end = b_->blocks.size();
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || (int)ready_.size() < depth_; });
                if (stop_ || b0 >= end) { ended_ = true; cv_.notify_all(); return; }
            }
            Pending pd;
            pd.b0 = b0;
            pd.b1 = std::min(end, b0 + win_blocks_);
            const uint64_t w0 = b_->blocks[b0].out_off, w1 = b_->blocks[pd.b1 - 1].out_off + b_->blocks[pd.b1 - 1].out_len;
            pd.bytes = (size_t)(w1 - w0);
            try {                                                // (no exception may leave a thread: next() sees ok == false)
                pd.buf = std::make_shared<RawBuf>();
                uint8_t *const d = pd.buf->ensure(HEAD + pd.bytes + 8) ? reinterpret_cast<uint8_t *>(pd.buf->p) + HEAD : nullptr;
                if (d && inflate_) {
                    pd.ok = inflate_(*b_->file, b_->blocks, b0, pd.b1, d, inflate_threads_);
                    if (!pd.ok) pd.err = g_err;                  // (the hook's words are this thread's: next() passes them on)
                } else {
                    pd.ok = d && bgzf_inflate_range(*b_->file, b_->blocks, b0, pd.b1, d, inflate_threads_);
                }
            } catch (...) {
                pd.ok = false;
            }
            b0 = pd.b1;
            {
                std::lock_guard<std::mutex> lk(m_);
                ready_.push_back(std::move(pd));
            }
            cv_.notify_all();
        }
    }
    const npore_bam *b_;
    size_t win_blocks_ = 1024;
    int depth_ = 3, inflate_threads_;
    BgzfInflateFn inflate_;
    size_t next_block_ = 0;                  // the block the next window begins with (the walking thread's)
    std::mutex m_;                           // guards ready_, stop_, ended_
    std::condition_variable cv_;
    std::deque<Pending> ready_;
    bool stop_ = false, ended_ = false;
    std::thread thread_;
};

// what a one-pass walk refuses before it begins
inline int one_pass_args_check(const npore_bam *b, int n_regions, const int32_t *ref_id, int64_t max_reads)
{
    if (!b->file || b->blocks.empty()) return fail(NPORE_E_INVALID, "one-pass ingest needs a handle opened on a BGZF file (modes 2 and 3)");
    for (int g = 0; g < n_regions; g++)
        if (ref_id[g] < 0 || ref_id[g] >= (int32_t)b->ref_names.size() || (g > 0 && ref_id[g] <= ref_id[g - 1]))
            return fail(NPORE_E_UNSUPPORTED, "one-pass ingest takes at most one region per contig, in the order of the BAM header");
    if (b->has_share && max_reads > 0)
        return fail(NPORE_E_UNSUPPORTED, "one-pass ingest: max_reads needs one process (the ranks cannot know how many reads the others keep)");
    return NPORE_OK;
}

// The records of a coordinate-sorted BAM that npore_bam_select would keep for the same regions (at most one per contig,
// in header order), max_reads and flag filter, found by ONE walk over the stream, batch by batch.  Several processes on
// one file (npore_bam_set_share): this one keeps the records that START in [share_begin, share_end) of the inflated
// stream -- a stretch that begins at a record; the header was read when the handle was opened.
// next_batch() is called by one thread at a time (whichever packing thread holds the file pipeline's `acquired` gate):
// the walker's state needs no lock, the window source's queue has its own.
class BamRecordWalker {
public:
    BamRecordWalker(const npore_bam *b, int n_regions, const int32_t *ref_id, const int64_t *start, const int64_t *stop,
                    int64_t max_reads, int threads, uint32_t drop_flags = PASS_FLAGS, BgzfInflateFn inflate = nullptr, uint32_t pass_mask = PASS_NONE)
        : b_(b), src_(b, threads, std::move(inflate)), n_regions_(n_regions), ref_id_(ref_id), start_(start), stop_(stop), max_reads_(max_reads),
          drop_flags_(drop_flags & ~pass_mask), pass_mask_(pass_mask), index_claims_(!b->has_reads_index.empty()),
          done_(n_regions == 0 && !index_claims_)          // (no region at all may be the index's doing: walk to the first placed record)
    {
        if (!b->has_share) return;
        if (b->share_begin == UINT64_MAX) done_ = true;          // nothing left for this rank
        else if (b->share_begin > 0) { src_.start_at(b->share_block); have_header_ = seek_share_ = true; }
    }
    // The next (up to) batch_reads kept records: pointers to them in rf.ptr, the windows they lie in added to `keep`.
    // Returns their number, 0 at the end of the walk, a negative code after fail().
    int64_t next_batch(RecFetch &rf, std::vector<std::shared_ptr<RawBuf>> &keep, int64_t batch_reads)
    {
        rf.ptr.clear();
        while ((int64_t)rf.ptr.size() < batch_reads && !done_) {
            if (!have_header_) {
                npore_bam scratch;
                size_t hdr_end = 0;
                const int hrc = win_.buf ? bam_parse_header(&scratch, win_.d, win_.n, &hdr_end) : -1;
                if (hrc == 0) return fail(NPORE_E_INVALID, "not a BAM file");
                if (hrc < 0) {                                   // the header does not end in what is inflated so far
                    p_ = 0;
                    if (load_window() != 1) return -1;           // (the blocks running out here is a failure too)
                    continue;
                }
                have_header_ = true;
                p_ = hdr_end;
                continue;
            }
            size_t nx = 0;
            const Frame f = frame_record(win_.d, win_.n, p_, nx);
            if (f == Frame::CORRUPT) return fail(NPORE_E_INVALID, "truncated BAM record");
            if (f == Frame::MORE) {
                const int lw = load_window();
                if (lw < 0) return lw;
                if (lw == 0) done_ = true;
                continue;
            }
            if (win_.abs0 + p_ >= b_->share_end) { done_ = true; break; }        // the next process's stretch begins here
            const uint8_t *q = win_.d + p_;
            p_ = nx;
            if (!record_is_sound(q)) return fail(NPORE_E_INVALID, "corrupt BAM record");
            const RecView rv = rec_view(q);
            const int32_t rid = rv.ref_id();
            if (rid < 0) continue;                               // unplaced
            if (rid < last_rid_) return fail(NPORE_E_UNSUPPORTED, "the BAM is not sorted by reference: one-pass ingest needs a coordinate-sorted file");
            last_rid_ = rid;
            // the contigs without reads are the index's claim (bam_open_header_only), and the default regions leave them
            // out: a record on one of them -- met between two regions, or where the walk stops behind the last -- says
            // that the index is stale, and reads would be missing from the output without a word
            if (index_claims_ && (size_t)rid < b_->ref_has_reads.size() && !b_->ref_has_reads[(size_t)rid])
                return fail(NPORE_E_INVALID, "the index '" + b_->has_reads_index + "' says that contig '" + b_->ref_names[(size_t)rid] +
                                                 "' has no reads, but the BAM has some: the index is stale (rebuild or remove it)");
            while (g_ < n_regions_ && ref_id_[g_] < rid) g_++;
            if (g_ == n_regions_) { done_ = true; break; }
            if (ref_id_[g_] != rid) continue;
            int64_t pos = rv.pos(), rl = rec_ref_len(rv);
            if (rl == 0 && staged_passes(rv.p, pass_mask_)) rl = 1;              // (bam_select's rule for a record that passes)
            if (!(pos < stop_[g_] && pos + rl > start_[g_])) continue;           // overlaps [start, stop)
            if (max_reads_ > 0 && kept_ >= max_reads_) { done_ = true; break; }  // src/bam.pyx:29-30
            if ((uint32_t)rv.flag() & drop_flags_) continue;                     // secondary / supplementary / unmapped, :31-32
            rf.ptr.push_back(q);
            if (keep.empty() || keep.back() != win_.buf) keep.push_back(win_.buf);
            kept_++;
        }
        return (int64_t)rf.ptr.size();
    }

private:
    // the next window behind what has been walked, the unread tail in front.  1: in place; 0: the blocks have run out
    // at a record's end; -1: failure (fail() called) -- they ran out inside a record, or before the header's end
    int load_window()
    {
        const int rc = src_.next(win_, p_);
        if (rc == 0 && (!have_header_ || (win_.buf && p_ < win_.n))) {
            fail(NPORE_E_INVALID, have_header_ ? "truncated BAM record" : "not a BAM file");
            return -1;
        }
        if (rc != 1) return rc;
        p_ = 0;
        if (seek_share_) { p_ = (size_t)(b_->share_begin - win_.abs0); seek_share_ = false; }   // (the first window of a share that begins mid-file)
        return 1;
    }
    const npore_bam *b_;
    BamWindowSource src_;
    BamWindow win_;                          // the window being walked
    size_t p_ = 0;                           // ... and the offset of the next record in it
    bool have_header_ = false, seek_share_ = false;
    const int n_regions_;
    const int32_t *const ref_id_;            // the regions, ascending in ref_id
    const int64_t *const start_, *const stop_;
    int g_ = 0;                              // the region the walk has reached
    const int64_t max_reads_;
    const uint32_t drop_flags_;              // (the realigner's; the recount of the confusion matrices filters for itself)
    const uint32_t pass_mask_;               // ... without these bits: such records pass through (staged_head.hpp)
    const bool index_claims_;                // ref_has_reads is what a .bai said: checked against every placed record met
    int64_t kept_ = 0;
    int32_t last_rid_ = -1;                // (the sorted-by-reference check)
    bool done_;
};

}  // namespace npore
