// file_pipeline.hpp -- what a batch of the BAM -> SAM / BAM file pipeline is: its slot, the run's mode and output, and the batch's
// stages (pack, enqueue, collect, write) as functions of the slot and the mode.  The order the stages of neighbouring batches run
// in is batch_order.hpp's; the device path of a batch is align_engine.hpp's, behind which npore_api.cpp includes this file.
#pragma once
#include "batch_order.hpp"

inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// One batch on its way through the BAM -> SAM pipeline: host staging (page-locked where it crosses PCIe) and offsets.
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
    // ... with NPORE_OUT_DEFLATE (bam_deflate_kernels.hpp): the members' plans, sizes and places, the coded members, the
    // batch's four numbers; the size table and the numbers here; recs_pin then holds members | head fragment | tail fragment
    DevBuf d_plans, d_sizes, d_moff, d_comp, d_info;
    DevBuf d_htab, d_tokens;               // NPORE_OUT_MATCH: per member the hash table (2^15 positions) and the tokens
    PinnedBuf sizes_pin, info_pin;
    int64_t max_members = 0;
    int64_t frag[4] = {0, 0, 0, 0};        // of the fetched batch: members, their bytes, head bytes, tail bytes
    int64_t ctext_copied = 0;              // bytes of the compact buffer the batch's last group sent behind its kernels
    TextCompact cmp{}; BamEmit emit{};     // what the batch's AlignArgs point at (slot_enqueue): they live as long as the batch
    PinnedBuf olen_pin, st_pin;            // lengths / status bits of an ASYNCHRONOUS batch land here (page-locked: a copy into
                                           // pageable memory would make the enqueueing call wait for the whole batch)
    hipEvent_t done = nullptr;             // ... behind which this event is recorded (npore_bam_realign_file)
    std::vector<std::shared_ptr<RawBuf>> keep;   // one-pass ingest: the inflated windows the batch's records lie in
    ~npore_batch_slot() { if (done) (void)hipEventDestroy(done); }
    RecFetch rf;                 // the batch's BAM records (streamed handles: inflated for the batch)
    double t_ms[6] = {0, 0, 0, 0, 0, 0};   // npore_bam_realign_file: fetch + pack, align call, standardise, format, write, (spare)
    std::vector<int64_t> ro, so, co, oo, fo, olen, flen;
    std::vector<BamRecMeta> meta;  // BAM output: what the index needs of every record written (sam then holds record bytes)
    int64_t sam_len = 0, m = 0;  // bytes of s.sam / the device's records; reads of the batch
    int rc = 0;                  // how the batch failed, and the message of its stage that did (batch_order.hpp keeps the run's)
    std::string err;
};

namespace {
int out_deflate_mode(int flags) { return !(flags & NPORE_OUT_DEFLATE) ? 0 : (flags & NPORE_OUT_MATCH) ? DEFLATE_MODE_MATCH : DEFLATE_MODE_HUFFMAN; }
// NPORE_OUT_DEFLATE on the device: room for the most members `bytes` record bytes can hold
int slot_deflate_buffers(npore_batch_slot &s, int64_t bytes, int mode)
{
    const int64_t mm = bytes / (int64_t)BGZF_STORED_PAYLOAD + 1;
    s.max_members = mm;
    int rc = 0;
    if (mode == DEFLATE_MODE_MATCH)         // a member's hash table and its tokens (a token per byte at the most)
        if ((rc = s.d_htab.ensure((size_t)mm * sizeof(uint16_t) << DEFLATE_HASH_BITS)) || (rc = s.d_tokens.ensure((size_t)mm * BGZF_STORED_PAYLOAD * sizeof(uint32_t) + 64)))
            return rc;
    if ((rc = s.d_plans.ensure((size_t)mm * sizeof(DeflateMemberPlan))) || (rc = s.d_sizes.ensure((size_t)mm * 4 + 64)) || (rc = s.d_moff.ensure((size_t)mm * 8 + 64)) ||
        (rc = s.d_comp.ensure((size_t)mm * (BGZF_STORED_PAYLOAD + BGZF_STORED_OVERHEAD) + 2 * BGZF_STORED_PAYLOAD + 64)) ||      // (members, two fragments)
        (rc = s.d_info.ensure(64)) || (rc = s.sizes_pin.ensure((size_t)mm * 4 + 64))) return rc;
    return s.info_pin.ensure(64);
}
DeflateParams slot_deflate_params(npore_batch_slot &s, const uint8_t *d_recs, const unsigned long long *d_total, unsigned long long *d_stream_pos, int mode)
{
    DeflateParams dp{};
    dp.mode = mode;
    if (mode == DEFLATE_MODE_MATCH) { dp.htab = s.d_htab.as<uint16_t>(); dp.tokens = s.d_tokens.as<uint32_t>(); }
    dp.recs = d_recs; dp.total = d_total; dp.stream_pos = d_stream_pos;
    dp.plans = s.d_plans.as<DeflateMemberPlan>(); dp.sizes = s.d_sizes.as<uint32_t>(); dp.off = s.d_moff.as<int64_t>();
    dp.comp = s.d_comp.as<uint8_t>(); dp.comp_cap = s.max_members * (int64_t)(BGZF_STORED_PAYLOAD + BGZF_STORED_OVERHEAD);
    dp.max_members = s.max_members; dp.info = s.d_info.as<int64_t>();
    return dp;
}

// npore_bam_set_output holds for ONE run: the run that writes takes the setting and leaves the default behind
struct OutputSetting { int format, flags; std::string bai; RecSpec rec; };
OutputSetting take_output_setting(npore_bam *b)
{
    OutputSetting o{b->out_format, b->out_flags, b->out_bai, b->out_rec};
    b->out_format = NPORE_OUT_SAM; b->out_flags = 0; b->out_rec = RecSpec{}; b->out_bai.clear();
    std::fill(b->out_info, b->out_info + 4, 0);
    return o;
}

// How a file run's batches travel, decided once per run (pipe_mode) and handed to every stage
struct PipeMode {
    bool glue = false;           // realign_read's glue on the device: the slots receive the final CIGAR text
    bool dpack = false;          // ... and align()'s inputs unpacked from the records on the device (the host glue needs the base arrays on the host)
    bool bam = false;            // BAM records out instead of SAM text ...
    RecSpec rec;                 // ... which records (hostio.hpp; the run's: RunOutput::open)
    int deflate = 0;             // the writer's DEFLATE_MODE_*, 0: stored members
    // BAM mode: the records are built on the device where the default pipeline runs (device pack + device glue:
    // bam_emit_kernels.hpp); with the host glue or the host pack the host twin makes them (format_bam_into)
    bool dev_records() const { return bam && dpack; }
    bool dev_deflate() const { return dev_records() && deflate != 0; }      // ... and coded into whole members there too (bam_deflate_kernels.hpp)
    int stage_form() const { return !bam ? STAGE_HEAD : rec.full ? STAGE_FULL : STAGE_QUALS; }      // of the device pack's record heads
};

// Where a file run's output goes: the SAM text's FILE, or (npore_bam_set_output) the BAM writer
struct RunOutput {
    FILE *fh = nullptr;
    std::unique_ptr<BgzfStoredWriter> bw;
    npore_bam *b = nullptr;
    RecSpec rec;                        // the records the run writes, as the setters built them (rec_spec_of)
    int open(npore_bam *bam, const char *out_path, int threads)
    {
        b = bam;
        const OutputSetting o = take_output_setting(b);
        rec = o.rec;
        if (o.format == NPORE_OUT_BAM) {
            bw.reset(new BgzfStoredWriter());
            return bw->open(out_path, b->ref_names.size(), o.bai.empty() ? nullptr : o.bai.c_str(), (o.flags & NPORE_OUT_EOF) != 0,
                            (o.flags & NPORE_OUT_PART) != 0, out_deflate_mode(o.flags), std::max(1, host_threads(threads) / 2));
        }
        fh = std::fopen(out_path, "ab");
        return fh ? NPORE_OK : fail(NPORE_E_INVALID, std::string("cannot open '") + out_path + "' for appending");
    }
    int write(const npore_batch_slot &t, const PipeMode &pm)      // a collected batch, in its turn
    {
        if (!bw) return std::fwrite(t.sam.p, 1, (size_t)t.sam_len, fh) == (size_t)t.sam_len ? NPORE_OK : fail(NPORE_E_INVALID, "short write");
        const uint8_t *q = reinterpret_cast<const uint8_t *>(pm.dev_records() ? t.recs_pin.p : t.sam.p);
        const int64_t n_rec = (int64_t)t.meta.size();
        // (the device's members: recs_pin holds members | head fragment | tail fragment)
        return (pm.dev_deflate() ? bw->add_coded(q + t.frag[1], t.frag[2], q, reinterpret_cast<const uint32_t *>(t.sizes_pin.p), t.frag[0],
                                                 q + t.frag[1] + t.frag[2], t.frag[3], t.meta.data(), n_rec)
                                 : bw->add(q, t.sam_len, t.meta.data(), n_rec)) ? NPORE_E_INVALID : NPORE_OK;
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

PipeMode pipe_mode(const npore_ctx *ctx, const RunOutput &out)      // (NPORE_DEVICE_GLUE was read when the context was made, NPORE_DEVICE_PACK is per run)
{
    const char *e = std::getenv("NPORE_DEVICE_PACK");
    const bool glue = ctx->device_glue != 0, dpack = glue && ctx->device_pack != 0 && !(e && std::atoi(e) == 0);
    PipeMode pm;
    pm.glue = glue; pm.dpack = dpack;
    pm.bam = out.bw != nullptr; pm.rec = out.rec;
    pm.deflate = out.bw ? out.bw->deflate_mode() : 0;
    return pm;
}

// The FASTA on the device (once per FASTA and context) and, per BAM reference, where its contig lies there.
int device_fasta(npore_ctx *ctx, const npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref)
{
    const size_t bytes = fa->off.empty() ? 0 : (size_t)fa->off.back();
    HIP_TRY(hipStreamSynchronize(ctx->stream));       // (no group of an earlier run still reads the FASTA or the table)
    if (ctx->d_fasta_serial != fa->serial || ctx->d_fasta_bytes != bytes) {
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
    if (int rc = ctx->d_ctg.ensure(tab.size() * sizeof(CtgEntry))) return rc;
    HIP_TRY(hipMemcpy(ctx->d_ctg.p, tab.data(), tab.size() * sizeof(CtgEntry), hipMemcpyHostToDevice));
    ctx->n_ctg = (int)nref;
    return NPORE_OK;
}

// ---- pack: the s.m records in s.rf into the slot, and the sizes of what comes back -------------------------------------------
// A read's slot receives its op string (host glue: a byte per base at the most), the collapsed CIGAR text (device glue: 2 bytes
// per op + 16 always suffice) or its CIGAR words (records built on the device: 4 bytes per op + 16); its final text the same
void slot_pack_sizes(npore_batch_slot &s, int threads, const PipeMode &pm)
{
    const size_t n = (size_t)s.m;
    for (auto *v : {&s.ro, &s.so, &s.co, &s.oo, &s.fo}) v->assign(n + 1, 0);
    s.olen.assign(n, 0);
    s.flen.assign(n, 0);
    pack_sizes_of(s.rf, s.m, s.ro.data(), s.so.data(), s.co.data(), threads, pm.rec.pass_mask);
    for (size_t k = 0; k < n; k++) {
        const int64_t cap = (s.ro[k + 1] - s.ro[k]) + (s.so[k + 1] - s.so[k]);
        s.oo[k + 1] = s.oo[k] + (!pm.glue ? cap : (pm.dev_records() ? 4 : 2) * cap + 16);
        s.fo[k + 1] = s.fo[k] + 2 * cap + 16;
    }
}
// host pack: the inputs of npore_align_batch as three arrays
int slot_pack_arrays(const npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, int threads, npore_batch_slot &s, const PipeMode &pm)
{
    const size_t n = (size_t)s.m;
    slot_pack_sizes(s, threads, pm);
    int rce = 0;
    if ((rce = s.refs.ensure((size_t)s.ro[n] + 64)) || (rce = s.seqs.ensure((size_t)s.so[n] + 64)) || (rce = s.cigs.ensure((size_t)s.co[n] + 64))) return rce;
    if (!fa || !fasta_of_ref) return fail(NPORE_E_INVALID, "bad argument");
    if (int rc = pack_records(b, s.rf, fa, fasta_of_ref, s.m, reinterpret_cast<uint8_t *>(s.refs.p), s.ro.data(), reinterpret_cast<uint8_t *>(s.seqs.p),
                              s.so.data(), s.cigs.p, s.co.data(), threads, true, pm.rec.pass_mask)) return rc;
    // (device glue: the texts come back compacted -- slot_enqueue --, neither a page-locked copy of the slots nor the host glue's finals)
    if (pm.glue) return NPORE_OK;
    if (int rc = s.alns.ensure((size_t)s.oo[n] + 64)) return rc;
    return s.finals.ensure((size_t)s.fo[n] + 64) ? NPORE_OK : fail(NPORE_E_NOMEM, "batch buffers");     // (a RawBuf: hostio.hpp)
}
// device pack: the sizes as above, and instead of the three arrays the HEADS of the records (block_size word, fixed fields,
// name, CIGAR words, 4-bit bases -- about half of a record; qualities and tags are not needed on the device) copied one
// after the other into the slot's page-locked buffer; unpack_kernels.hpp does the rest per group.
// BAM mode: each record up to the end of its QUALITIES (the tags stay on the host), the reads' HP values, and the bound of the
// batch's record bytes, s.rec_cap (its terms: hostio.hpp).
// FULL records: the kept aux bytes behind the qualities (STAGE_FULL) and their number in the HP values' place.
// A record that passes (RecSpec::pass_mask, staged_head.hpp): the block_size word and the whole record are staged.
// THE plan of the staged heads of the n records in rf, whoever stages them (the file pipeline below, the debug entry of
// npore_api.cpp): a read on a contig that is not in the FASTA is refused; raw_off[n + 1]: the heads one after the other, each
// as long as stage_record(form) makes it, no padding between them; BAM out (form above STAGE_HEAD) also hp[n]: the read's HP
// value, the kept aux bytes of a FULL record, 0 for a record that passes -- and the sum of record_bound (hostio.hpp) over the
// records, read k's final as long as extent_of(k) says.  seq_off: the reads' slices of unclipped bases (pack_sizes_of).
template <class ExtentOf>
int plan_staged_heads(const npore_bam *b, const RecFetch &rf, int64_t n, const int32_t *fasta_of_ref, int n_fasta, const RecSpec &rec, int form,
                      const int64_t *seq_off, int64_t *raw_off, int64_t *hp, int64_t *bound, ExtentOf extent_of)
{
    const bool records = form != STAGE_HEAD;
    raw_off[0] = 0;
    if (records) *bound = 0;
    for (int64_t k = 0; k < n; k++) {
        const RecView r = rec_of(rf, k);
        const int32_t rid = r.ref_id();
        const int fi = (rid >= 0 && rid < (int32_t)b->ref_names.size()) ? fasta_of_ref[rid] : -1;
        if (fi < 0 || fi >= n_fasta) return fail(NPORE_E_INVALID, "a selected read lies on a contig that is not in the FASTA");
        RecMeasures m{r.l_read_name(), r.l_seq(), seq_off[k + 1] - seq_off[k], 0, 0, staged_passes(r.p, rec.pass_mask) ? staged_pass_bytes(r.p) : 0};
        int64_t head = m.pass_bytes, hp_k = 0;
        if (!m.pass_bytes) {
            const RecCigar cg = rec_cigar(r);
            m.in_words = cg.n;
            m.aux = form == STAGE_FULL ? filter_aux(r.aux(), r.end(), nullptr, rec.oc()) : 0;
            head = staged_head_bytes(r, cg, records ? STAGE_QUALS : STAGE_HEAD, false) + m.aux;
            hp_k = !records ? 0 : form == STAGE_FULL ? m.aux : rec_hp(r);
        }
        raw_off[k + 1] = raw_off[k] + head;
        if (!records) continue;
        hp[k] = hp_k;
        *bound += record_bound(rec, m, extent_of(k));
    }
    return NPORE_OK;
}
int slot_pack_heads(const npore_bam *b, const int32_t *fasta_of_ref, int n_fasta, int threads, npore_batch_slot &s, const PipeMode &pm)
{
    const int64_t n = s.m;
    if (int rc = pm.bam ? s.hp_pin.ensure((size_t)n * 8 + 64) : 0) return rc;
    s.rec_cap = 0;
    slot_pack_sizes(s, threads, pm);
    s.rawo.assign((size_t)n + 1, 0);
    // (a batch's own final covers the read's reference positions and bases, no more: the size of its slot too)
    if (int rc = plan_staged_heads(b, s.rf, n, fasta_of_ref, n_fasta, pm.rec, pm.stage_form(), s.so.data(), s.rawo.data(),
                                   reinterpret_cast<int64_t *>(s.hp_pin.p), &s.rec_cap,
                                   [&](int64_t k) { return own_final_extent(s.ro[(size_t)k + 1] - s.ro[(size_t)k], s.so[(size_t)k + 1] - s.so[(size_t)k]); }))
        return rc;
    if (int rc = s.raw.ensure((size_t)s.rawo[(size_t)n] + 64)) return rc;
    const int64_t per = 16;
    parallel_for((n + per - 1) / per, threads, [&](int64_t t) {
        for (int64_t k = t * per; k < std::min(n, (t + 1) * per); k++) {
            char *dst = s.raw.p + s.rawo[(size_t)k];
            const size_t len = (size_t)(s.rawo[(size_t)k + 1] - s.rawo[(size_t)k]);
            stage_record(s.rf.ptr[(size_t)k], pm.stage_form(), reinterpret_cast<uint8_t *>(dst), pm.rec);
            cache_writeback(dst, len);         // page-locked staging about to cross PCIe: out of this core's cache first (hostio.hpp)
        }
    });
    return NPORE_OK;
}
int slot_pack(const npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, int threads, npore_batch_slot &s, const PipeMode &pm)
{
    return pm.dpack ? slot_pack_heads(b, fasta_of_ref, (int)fa->names.size(), threads, s, pm) : slot_pack_arrays(b, fa, fasta_of_ref, threads, s, pm);
}

// ---- enqueue: the packed batch to the device through the context's asynchronous path, s.done recorded behind it (returns once
// the batch's groups are enqueued; waits only when all work sets of the context are still busy) --------------------------------
struct AlignKnobs { float indel_start, indel_extend; int max_b_rows, r; };
int slot_enqueue(npore_ctx *ctx, npore_batch_slot &s, const PipeMode &pm, const AlignKnobs &q)
{
    const int64_t m = s.m;
    int rc = 0;
    if ((rc = s.olen_pin.ensure((size_t)m * 8 + 64)) || (rc = s.st_pin.ensure((size_t)m * 4 + 64))) return fail(rc, "batch buffers");
    if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) return fail(NPORE_E_HIP, "hipEventCreate");
    s.ctext_copied = 0;
    if (pm.dev_records()) {
        if ((rc = s.d_recs.ensure((size_t)s.rec_cap + 64)) || (rc = s.d_cursor.ensure(64)) || (rc = s.ctext_pin.ensure(64)) ||
            (rc = s.reclen_pin.ensure((size_t)m * 8 + 64)) || (rc = s.total_pin.ensure(64))) return fail(rc, "batch buffers");
        s.emit = BamEmit{};
        s.emit.rec = pm.rec;
        s.emit.d_recs = s.d_recs.as<uint8_t>(); s.emit.cap = s.rec_cap; s.emit.d_cursor = s.d_cursor.as<unsigned long long>();
        s.emit.h_hp = reinterpret_cast<const int64_t *>(s.hp_pin.p); s.emit.h_rec_len = reinterpret_cast<int64_t *>(s.reclen_pin.p);
        s.emit.h_total = reinterpret_cast<unsigned long long *>(s.total_pin.p);
        if (pm.dev_deflate()) {
            if ((rc = slot_deflate_buffers(s, s.rec_cap, pm.deflate))) return fail(rc, "batch buffers");
            s.emit.dfl = slot_deflate_params(s, s.d_recs.as<uint8_t>(), s.d_cursor.as<unsigned long long>(), ctx->d_stream_pos.as<unsigned long long>(),
                                             pm.deflate);
            s.emit.deflate = true; s.emit.h_sizes = reinterpret_cast<uint32_t *>(s.sizes_pin.p); s.emit.h_info = reinterpret_cast<int64_t *>(s.info_pin.p);
        }
    } else if (pm.glue) {
        // device glue: the texts come back compacted -- the front of the batch's compact buffer (0.5 bytes per base are sent with the
        // batch's last group; usual reads need a quarter of that) and the reads' offsets (a text takes whole 16-byte granules)
        const int64_t slots = s.oo[(size_t)m] + 16 * m, bound = std::min(slots, slots / 4 + 4096);
        if ((rc = s.d_ctext.ensure((size_t)slots + 64)) || (rc = s.d_cursor.ensure(64)) || (rc = s.ctext_pin.ensure((size_t)bound + 64)) ||
            (rc = s.coff_pin.ensure((size_t)m * 8 + 64))) return fail(rc, "batch buffers");
        s.cmp = TextCompact{s.d_ctext.as<uint8_t>(), s.d_cursor.as<unsigned long long>(), slots, reinterpret_cast<int64_t *>(s.coff_pin.p), s.ctext_pin.p, bound};
        s.ctext_copied = bound;
    }
    AlignArgs a = host_batch_args(m, s.ro.data(), s.so.data(), s.co.data(), q.indel_start, q.indel_extend, q.max_b_rows, q.r,
                                  pm.glue ? s.ctext_pin.p : s.alns.p /* (with the compaction nothing is copied there) */, s.oo.data(),
                                  reinterpret_cast<int64_t *>(s.olen_pin.p), reinterpret_cast<int32_t *>(s.st_pin.p));
    if (pm.dpack) {
        a.h_raw = reinterpret_cast<uint8_t *>(s.raw.p); a.h_raw_off = s.rawo.data();
        a.d_ctg = ctx->d_ctg.as<CtgEntry>(); a.n_ctg = ctx->n_ctg;
    } else {
        a.h_refs = reinterpret_cast<uint8_t *>(s.refs.p); a.h_seqs = reinterpret_cast<uint8_t *>(s.seqs.p); a.h_cigs = s.cigs.p;
    }
    a.final_text = pm.glue;
    if (pm.dev_records()) a.bam = &s.emit;
    else if (pm.glue) a.compact = &s.cmp;
    if ((rc = align_batch(ctx, a, false))) return rc;
    return hipEventRecord(s.done, ctx->s_post) == hipSuccess ? NPORE_OK : fail(NPORE_E_HIP, "hipEventRecord");
}

// ---- collect: what the device left of the batch (s.olen, status) into what the writer takes (s.sam / s.recs_pin, s.meta) ------
// BAM mode, records built on the device: nothing is formatted here -- the batch's bytes as they lie there, into page-locked
// memory, and from the records' lengths what the writer's index needs (reference, position and span are the input record's)
// What the emit kernels left of n records, wherever it is fetched (below, the debug entry): no length negative (a record that
// did not fit), the lengths add up to the cursor, the cursor within the buffer's bound
int check_record_sizes(const int64_t *len, int64_t n, int64_t total, int64_t bound)
{
    if (total < 0 || total > bound) return fail(NPORE_E_HIP, "internal: BAM record buffer overflow");
    int64_t sum = 0;
    for (int64_t k = 0; k < n; k++) {
        if (len[k] < 0) return fail(NPORE_E_HIP, "internal: BAM record buffer overflow");
        sum += len[k];
    }
    return sum == total ? NPORE_OK : fail(NPORE_E_HIP, "internal: BAM record sizes do not add up");
}
int slot_fetch_records(const int32_t *status, npore_batch_slot &s, const PipeMode &pm)
{
    const int64_t total = (int64_t)*reinterpret_cast<const unsigned long long *>(s.total_pin.p);
    const int64_t *len = reinterpret_cast<const int64_t *>(s.reclen_pin.p);
    if (int rc = check_record_sizes(len, s.m, total, s.rec_cap)) return rc;
    s.meta.clear();
    for (int64_t k = 0; k < s.m; k++) {
        if ((len[k] == 0) != ((status[k] & NPORE_ST_BAD_INPUT) != 0)) return fail(NPORE_E_HIP, "internal: BAM records and status bits disagree");
        if (len[k] == 0) continue;
        const RecView r = rec_of(s.rf, k);
        // (a record that passed gave align() no reference slice: the index takes the input record's own reference length)
        const int64_t span = staged_passes(r.p, pm.rec.pass_mask) ? rec_ref_len(r) : s.ro[(size_t)k + 1] - s.ro[(size_t)k];
        s.meta.push_back(BamRecMeta{r.ref_id(), r.pos(), span, len[k]});
    }
    const char *src = s.d_recs.p;
    int64_t bytes = total;
    if (pm.dev_deflate()) {          // exactly the coded members and the two raw fragments around them
        const int64_t *info = reinterpret_cast<const int64_t *>(s.info_pin.p);
        const int64_t nm = info[0], comp = info[1], head = info[2], tail = info[3];
        if (nm < 0 || nm > s.max_members || head < 0 || tail < 0 || head + nm * (int64_t)BGZF_STORED_PAYLOAD + tail != total || comp < 0 ||
            comp > nm * (int64_t)(BGZF_STORED_PAYLOAD + BGZF_STORED_OVERHEAD))
            return fail(NPORE_E_HIP, "internal: the coded members do not add up to the batch's bytes");
        std::copy(info, info + 4, s.frag);
        src = s.d_comp.p;            // (one copy: the fragments lie behind the last member -- emit_deflate_kernel)
        bytes = comp + head + tail;
    }
    if (int rc = s.recs_pin.ensure((size_t)bytes + 64)) return rc;
    if (bytes > 0) HIP_TRY(hipMemcpy(s.recs_pin.p, src, (size_t)bytes, hipMemcpyDeviceToHost));
    s.sam_len = total;
    return NPORE_OK;
}
// realign_read's glue (src/bam.pyx:65-78) where the device has not done it (*ms_std, else left as it is: how long that took), and the SAM lines or
// (BAM mode) the host twin's records; reads refused by align() have no string and get an empty CIGAR
int slot_collect(const npore_bam *b, const int32_t *status, int threads, npore_batch_slot &s, const PipeMode &pm, double *ms_std)
{
    if (pm.dev_records()) return slot_fetch_records(status, s, pm);
    const int64_t n = s.m;
    const ReadCodes codes{pm.rec, reinterpret_cast<const uint8_t *>(s.refs.p), s.ro.data(), reinterpret_cast<const uint8_t *>(s.seqs.p), s.so.data()};
    auto format_into = [&](const char *finals, const int64_t *final_off) {          // (FULL records: NM and MD from the slot's code arrays)
        return pm.bam ? format_bam_into(b, s.rf, n, finals, final_off, s.flen.data(), status, threads, s.sam, &s.sam_len, &s.meta, codes)
                      : format_sam_into(b, s.rf, n, finals, final_off, s.flen.data(), status, threads, s.sam, &s.sam_len);
    };
    if (pm.glue) {          // the device has left the final CIGAR texts (standardize_kernel), compacted: the front of that buffer is here
        const int64_t *coff = reinterpret_cast<const int64_t *>(s.coff_pin.p);
        int64_t extent = 0;
        for (int64_t k = 0; k < n; k++) {
            const int64_t l = s.flen[(size_t)k] = std::max<int64_t>(s.olen[(size_t)k], 0);
            if (l > 0 && coff[k] < 0) return fail(NPORE_E_HIP, "internal: compact text buffer overflow");
            if (l > 0) extent = std::max(extent, coff[k] + l);
        }
        if (extent > s.ctext_copied) {        // (texts far longer than usual -- 0.5 bytes per base were sent with the batch: the rest is fetched now)
            if (int rc = s.ctext_pin.ensure((size_t)extent + 64)) return rc;
            HIP_TRY(hipMemcpy(s.ctext_pin.p, s.d_ctext.p, (size_t)extent, hipMemcpyDeviceToHost));
            s.ctext_copied = extent;
        }
        return format_into(s.ctext_pin.p, coff);
    }
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t *refs = reinterpret_cast<const uint8_t *>(s.refs.p), *seqs = reinterpret_cast<const uint8_t *>(s.seqs.p);
    parallel_for(n, threads, [&](int64_t k) {
        const int64_t l = s.olen[(size_t)k] > 0 ? s.olen[(size_t)k] : 0;
        s.flen[(size_t)k] = standardize_collapsed_into(s.alns.p + s.oo[(size_t)k], l, refs + s.ro[(size_t)k],     // 2 bytes per op + 16 always suffice
                                                       s.ro[(size_t)k + 1] - s.ro[(size_t)k], seqs + s.so[(size_t)k],
                                                       s.so[(size_t)k + 1] - s.so[(size_t)k], s.finals.p + s.fo[(size_t)k]);
    });
    *ms_std = ms_since(t0);
    return format_into(s.finals.p, s.fo.data());
}

// The BAM -> SAM pipeline over a stream of batches, in batch_order.hpp's order.  A batch is enqueued the moment it is packed and that
// call returns at once, so up to N_SETS batches are on the device, the upload / preparation of one and the traceback / download of
// another beside the fill kernel of a third (run_core); six slots cover two batches being packed, three on the device and one being
// written.  acquire(k, slot) -> records of batch k now in slot.rf (< 0: fail() called);  on_status(k, m, status bits): in front of its text.
template <class Acquire, class OnStatus>
int file_pipeline(npore_ctx *ctx, npore_bam *b, const npore_fasta *fa, const int32_t *fasta_of_ref, const AlignKnobs &knobs, int threads, RunOutput &out,
                  bool serial_acquire, Acquire acquire, OnStatus on_status)
{
    // (run_core refuses them too, but on a worker thread: refuse here, before a batch is read or a record written)
    if (!std::isfinite(knobs.indel_start) || !std::isfinite(knobs.indel_extend)) return fail(NPORE_E_INVALID, "indel_start and indel_extend must be finite");
    const auto wall0 = std::chrono::steady_clock::now();
    for (auto &sp : ctx->slots) {
        if (!sp) sp = new npore_batch_slot();
        std::fill(sp->t_ms, sp->t_ms + 6, 0.0);
    }
    ctx->file_mark[0] = ctx->totals[0] + ctx->totals[1] + ctx->totals[2];
    ctx->file_mark[1] = ctx->totals[3] + ctx->totals[4];
    // Several batches are in the host stages at once (two being packed, up to two being written): each stage gets half of the
    // CPUs, so that the process does not run five times as many busy threads as it has CPUs -- under a cgroup quota that ends in
    // the whole process being throttled for the rest of the scheduling period (NPORE_PACK_THREADS / NPORE_POST_THREADS override)
    auto stage_threads = [&](const char *name) { const char *e = std::getenv(name); return std::max(1, e ? std::atoi(e) : host_threads(threads) / 2); };
    const int pack_threads = stage_threads("NPORE_PACK_THREADS"), post_threads = stage_threads("NPORE_POST_THREADS");
    const PipeMode pm = pipe_mode(ctx, out);
    if (int rc = pm.dpack ? device_fasta(ctx, b, fa, fasta_of_ref) : 0) return rc;
    if (pm.dev_deflate()) {          // the run's stream position starts at 0
        if (int rc = ctx->d_stream_pos.ensure(64)) return rc;
        HIP_TRY(hipMemset(ctx->d_stream_pos.p, 0, 8));
    }
    const bool trace = std::getenv("NPORE_PIPE_TRACE") != nullptr;      // one line per batch and stage boundary on stderr (ms since the call began)
    std::mutex trace_m;
    auto mark = [&](const char *what, int64_t k) {
        if (!trace) return;
        const double ms = ms_since(wall0);
        std::lock_guard<std::mutex> lk(trace_m);
        std::fprintf(stderr, "pipe %8.2f ms  batch %3lld  %s\n", ms, (long long)k, what);
    };
    // (a stage's message is its thread's: into the slot with it)
    auto kept = [](npore_batch_slot &s, int64_t rc) { if (rc < 0) s.err = npore_last_error(); return rc; };
    auto timed = [](double &ms, auto &&stage) { const auto t0 = std::chrono::steady_clock::now(); const auto rc = stage(); ms += ms_since(t0); return rc; };
    auto status_of = [](const npore_batch_slot &s) { return reinterpret_cast<const int32_t *>(s.st_pin.p); };
    std::string err;
    int rc = run_batches_in_order(
        ctx->slots, npore_ctx::N_SLOTS, serial_acquire, NPORE_E_NOMEM,
        [&](int64_t k, npore_batch_slot &s) { s.keep.clear(); return timed(s.t_ms[0], [&] { return kept(s, acquire(k, s)); }); },
        [&](int64_t, npore_batch_slot &s) { return timed(s.t_ms[0], [&] { return (int)kept(s, slot_pack(b, fa, fasta_of_ref, pack_threads, s, pm)); }); },
        [&](int64_t, npore_batch_slot &s) { return (int)kept(s, slot_enqueue(ctx, s, pm, knobs)); },
        [&](int64_t k, npore_batch_slot &s) {
            (void)hipSetDevice(ctx->device);
            if (timed(s.t_ms[1], [&] { return hipEventSynchronize(s.done); }) != hipSuccess) { s.err = "waiting for a batch failed"; return (int)NPORE_E_HIP; }
            mark("device done", k);
            std::memcpy(s.olen.data(), s.olen_pin.p, (size_t)s.m * 8);
            if (pm.rec.pass_mask) {          // NPORE_ST_PASSED: not realigned, written as it came (the device left these reads' status 0)
                int32_t *st = reinterpret_cast<int32_t *>(s.st_pin.p);
                for (int64_t q = 0; q < s.m; q++)
                    if (staged_passes(rec_of(s.rf, q).p, pm.rec.pass_mask)) st[q] |= NPORE_ST_PASSED;
            }
            double ms_std = 0.0, ms_all = 0.0;
            const int rcc = timed(ms_all, [&] { return (int)kept(s, slot_collect(b, status_of(s), post_threads, s, pm, &ms_std)); });
            s.t_ms[2] += ms_std; s.t_ms[3] += ms_all - ms_std;
            if (!rcc) mark("text made", k);
            return rcc;
        },
        [&](int64_t k, npore_batch_slot &s) {
            on_status(k, s.m, status_of(s));
            const int rcw = timed(s.t_ms[4], [&] { return (int)kept(s, out.write(s, pm)); });
            s.keep.clear();
            return rcw;
        },
        mark, err);
    if (const int rcw = npore_ctx_wait(ctx))                  // stage clocks of every group; a failure found while a work set was recycled
        if (rc == NPORE_OK) { rc = rcw; err = npore_last_error(); }
    // stage clocks of this call: sums over the batches of the time each stage's thread spent (stages of
    // neighbouring batches overlap, so the sums exceed the wall time), the wall time, and the GPU's share
    std::fill(b->file_ms, b->file_ms + 8, 0.0);
    for (auto &sp : ctx->slots) {
        sp->keep.clear();
        for (int q = 0; q < 5; q++) b->file_ms[q] += sp->t_ms[q];
    }
    b->file_ms[5] = ms_since(wall0);
    b->file_ms[6] = ctx->totals[0] + ctx->totals[1] + ctx->totals[2] - ctx->file_mark[0];     // stage clocks of the device path (prep + fill + traceback;
    b->file_ms[7] = ctx->totals[3] + ctx->totals[4] - ctx->file_mark[1];                     // H2D + D2H): SUMS over groups that run beside each other
    return rc == NPORE_OK ? NPORE_OK : fail(rc, err);
}
}  // namespace
