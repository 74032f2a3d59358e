// bam_emit_kernels.hpp -- the realigned reads as BAM records, built on the device (the file pipeline's BAM mode).
//
// bam_reader.hpp states the record and holds the host twin (bam_record_into).  Almost everything a record needs is on
// the device already: the input record up to the end of its qualities (what unpack_records_kernel reads, uploaded a
// little further in this mode), and the final CIGAR, which standardize_words_kernel (kernels.hpp) leaves as
// `len << 4 | op` words in the read's slot.  launch_bam_emit, at the end of this file, states what runs per group of reads,
// behind its standardisation, on the traceback stream.  Either form is a placement and an assembly:
//   place_bam_*_kernel  one workgroup: every kept read's size and a scan over the sizes -- the group's records lie one after
//                       the other, in input order, behind those of the batch's groups before it (a cursor that the groups,
//                       which follow each other on one stream, hand on);
//   emit_bam_*_kernel   one wavefront per read: fixed fields, name, CIGAR words, bases, qualities, tags.
// The reference form (place_bam_records_kernel, emit_bam_records_kernel) writes the 4-bit bases from the leading soft clip on
// (an odd clip moves every nibble), the quality slice and the HP tag.  FULL records (NPORE_OUT_FULL, bam_reader.hpp FULL
// RECORD; place_bam_full_kernel, emit_bam_full_kernel) keep clips and aux and end in tags made from the final CIGAR, each by a
// kernel in front of the placement, which needs its size, and, where it is a text, one behind the assembly, which writes it:
//   NM       nm_count_kernel                   (nm_rec.hpp)
//   MD       md_size_kernel, emit_md_kernel    (md_rec.hpp, NPORE_OUT_MD): ONE walk, md_walk, launched with two sinks
//   cs, de   cs_size_kernel, emit_cs_kernel    (cs_rec.hpp, NPORE_TAG_*): ONE walk, cs_walk, likewise
// and, the same way, in the CIGAR's =/X form where that is asked for:
//   =/X      eqx_size_kernel, emit_eqx_kernel  (eqx_rec.hpp, NPORE_CIGAR_EQX): ONE walk, eqx_walk, likewise -- the placement
//                                              takes the number of split words, the assembly leaves their span to the walk
// and the read's ORIGINAL CIGAR where the run changed it and that is asked for:
//   OC       oc_size_kernel, emit_oc_kernel    (oc_rec.hpp, NPORE_TAG_OC): changed or not is decided in front of the placement, which
//                                              the host could not do -- it never sees the final words; ONE walk, oc_walk, likewise
// What these share stands once: which reads get no such tags is bam_no_tags; where every part of a FULL record lies, and so
// its size, is BamFullShape's *_at members (a new tag is a size in bam_full_shape and one more *_at); what a tag's emit kernel
// starts from is bam_tag_shape.  The walks over the FINAL words of NM and =/X are a pick and a visit body under one wave frame
// (cigar_tiles, differ_round, since_mark; wave_incl_sum also serves OC's two).  md_walk and cs_walk keep the same loop written
// out: under the frame their kernels measured 2 - 3 % slower ("the emit chain's own time").
// A final CIGAR of more than 65 535 operations goes out as htslib writes it (bam_reader.hpp RECORD): two placeholder words
// in the CIGAR's place, the real words in a CG:B,I tag behind the other tags, in either form.
// The host then takes the batch's bytes as they lie (BgzfStoredWriter) and the records' lengths for its index.
// All run beside the next batch's fill kernel and keep to what the other light kernels keep to: at most
// 64 vector registers; the placement's 2 KB of LDS are less than a fill workgroup leaves free, the others have none.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/npore_amd.h"
#include "cs_rec.hpp"
#include "eqx_rec.hpp"
#include "md_rec.hpp"
#include "nm_rec.hpp"
#include "oc_rec.hpp"
#include "unpack_kernels.hpp"

namespace npore {

struct BamEmitParams {
    const uint8_t *raw;            // the group's staged heads (hostio.hpp stage_record_head), with the qualities
    const int64_t *raw_off;        // [n_reads + 1]
    const int64_t *ref_off;        // [n_reads + 1]: reference length of read k = ref_off[k + 1] - ref_off[k]
    const int64_t *seq_off;        // [n_reads + 1]: bases without the soft clips
    const int64_t *hp;             // [n_reads] the HP tag's value (0: none); FULL records: the bytes of kept aux behind the qualities
    const uint8_t *words;          // the slots: the final CIGAR as words (standardize_words_kernel)
    const int64_t *words_off;      // [reads of the target + 1]
    const int64_t *words_len;      // bytes of words per read (<= 0: none)
    const int32_t *status;
    int64_t read_base, n_reads;    // this group's reads within words_off / words_len / status
    uint8_t *recs;                 // the batch's record buffer
    int64_t cap;
    unsigned long long *cursor;    // bytes of it in use
    int64_t *rec_off;              // [n_reads] of this group: where the read's record begins
    int64_t *rec_len;              // [n_reads]: its bytes (0: the read is not written; -1: no room)
    // FULL records only (nm_count_kernel): the group's code arrays, which ref_off / seq_off index, and the reads' NM
    const uint8_t *refs = nullptr, *seqs = nullptr;
    int32_t *nm = nullptr;         // [n_reads]
    int32_t *md_len = nullptr;     // [n_reads] NPORE_OUT_MD (md_size_kernel): bytes of the read's MD text; null: no MD tag
    // NPORE_TAG_* (cs_size_kernel): which of cs / de follow MD, the bytes of the read's cs text, its de value
    int tags = 0;
    int32_t *cs_len = nullptr;     // [n_reads], with any tag (0 without NPORE_TAG_CS)
    float *de = nullptr;           // [n_reads], with any tag
    // FULL records, npore_bam_set_output_pass: reads whose staged flag has one of these bits pass (staged_head.hpp) -- their staged
    // head is the whole input record and so is their output record; nm, md_len, cs_len and de are 0 for them
    uint32_t pass_mask = 0;
    // NPORE_CIGAR_EQX (eqx_size_kernel): the words of the read's final CIGAR in =/X form (0 for a refused or passing read); null:
    // the final words go out as they are
    int32_t *eqx_len = nullptr;    // [n_reads]
    // NPORE_TAG_OC (oc_size_kernel): the bytes of the read's OC text (0: the read is refused, passes or did not change -- no tag);
    // null: no OC tags
    int32_t *oc_len = nullptr;     // [n_reads]
};

__device__ __forceinline__ void st32(uint8_t *q, uint32_t w)      // little-endian, unaligned
{
    q[0] = (uint8_t)w; q[1] = (uint8_t)(w >> 8); q[2] = (uint8_t)(w >> 16); q[3] = (uint8_t)(w >> 24);
}

__device__ __forceinline__ int bam_hp_bytes(int64_t hp)
{
    if (hp >= 0) return hp <= 0xFF ? 1 : hp <= 0xFFFF ? 2 : 4;
    return hp >= -128 ? 1 : hp >= -32768 ? 2 : 4;
}

__device__ __forceinline__ uint32_t bam_reg2bin_dev(int64_t beg, int64_t end)      // SAM specification 5.3
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}

// more operations than n_cigar_op holds: placeholder + CG tag
__device__ __forceinline__ bool bam_long_cigar(int64_t words_bytes) { return words_bytes > 4 * 0xFFFF; }

// size of read k's record (0: not written -- NPORE_ST_BAD_INPUT, as format_sam_into leaves the line out)
__device__ __forceinline__ int64_t bam_record_size(const BamEmitParams &p, int64_t k)
{
    const int64_t g = p.read_base + k;
    if (p.status[g] & 32) return 0;
    const uint8_t *f = p.raw + p.raw_off[k] + 4;
    const int64_t sl = p.seq_off[k + 1] - p.seq_off[k], wl = p.words_len[g] > 0 ? p.words_len[g] : 0;
    return 36 + (int64_t)f[8] + wl + (sl + 1) / 2 + sl + 3 + bam_hp_bytes(p.hp[k]) + (bam_long_cigar(wl) ? 16 : 0);
}

__device__ __forceinline__ int64_t bam_full_record_size(const BamEmitParams &p, int64_t k);

// one workgroup of 256: every thread sizes a contiguous share of the reads; their places follow from the sums of the shares
template <bool FULL>
__device__ __forceinline__ void place_records(const BamEmitParams &p)
{
    __shared__ int64_t s_sum[257];
    const int t = threadIdx.x;
    const int64_t n = p.n_reads, seg = (n + 255) / 256;
    const int64_t k0 = min(n, t * seg), k1 = min(n, k0 + seg);
    int64_t mine = 0;
    for (int64_t k = k0; k < k1; k++) mine += FULL ? bam_full_record_size(p, k) : bam_record_size(p, k);
    s_sum[t + 1] = mine;
    __syncthreads();
    if (t == 0) {
        s_sum[0] = (int64_t)*p.cursor;
        for (int q = 1; q <= 256; q++) s_sum[q] += s_sum[q - 1];
        *p.cursor = (unsigned long long)s_sum[256];
    }
    __syncthreads();
    int64_t at = s_sum[t];
    for (int64_t k = k0; k < k1; k++) {
        const int64_t sz = FULL ? bam_full_record_size(p, k) : bam_record_size(p, k);
        p.rec_off[k] = at;
        p.rec_len[k] = at + sz <= p.cap ? sz : -1;
        at += sz;
    }
}
__global__ __launch_bounds__(256) void place_bam_records_kernel(BamEmitParams p) { place_records<false>(p); }
__global__ __launch_bounds__(256) void place_bam_full_kernel(BamEmitParams p) { place_records<true>(p); }

// dst[j] = src[j] (NIB == 0) or the bytes one nibble further on, src[j] << 4 | src[j + 1] >> 4 (NIB == 1), j in [0, n),
// by the 64 lanes of a wavefront: four bytes per store where dst is aligned, each from two aligned words of the source;
// bytes in front of the first aligned word and behind the last whole one singly.  NIB == 1 reads src[n]; both sides read
// whole words around [src, src + n + NIB): the buffers they lie in end 64 bytes behind their last record.
// clear_low: the low nibble of the last byte is 0 (an odd number of bases).
template <int NIB>
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, int64_t n, bool clear_low, int lane)
{
    auto one = [&](int64_t j) {
        uint32_t v = NIB ? ((uint32_t)src[j] << 4 | (uint32_t)src[j + 1] >> 4) : src[j];
        if (clear_low && j == n - 1) v &= 0xF0u;
        dst[j] = (uint8_t)v;
    };
    const int64_t head = min(n, (int64_t)((4 - ((uintptr_t)dst & 3)) & 3));
    const int64_t n_words = (n - head) >> 2, tail = head + 4 * n_words;
    if (lane < head) one(lane);
    if (lane >= 60 && tail + (lane - 60) < n) one(tail + (lane - 60));
    const uint8_t *s0 = src + head;
    const int sa = (int)((uintptr_t)s0 & 3);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s0 - sa);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    for (int64_t w = lane; w < n_words; w += 64) {
        const uint64_t v = ((uint64_t)sw[w + 1] << 32 | sw[w]) >> (8 * sa);        // bytes 4w ... 4w + 4 of s0
        uint32_t o;
        if (NIB) o = ((uint32_t)v & 0x0F0F0F0Fu) << 4 | ((uint32_t)(v >> 8) >> 4 & 0x0F0F0F0Fu);
        else o = (uint32_t)v;
        if (clear_low && head + 4 * w + 4 == n) o &= 0xF0FFFFFFu;
        dw[w] = o;
    }
}

// one wavefront per read
__global__ __launch_bounds__(64) void emit_bam_records_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    if (k >= p.n_reads) return;
    const int lane = threadIdx.x;
    const int64_t size = p.rec_len[k];
    if (size <= 0) return;
    const int64_t g = p.read_base + k;
    const uint8_t *f = p.raw + p.raw_off[k] + 4;                 // the fixed fields (hostio.hpp RecView)
    const int32_t pos = (int32_t)ld32(f + 4);
    const int l_rn = f[8];
    const int64_t l_seq = (int32_t)ld32(f + 16);
    const uint8_t *cg, *sq;
    int nc;
    staged_cigar(f, cg, nc, sq);
    const uint8_t *ql = sq + (l_seq + 1) / 2;
    auto op_of = [&](int c) { return ld32(cg + 4 * (size_t)c); };
    int64_t lead = 0;                                            // (hostio.hpp rec_clips)
    if (nc >= 1 && (op_of(0) & 15u) == 4) lead = op_of(0) >> 4;
    if (nc > 1 && (op_of(0) & 15u) == 5 && (op_of(1) & 15u) == 4) lead = op_of(1) >> 4;
    const int64_t sl = p.seq_off[k + 1] - p.seq_off[k], reflen = p.ref_off[k + 1] - p.ref_off[k];
    const int64_t wl = p.words_len[g] > 0 ? p.words_len[g] : 0, nb = (sl + 1) / 2;
    const int64_t hp = p.hp[k];
    const int hb = bam_hp_bytes(hp);
    const bool lng = bam_long_cigar(wl);
    uint8_t *o = p.recs + p.rec_off[k];
    if (lane < 9) {                                              // block_size and the fixed fields, a word per lane
        uint32_t w = 0xFFFFFFFFu;                                // (next_refID, next_pos)
        switch (lane) {
            case 0: w = (uint32_t)(size - 4); break;
            case 1: w = ld32(f); break;
            case 2: w = (uint32_t)pos; break;
            case 3: w = (uint32_t)l_rn | (uint32_t)f[9] << 8 | bam_reg2bin_dev(pos, (int64_t)pos + max((int64_t)1, reflen)) << 16; break;
            case 4: w = (lng ? 2u : (uint32_t)(wl >> 2)) | ld16(f + 14) << 16; break;
            case 5: w = (uint32_t)sl; break;
            case 8: w = (uint32_t)reflen; break;
            default: break;
        }
        st32(o + 4 * lane, w);
    }
    o += 36;
    for (int j = lane; j < l_rn; j += 64) o[j] = f[32 + j];
    o += l_rn;
    if (lng) {                                                   // the placeholder: <l_seq>S<reflen>N
        if (lane < 2) {
            const uint32_t w = lane == 0 ? ((uint32_t)sl << 4 | 4u) : ((uint32_t)reflen << 4 | 3u);
            st32(o + 4 * lane, w);
        }
        o += 8;
    } else {
        wave_copy<0>(o, p.words + p.words_off[g], wl, false, lane);
        o += wl;
    }
    if (sl > 0) {
        if (lead & 1) wave_copy<1>(o, sq + (lead >> 1), nb, (sl & 1) != 0, lane);
        else wave_copy<0>(o, sq + (lead >> 1), nb, (sl & 1) != 0, lane);
        o += nb;
        if (ql[0] == 0xFF) for (int64_t j = lane; j < sl; j += 64) o[j] = 0xFF;
        else wave_copy<0>(o, ql + lead, sl, false, lane);
        o += sl;
    }
    if (lane == 0) {
        o[0] = 'H'; o[1] = 'P';
        o[2] = (uint8_t)(hp >= 0 ? (hb == 1 ? 'C' : hb == 2 ? 'S' : 'I') : (hb == 1 ? 'c' : hb == 2 ? 's' : 'i'));
        const uint32_t v = (uint32_t)(int32_t)hp;
        for (int q = 0; q < hb; q++) o[3 + q] = (uint8_t)(v >> (8 * q));
    }
    if (lng) {                                                   // CG:B,I behind HP: the count, then the words
        o += 3 + hb;
        if (lane < 4) o[lane] = (uint8_t)"CGBI"[lane];
        else if (lane < 8) o[lane] = (uint8_t)((uint32_t)(wl >> 2) >> (8 * (lane - 4)));
        wave_copy<0>(o + 8, p.words + p.words_off[g], wl, false, lane);
    }
}

// ---- the wave frame under the walks over a read's final CIGAR (NM, =/X; md_walk and cs_walk write the same loop out) ----
// One wavefront per read over tiles of 64 CIGAR words: lane l holds word l of the tile (`0M` behind the end), and inclusive wave
// sums of what the words consume place every word on the reference and on the query.  The sums fit 32 bits, a read has fewer
// than 2^31 operations; the slots lie at multiples of 4, so the words are read as words.  A walk is a PICK of the words it
// visits and the BODY of a visit (cigar_tiles); a compared word is taken 64 positions per round (differ_round); what a walk
// carries from round to round, word to word and tile to tile is the same in every lane.

// read k gets no tags made from its final CIGAR: it is refused and has no record, or it passes as it came (staged_head.hpp)
__device__ __forceinline__ bool bam_no_tags(const BamEmitParams &p, int64_t k)
{
    return (p.status[p.read_base + k] & 32) || staged_passes(p.raw + p.raw_off[k] + 4, p.pass_mask);
}

// read k's final words and the two code arrays they walk over
struct FinalWords {
    int64_t n;
    const uint32_t *w;
    const uint8_t *ref, *seq;
    int64_t rl, sl;
};
__device__ __forceinline__ FinalWords final_words(const BamEmitParams &p, int64_t k)
{
    const int64_t g = p.read_base + k;
    FinalWords r;
    r.n = p.words_len[g] <= 0 ? 0 : p.words_len[g] >> 2;
    r.w = reinterpret_cast<const uint32_t *>(p.words + p.words_off[g]);
    r.ref = p.refs + p.ref_off[k];
    r.seq = p.seqs + p.seq_off[k];
    r.rl = p.ref_off[k + 1] - p.ref_off[k];
    r.sl = p.seq_off[k + 1] - p.seq_off[k];
    return r;
}

// v summed over the lanes up to and including this one (uint32_t; 64 bits for oc_changed)
template <class T>
__device__ __forceinline__ T wave_incl_sum(T v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const T x = __shfl_up(v, d);
        if (lane >= d) v += x;
    }
    return v;
}

// pick(op, len) is asked once for every word of the read, in the lane that holds it -- so it is also where a per-lane tally goes
// (NM's bases under I and D).  The picked words of a tile are then visited in word order, all lanes together:
// visit(op, len, a, b) gets the word and where it begins on the reference and on the query, the same in every lane.
template <class Pick, class Visit>
__device__ __forceinline__ void cigar_tiles(const FinalWords &r, int lane, Pick pick, Visit visit)
{
    int64_t a0 = 0, b0 = 0;                  // consumed in front of the tile
    for (int64_t t0 = 0; t0 < r.n; t0 += 64) {
        const uint32_t v = t0 + lane < r.n ? r.w[t0 + lane] : 0u;
        const uint32_t op = v & 15u, len = v >> 4, use = nm_consumes(op);
        const uint32_t ra = (use & 1u) ? len : 0u, qa = (use & 2u) ? len : 0u;
        const uint32_t ri = wave_incl_sum(ra, lane), qi = wave_incl_sum(qa, lane);
        unsigned long long todo = __builtin_amdgcn_ballot_w64(pick(op, len));
        while (todo) {
            const int j = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            visit(__shfl(op, j), __shfl(len, j), a0 + __shfl(ri - ra, j), b0 + __shfl(qi - qa, j));
        }
        a0 += __shfl(ri, 63);
        b0 += __shfl(qi, 63);
    }
}

// one round of a compared word of lj positions that begins at (aj, bj): lane l looks at position q = q0 + l; in_round of the 64
// lie inside the word; d: this lane's position differs (nm_differs); ev: the lanes where it does
struct DifferRound {
    uint32_t q, in_round;
    bool d;
    unsigned long long ev;
};
__device__ __forceinline__ DifferRound differ_round(const FinalWords &r, int lane, uint32_t lj, int64_t aj, int64_t bj, uint32_t q0)
{
    DifferRound x;
    x.q = q0 + (uint32_t)lane;
    x.in_round = min(64u, lj - q0);
    x.d = x.q < lj && nm_differs(r.ref, r.rl, aj + x.q, r.seq, r.sl, bj + x.q);
    x.ev = __builtin_amdgcn_ballot_w64(x.d);
    return x;
}

// How far a stretch reaches back from position `at` of a round, given `below`, the round's marks below `at`: to the last of
// them -- OWN = 0: that mark's position counted (at - its position), =/X's runs begin AT a boundary; OWN = 1: not counted,
// MD's and cs's counts begin BEHIND a differing position -- and with none below, over the round's positions so far and the
// `carry` from the rounds before (carry + at).  at = the lane, below = marks & lanes_below(lane): the stretch that ends in front
// of the lane; at = in_round, below = all marks (none lies further up): the carry out of the round.
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }
template <int OWN>
__device__ __forceinline__ uint32_t since_mark(unsigned long long below, uint32_t at, uint32_t carry)
{
    return below ? at - (uint32_t)OWN - (uint32_t)(63 - (int)__builtin_clzll(below)) : carry + at;
}

// ---- FULL records (bam_reader.hpp FULL RECORD; host twin: bam_record_full_into) ------------------------------------------
// The staged head carries the kept aux bytes behind the qualities (hostio.hpp STAGE_FULL; p.hp[k]: how many), so bases,
// qualities and tags are ONE contiguous copy; the clip words come from the staged CIGAR; NM is counted by nm_count_kernel
// between the standardisation and the placement.

// NM (nm_rec.hpp) of every read of the group: I and D add their lengths in their lanes; an M run is a ballot + popcount a round.
__global__ __launch_bounds__(64) void nm_count_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    if (k >= p.n_reads) return;
    const int lane = threadIdx.x;
    uint32_t whole = 0, differ = 0;          // per lane: bases under I and D; the same in every lane: compared positions that count
    if (!bam_no_tags(p, k)) {
        const FinalWords r = final_words(p, k);
        cigar_tiles(
            r, lane,
            [&](uint32_t op, uint32_t len) {
                if (nm_counts_whole(op)) whole += len;
                return nm_compares(op) && len > 0;
            },
            [&](uint32_t, uint32_t lj, int64_t aj, int64_t bj) {
                for (uint32_t q0 = 0; q0 < lj; q0 += 64) differ += (uint32_t)__builtin_popcountll(differ_round(r, lane, lj, aj, bj, q0).ev);
            });
        for (int d = 32; d; d >>= 1) whole += __shfl_xor(whole, d);
    }
    if (lane == 0) p.nm[k] = (int32_t)(whole + differ);
}

// what both FULL kernels need of read k: the clip words [0, ci) and [cj, nc) of the staged CIGAR (bam_reader.hpp
// full_clip_words), the sizes of the parts, the record's size (0: not written)
struct BamFullShape {
    const uint8_t *f, *cg, *sq;
    int nc, ci, cj, nmb;
    bool lng, pass;                // pass: the record is the staged head's bytes (staged_head.hpp); only f and size are set
    int64_t wl, n_cig, l_seq, aux, size;      // wl: bytes of the final words as they go out (NPORE_CIGAR_EQX: of the split ones)
    int64_t mdb;                   // bytes of the MD tag behind NM (4 + its text; 0: none)
    int64_t csb, deb;              // bytes of the cs tag behind that (4 + its text; 0: none) and of the de tag (7; 0: none)
    int64_t ocb;                   // bytes of the OC tag behind those (4 + its text; 0: none)
    // THE RECORD'S LAYOUT, which the FULL kernels take from here: where each part begins, in bytes from the record's block_size word.
    // Every part lies behind the one before it, so a tag that has a size has a place, and the record ends behind the last.
    __device__ int64_t cigar_at() const { return 36 + (int64_t)f[8]; }                      // behind the fixed fields and the name
    __device__ int64_t body_at() const { return cigar_at() + (lng ? 8 : 4 * n_cig); }       // bases, qualities, kept aux (long: behind the placeholder)
    __device__ int64_t nm_at() const { return body_at() + (l_seq + 1) / 2 + l_seq + aux; }
    __device__ int64_t md_at() const { return nm_at() + 3 + nmb; }
    __device__ int64_t cs_at() const { return md_at() + mdb; }
    __device__ int64_t de_at() const { return cs_at() + csb; }
    __device__ int64_t oc_at() const { return de_at() + deb; }
    __device__ int64_t cg_at() const { return oc_at() + ocb; }                              // long only: C G B I, the count, the words
    __device__ int64_t words_at() const { return lng ? cg_at() + 8 : cigar_at(); }          // the CIGAR words, wherever they go
    __device__ int64_t end() const { return cg_at() + (lng ? 8 + 4 * n_cig : 0); }
};
// the clip words [0, ci) and [cj, nc) of a staged CIGAR's nc words at cg (bam_reader.hpp full_clip_words)
__device__ __forceinline__ void staged_clip_words(const uint8_t *cg, int nc, int &ci, int &cj)
{
    auto op_of = [&](int c) { return ld32(cg + 4 * (size_t)c) & 15u; };
    ci = 0;
    cj = nc;
    if (ci < cj && op_of(ci) == 5) ci++;
    if (ci < cj && op_of(ci) == 4) ci++;
    if (cj > ci && op_of(cj - 1) == 5) cj--;
    if (cj > ci && op_of(cj - 1) == 4) cj--;
}
__device__ __forceinline__ BamFullShape bam_full_shape(const BamEmitParams &p, int64_t k)
{
    BamFullShape s;
    const int64_t g = p.read_base + k;
    s.f = p.raw + p.raw_off[k] + 4;
    s.pass = staged_passes(s.f, p.pass_mask);
    if (s.pass) {
        s.size = (p.status[g] & 32) ? 0 : staged_pass_bytes(s.f);
        return s;
    }
    staged_cigar(s.f, s.cg, s.nc, s.sq);
    staged_clip_words(s.cg, s.nc, s.ci, s.cj);
    s.wl = p.eqx_len ? 4 * (int64_t)p.eqx_len[k] : p.words_len[g] > 0 ? p.words_len[g] : 0;
    s.n_cig = s.ci + (s.wl >> 2) + (s.nc - s.cj);
    s.lng = s.n_cig > 0xFFFF;
    s.l_seq = (int32_t)ld32(s.f + 16);
    s.aux = p.hp[k];
    const uint32_t nm = (uint32_t)p.nm[k];
    s.nmb = nm <= 0xFFu ? 1 : nm <= 0xFFFFu ? 2 : 4;
    s.mdb = p.md_len ? 4 + (int64_t)p.md_len[k] : 0;
    s.csb = (p.tags & NPORE_TAG_CS) ? 4 + (int64_t)p.cs_len[k] : 0;
    s.deb = (p.tags & NPORE_TAG_DE) ? 7 : 0;
    s.ocb = p.oc_len && p.oc_len[k] ? 4 + (int64_t)p.oc_len[k] : 0;
    s.size = (p.status[g] & 32) ? 0 : s.end();
    return s;
}
__device__ __forceinline__ int64_t bam_full_record_size(const BamEmitParams &p, int64_t k) { return bam_full_shape(p, k).size; }
// what a kernel that writes a tag into read k's placed record starts from: the record's shape; false: there is nothing to
// write -- no such read, no record, no room, or a record that passed as it came
__device__ __forceinline__ bool bam_tag_shape(const BamEmitParams &p, int64_t k, BamFullShape &s)
{
    if (k >= p.n_reads || p.rec_len[k] <= 0) return false;
    s = bam_full_shape(p, k);
    return !s.pass;
}

// one wavefront per read
__global__ __launch_bounds__(64) void emit_bam_full_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    if (k >= p.n_reads) return;
    const int lane = threadIdx.x;
    const int64_t size = p.rec_len[k];
    if (size <= 0) return;
    const int64_t g = p.read_base + k;
    const BamFullShape s = bam_full_shape(p, k);
    const uint8_t *f = s.f;
    if (s.pass) {                                                // the input record as it was staged, block_size word first
        wave_copy<0>(p.recs + p.rec_off[k], f - 4, size, false, lane);
        return;
    }
    const int32_t pos = (int32_t)ld32(f + 4);
    const int l_rn = f[8];
    const int64_t reflen = p.ref_off[k + 1] - p.ref_off[k];
    uint8_t *rec = p.recs + p.rec_off[k];                        // every part at its place of the shape's map
    if (lane < 9) {                                              // block_size and the fixed fields, a word per lane: the input's but bin and n_cigar_op
        uint32_t w = ld32(f + 4 * (lane > 0 ? lane - 1 : 0));
        if (lane == 0) w = (uint32_t)(size - 4);
        if (lane == 3) w = (uint32_t)l_rn | (uint32_t)f[9] << 8 | bam_reg2bin_dev(pos, (int64_t)pos + max((int64_t)1, reflen)) << 16;
        if (lane == 4) w = (s.lng ? 2u : (uint32_t)s.n_cig) | ld16(f + 14) << 16;
        st32(rec + 4 * lane, w);
    }
    for (int j = lane; j < l_rn; j += 64) rec[36 + j] = f[32 + j];
    uint8_t *cw = rec + s.words_at();                            // where the CIGAR words go
    if (s.lng) {                                                 // the placeholder in the CIGAR's place, CG:B,I behind NM (and MD, cs, de, OC)
        if (lane < 2) st32(rec + s.cigar_at() + 4 * lane, lane == 0 ? ((uint32_t)s.l_seq << 4 | 4u) : ((uint32_t)reflen << 4 | 3u));
        if (lane >= 4 && lane < 8) cw[lane - 12] = (uint8_t)"CGBI"[lane - 4];
        if (lane >= 8 && lane < 12) cw[lane - 12] = (uint8_t)((uint32_t)s.n_cig >> (8 * (lane - 8)));
    }
    wave_copy<0>(cw, s.cg, 4 * (int64_t)s.ci, false, lane);
    if (!p.eqx_len) wave_copy<0>(cw + 4 * s.ci, p.words + p.words_off[g], s.wl, false, lane);      // (=/X form: emit_eqx_kernel's span)
    wave_copy<0>(cw + 4 * s.ci + s.wl, s.cg + 4 * (int64_t)s.cj, 4 * (int64_t)(s.nc - s.cj), false, lane);
    wave_copy<0>(rec + s.body_at(), s.sq, s.nm_at() - s.body_at(), false, lane);      // bases, qualities, kept aux: as they lie in the staged head
    if (lane == 0) {
        uint8_t *o = rec + s.nm_at();
        const uint32_t nm = (uint32_t)p.nm[k];
        o[0] = 'N'; o[1] = 'M';
        o[2] = (uint8_t)(s.nmb == 1 ? 'C' : s.nmb == 2 ? 'S' : 'I');
        for (int q = 0; q < s.nmb; q++) o[3 + q] = (uint8_t)(nm >> (8 * q));
    }
}

// ---- the MD tag of a FULL record (NPORE_OUT_MD; md_rec.hpp states the rule and holds the sequential twin) ----------------
// One wavefront per read over tiles of 64 CIGAR words, as nm_count_kernel: lane l holds word l, wave prefix sums place every
// word on both arrays, the M-type and D words are visited in word order.  `at` (bytes of text so far) and `u` (matches
// since the last item) are the same in every lane.
//   M word, 64 positions per round: the ballot of nm_differs gives the events.  An event lane's count is the distance to
//     the previous set bit of the round (the round's first event: u + its lane), its bytes digits(count) + 1, its place a
//     wave prefix sum of those bytes over the event lanes; the carry out is u + the round's positions where the round has no
//     event, otherwise the positions behind the last event.
//   D word: the count's digits and '^' by lane 0, then the letters with the lanes striding over them.
// The walk is ONE function over a sink (md_rec.hpp): md_size_kernel runs it with MdCount, emit_md_kernel with MdStore, so
// size and text cannot differ.  Returns the text's length (no NUL).
template <class Sink>
__device__ __forceinline__ uint32_t md_walk(const BamEmitParams &p, int64_t k, int lane, const Sink &sink)
{
    const int64_t g = p.read_base + k;
    const int64_t n = p.words_len[g] <= 0 ? 0 : p.words_len[g] >> 2;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p.words + p.words_off[g]);      // (the slots lie at multiples of 4)
    const uint8_t *ref = p.refs + p.ref_off[k], *seq = p.seqs + p.seq_off[k];
    const int64_t rl = p.ref_off[k + 1] - p.ref_off[k], sl = p.seq_off[k + 1] - p.seq_off[k];
    const unsigned long long below_me = (1ull << lane) - 1ull;
    int64_t a0 = 0, b0 = 0;                  // consumed in front of the tile
    uint32_t at = 0, u = 0;
    for (int64_t t0 = 0; t0 < n; t0 += 64) {
        const uint32_t v = t0 + lane < n ? w[t0 + lane] : 0u;       // (behind the end: `0M`)
        const uint32_t op = v & 15u, len = v >> 4, use = nm_consumes(op);
        const uint32_t ra = (use & 1u) ? len : 0u, qa = (use & 2u) ? len : 0u;
        uint32_t ri = ra, qi = qa;           // inclusive sums over the tile
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t x = (uint32_t)__shfl_up((int)ri, d), y = (uint32_t)__shfl_up((int)qi, d);
            if (lane >= d) { ri += x; qi += y; }
        }
        unsigned long long runs = __builtin_amdgcn_ballot_w64((nm_compares(op) || op == 2u) && len > 0);
        while (runs) {
            const int j = (int)__builtin_ctzll(runs);
            runs &= runs - 1;
            const uint32_t lj = (uint32_t)__shfl((int)len, j), opj = (uint32_t)__shfl((int)op, j);
            const int64_t aj = a0 + (uint32_t)__shfl((int)(ri - ra), j), bj = b0 + (uint32_t)__shfl((int)(qi - qa), j);
            if (opj == 2u) {
                const int nd = md_digits(u);
                if (lane == 0) {
                    md_put_decimal(sink, at, u, nd);
                    sink.put(at + nd, (uint8_t)'^');
                }
                at += (uint32_t)nd + 1u;
                for (uint32_t q = (uint32_t)lane; q < lj; q += 64) sink.put(at + q, md_letter(code_at(ref, rl, aj + q)));
                at += lj;
                u = 0;
                continue;
            }
            for (uint32_t q0 = 0; q0 < lj; q0 += 64) {
                const uint32_t q = q0 + (uint32_t)lane, in_round = min(64u, lj - q0);
                const bool d = q < lj && nm_differs(ref, rl, aj + q, seq, sl, bj + q);
                const unsigned long long ev = __builtin_amdgcn_ballot_w64(d);
                if (!ev) { u += in_round; continue; }
                const unsigned long long before = ev & below_me;
                const uint32_t cnt = before ? (uint32_t)(lane - 1 - (63 - (int)__builtin_clzll(before))) : u + (uint32_t)lane;
                const int nd = md_digits(cnt);
                const uint32_t bytes = d ? (uint32_t)nd + 1u : 0u;
                uint32_t incl = bytes;
                for (int s = 1; s < 64; s <<= 1) {
                    const uint32_t x = (uint32_t)__shfl_up((int)incl, s);
                    if (lane >= s) incl += x;
                }
                if (d) {
                    const uint32_t mine = at + incl - bytes;
                    md_put_decimal(sink, mine, cnt, nd);
                    sink.put(mine + nd, md_letter(code_at(ref, rl, aj + q)));
                }
                at += (uint32_t)__shfl((int)incl, 63);
                u = in_round - 1u - (uint32_t)(63 - (int)__builtin_clzll(ev));
            }
        }
        a0 += (uint32_t)__shfl((int)ri, 63);
        b0 += (uint32_t)__shfl((int)qi, 63);
    }
    const int nd = md_digits(u);
    if (lane == 0) md_put_decimal(sink, at, u, nd);
    return at + (uint32_t)nd;
}

// bytes of every read's MD text (0: the read gets no tags), between nm_count_kernel and the placement
__global__ __launch_bounds__(64) void md_size_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    if (k >= p.n_reads) return;
    const int lane = threadIdx.x;
    const uint32_t len = bam_no_tags(p, k) ? 0u : md_walk(p, k, lane, MdCount{});
    if (lane == 0) p.md_len[k] = (int32_t)len;
}

// 'M' 'D' 'Z' text NUL at the record's md_at, behind emit_bam_full_kernel on its stream
__global__ __launch_bounds__(64) void emit_md_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    BamFullShape s;
    if (!bam_tag_shape(p, k, s)) return;
    uint8_t *o = p.recs + p.rec_off[k] + s.md_at();
    if (lane < 3) o[lane] = (uint8_t)"MDZ"[lane];
    const int64_t cap = p.md_len[k];
    md_walk(p, k, lane, MdStore{o + 3, cap});
    if (lane == 0) o[3 + cap] = 0;
}

// ---- the cs and de tags of a FULL record (NPORE_TAG_CS / NPORE_TAG_DE; cs_rec.hpp states the rule and holds the sequential twin) ----
// md_walk's frame: one wavefront per read over tiles of 64 CIGAR words, the M-type, I, D and N words of a tile visited in word
// order; `at` (bytes of text so far), `u` (the open stretch's positions, carried across words and tiles) and the counts E X G
// are the same in every lane.
//   I / D word: the open stretch's `:count` (short form) by lane 0, the sign by lane 0, then a lane per base, codes to letters,
//     64 bases per round.  N only ends the stretch.
//   M-type word, 64 positions per round, the ballot of nm_differs gives the differing lanes.  Every lane knows the bytes of its
//     own item and a wave prefix sum of those bytes places it:
//       short form: a differing lane writes `:count` -- the distance to the previous differing lane of the round, u + its lane
//         for the round's first; nothing when that is 0 -- and `*` and its two letters;
//       long form: a differing lane writes its three bytes, every other lane its reference letter, with `=` in front where
//         the lane before it differs (lane 0: where no stretch is open).
//     The carry out is u + the round's positions where nothing differs, otherwise the positions behind the last differing one.
// The walk is ONE function over a sink: cs_size_kernel runs it with MdCount, emit_cs_kernel with MdStore, so size and text
// cannot differ.  Returns the text's length (no NUL), the counts in c.
template <bool LNG, class Sink>
__device__ __forceinline__ uint32_t cs_walk(const BamEmitParams &p, int64_t k, int lane, const Sink &sink, CsCounts &c)
{
    const int64_t g = p.read_base + k;
    const int64_t n = p.words_len[g] <= 0 ? 0 : p.words_len[g] >> 2;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p.words + p.words_off[g]);      // (the slots lie at multiples of 4)
    const uint8_t *ref = p.refs + p.ref_off[k], *seq = p.seqs + p.seq_off[k];
    const int64_t rl = p.ref_off[k + 1] - p.ref_off[k], sl = p.seq_off[k + 1] - p.seq_off[k];
    const unsigned long long below_me = (1ull << lane) - 1ull;
    int64_t a0 = 0, b0 = 0;                  // consumed in front of the tile
    uint32_t at = 0, u = 0;
    auto end_stretch = [&]() {
        if (!LNG && u > 0) {
            const int nd = md_digits(u);
            if (lane == 0) {
                sink.put(at, (uint8_t)':');
                md_put_decimal(sink, at + 1u, u, nd);
            }
            at += 1u + (uint32_t)nd;
        }
        u = 0;
    };
    for (int64_t t0 = 0; t0 < n; t0 += 64) {
        const uint32_t v = t0 + lane < n ? w[t0 + lane] : 0u;       // (behind the end: `0M`)
        const uint32_t op = v & 15u, len = v >> 4, use = nm_consumes(op);
        const uint32_t ra = (use & 1u) ? len : 0u, qa = (use & 2u) ? len : 0u;
        uint32_t ri = ra, qi = qa;           // inclusive sums over the tile
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t x = (uint32_t)__shfl_up((int)ri, d), y = (uint32_t)__shfl_up((int)qi, d);
            if (lane >= d) { ri += x; qi += y; }
        }
        unsigned long long runs = __builtin_amdgcn_ballot_w64((nm_compares(op) || (op >= 1u && op <= 3u)) && len > 0);
        while (runs) {
            const int j = (int)__builtin_ctzll(runs);
            runs &= runs - 1;
            const uint32_t lj = (uint32_t)__shfl((int)len, j), opj = (uint32_t)__shfl((int)op, j);
            const int64_t aj = a0 + (uint32_t)__shfl((int)(ri - ra), j), bj = b0 + (uint32_t)__shfl((int)(qi - qa), j);
            if (!nm_compares(opj)) {
                end_stretch();
                if (opj == 3u) continue;
                if (lane == 0) sink.put(at, (uint8_t)(opj == 1u ? '+' : '-'));
                at += 1u;
                const uint8_t *arr = opj == 1u ? seq : ref;
                const int64_t al = opj == 1u ? sl : rl, from = opj == 1u ? bj : aj;
                for (uint32_t q = (uint32_t)lane; q < lj; q += 64) sink.put(at + q, cs_lower(code_at(arr, al, from + q)));
                at += lj;
                c.g++;
                continue;
            }
            for (uint32_t q0 = 0; q0 < lj; q0 += 64) {
                const uint32_t q = q0 + (uint32_t)lane, in_round = min(64u, lj - q0);
                const bool d = q < lj && nm_differs(ref, rl, aj + q, seq, sl, bj + q);
                const unsigned long long ev = __builtin_amdgcn_ballot_w64(d);
                const uint32_t n_ev = (uint32_t)__builtin_popcountll(ev);
                c.x += n_ev;
                c.e += in_round - n_ev;
                if (!LNG && !ev) { u += in_round; continue; }
                const unsigned long long before = ev & below_me;
                uint32_t cnt = 0, bytes = 0;
                int nd = 0;
                if (LNG) {
                    const bool opens = lane == 0 ? u == 0u : ((ev >> (lane - 1)) & 1ull) != 0;
                    bytes = q >= lj ? 0u : d ? 3u : opens ? 2u : 1u;
                } else {
                    cnt = before ? (uint32_t)(lane - 1 - (63 - (int)__builtin_clzll(before))) : u + (uint32_t)lane;
                    nd = md_digits(cnt);
                    bytes = d ? 3u + (cnt > 0u ? 1u + (uint32_t)nd : 0u) : 0u;
                }
                uint32_t incl = bytes;
                for (int s = 1; s < 64; s <<= 1) {
                    const uint32_t x = (uint32_t)__shfl_up((int)incl, s);
                    if (lane >= s) incl += x;
                }
                uint32_t mine = at + incl - bytes;
                if (d) {
                    if (!LNG && cnt > 0u) {
                        sink.put(mine, (uint8_t)':');
                        md_put_decimal(sink, mine + 1u, cnt, nd);
                        mine += 1u + (uint32_t)nd;
                    }
                    sink.put(mine, (uint8_t)'*');
                    sink.put(mine + 1u, cs_lower(code_at(ref, rl, aj + q)));
                    sink.put(mine + 2u, cs_lower(code_at(seq, sl, bj + q)));
                } else if (LNG && q < lj) {
                    if (bytes == 2u) sink.put(mine, (uint8_t)'=');
                    sink.put(mine + bytes - 1u, md_letter(code_at(ref, rl, aj + q)));
                }
                at += (uint32_t)__shfl((int)incl, 63);
                u = ev ? in_round - 1u - (uint32_t)(63 - (int)__builtin_clzll(ev)) : u + in_round;
            }
        }
        a0 += (uint32_t)__shfl((int)ri, 63);
        b0 += (uint32_t)__shfl((int)qi, 63);
    }
    end_stretch();
    return at;
}

// bytes of every read's cs text and its de value (0, 0.0f: the read gets no tags), beside md_size_kernel in front of the
// placement; only NPORE_TAG_DE: the walk runs for the counts and the size stays 0
__global__ __launch_bounds__(64) void cs_size_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    if (k >= p.n_reads) return;
    const int lane = threadIdx.x;
    CsCounts c;
    uint32_t len = 0;
    if (!bam_no_tags(p, k)) len = (p.tags & NPORE_TAG_CS_LONG) ? cs_walk<true>(p, k, lane, MdCount{}, c) : cs_walk<false>(p, k, lane, MdCount{}, c);
    if (lane == 0) {
        p.cs_len[k] = (p.tags & NPORE_TAG_CS) ? (int32_t)len : 0;
        p.de[k] = de_of_counts(c.e, c.x, c.g);
    }
}

// 'c' 's' 'Z' text NUL at the record's cs_at and 'd' 'e' 'f' value at its de_at, behind emit_bam_full_kernel (and emit_md_kernel)
// on its stream
__global__ __launch_bounds__(64) void emit_cs_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    BamFullShape s;
    if (!bam_tag_shape(p, k, s)) return;
    if (s.csb) {
        uint8_t *o = p.recs + p.rec_off[k] + s.cs_at();
        if (lane < 3) o[lane] = (uint8_t)"csZ"[lane];
        const int64_t cap = p.cs_len[k];
        CsCounts c;
        if (p.tags & NPORE_TAG_CS_LONG) cs_walk<true>(p, k, lane, MdStore{o + 3, cap}, c);
        else cs_walk<false>(p, k, lane, MdStore{o + 3, cap}, c);
        if (lane == 0) o[3 + cap] = 0;
    }
    if (s.deb) {
        uint8_t *o = p.recs + p.rec_off[k] + s.de_at();
        const uint32_t bits = __float_as_uint(p.de[k]);
        if (lane < 3) o[lane] = (uint8_t)"def"[lane];
        else if (lane < 7) o[lane] = (uint8_t)(bits >> (8 * (lane - 3)));
    }
}

// ---- the =/X form of a FULL record's CIGAR (NPORE_CIGAR_EQX; eqx_rec.hpp states the rule and holds the sequential twin) ----
// Every word of length > 0 is visited.  The open run (`cls`, its op, and `run`, its positions; run == 0: none) and `cnt` (words
// out so far) are the same in every lane and are carried across rounds, words and tiles.
//   a word that is not compared: lane 0 closes the open run -- its word at cnt -- and copies the word behind it.
//   M-type word: a round's ballot gives every lane's class and the class of the lane below it (lane 0: the open run's).  A lane
//     whose class differs from the one below is a BOUNDARY: it writes the run that ends in front of it -- the class below, the
//     positions from the previous boundary of the round on (the round's first boundary: run + its lane) -- at cnt + the
//     boundaries below it.  The carry out: the last position's class; run + the round's positions where the round has no
//     boundary, otherwise the positions from the last boundary on.
// The walk is ONE function over a sink (eqx_rec.hpp): eqx_size_kernel runs it with EqxCount, emit_eqx_kernel with EqxStore, so
// count and words cannot differ.  Returns the number of words.
template <class Sink>
__device__ __forceinline__ uint32_t eqx_walk(const BamEmitParams &p, int64_t k, int lane, const Sink &sink)
{
    const FinalWords r = final_words(p, k);
    uint32_t cnt = 0, run = 0, cls = EQX_EQ;
    auto close_run = [&]() {
        if (run > 0) {
            if (lane == 0) sink.put(cnt, run << 4 | cls);
            cnt++;
        }
        run = 0;
    };
    cigar_tiles(
        r, lane, [](uint32_t, uint32_t len) { return len > 0; },
        [&](uint32_t opj, uint32_t lj, int64_t aj, int64_t bj) {
            if (!nm_compares(opj)) {
                close_run();
                if (lane == 0) sink.put(cnt, lj << 4 | opj);
                cnt++;
                return;
            }
            for (uint32_t q0 = 0; q0 < lj; q0 += 64) {
                const DifferRound x = differ_round(r, lane, lj, aj, bj, q0);
                const unsigned long long valid = x.in_round < 64u ? (1ull << x.in_round) - 1ull : ~0ull;
                const bool opens = run > 0 && cls != ((x.ev & 1ull) ? EQX_X : EQX_EQ);       // lane 0 ends the carried run
                const unsigned long long bd = ((x.ev ^ (x.ev << 1)) & valid & ~1ull) | (opens ? 1ull : 0ull);
                if ((bd >> lane) & 1ull) {
                    const uint32_t below = lane == 0 ? cls : ((x.ev >> (lane - 1)) & 1ull) ? EQX_X : EQX_EQ;
                    const uint32_t slot = cnt + (uint32_t)__builtin_popcountll(bd & lanes_below(lane));
                    sink.put(slot, since_mark<0>(bd & lanes_below(lane), (uint32_t)lane, run) << 4 | below);
                }
                cnt += (uint32_t)__builtin_popcountll(bd);
                run = since_mark<0>(bd, x.in_round, run);
                cls = ((x.ev >> (x.in_round - 1u)) & 1ull) ? EQX_X : EQX_EQ;
            }
        });
    close_run();
    return cnt;
}

// words of every read's final CIGAR in =/X form (0: the read gets no tags), beside md_size_kernel and cs_size_kernel in front
// of the placement, which takes the record's n_cigar_op, its CG decision and its size from it (bam_full_shape)
__global__ __launch_bounds__(64) void eqx_size_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    if (k >= p.n_reads) return;
    const int lane = threadIdx.x;
    const uint32_t cnt = bam_no_tags(p, k) ? 0u : eqx_walk(p, k, lane, EqxCount{});
    if (lane == 0) p.eqx_len[k] = (int32_t)cnt;
}

// the split words between the record's clip words, in the CIGAR field or (long) behind CG:B,I's count: the span that
// emit_bam_full_kernel, in front of this one on its stream, left out
__global__ __launch_bounds__(64) void emit_eqx_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    BamFullShape s;
    if (!bam_tag_shape(p, k, s)) return;
    eqx_walk(p, k, lane, EqxStore{p.recs + p.rec_off[k] + s.words_at() + 4 * s.ci, (int64_t)p.eqx_len[k]});
}

// ---- the OC tag of a FULL record (NPORE_TAG_OC; oc_rec.hpp states the rule and holds the sequential twins) --------------------
// One wavefront per read over tiles of 64 words of the read's STAGED CIGAR (staged_cigar: its real words), tile t holding the
// words [64 t, 64 t + 64), lane l word 64 t + l; the clip words [0, ci) and [cj, nc) as bam_full_shape finds them.

// CHANGED: the parallel form of oc_changed_words.  A lane is LIVE where its word lies in [ci, cj) and has length > 0.  A live lane
// BEGINS a run where its mapped op differs from the previous live word's -- the previous live lane of the tile, or the open run
// carried in (op `rop`; `runs`, the runs begun so far, 0: none).  The run a lane belongs to has the index runs + (begins at or
// below the lane) - 1; a run's length within the tile is a difference of the exclusive prefix sums (64 bits) at the two lanes
// that begin it and the next.  A lane that begins a run CLOSES the one in front of it and compares it -- op, length, index -- with
// its final word; the open run (rop, rlen, its index runs - 1) is carried wave-uniformly and closed at the end, where the count
// is compared with nf.  The first difference ends the walk: the answer is the same in every lane.
__device__ __forceinline__ bool oc_changed(const BamEmitParams &p, int64_t k, int lane, const uint8_t *cg, int ci, int cj)
{
    const int64_t g = p.read_base + k;
    const int64_t nf = p.words_len[g] <= 0 ? 0 : p.words_len[g] >> 2;
    const uint32_t *fin = reinterpret_cast<const uint32_t *>(p.words + p.words_off[g]);      // (the slots lie at multiples of 4)
    const unsigned long long below_me = (1ull << lane) - 1ull;
    int64_t runs = 0;
    uint32_t rop = 0;
    unsigned long long rlen = 0;
    for (int64_t t0 = 0; t0 < cj; t0 += 64) {
        const int64_t c = t0 + lane;
        const bool in = c >= ci && c < cj;
        const uint32_t v = in ? ld32(cg + 4 * c) : 0u;
        const uint32_t op = oc_canon_op(v & 15u), len = v >> 4;
        const unsigned long long live = __builtin_amdgcn_ballot_w64(len > 0);
        if (!live) continue;
        const unsigned long long before = live & below_me;
        const int prev = before ? 63 - (int)__builtin_clzll(before) : 0;
        const uint32_t op_prev = (uint32_t)__shfl((int)op, prev);
        const bool begins = len > 0 && (before ? op != op_prev : (runs == 0 || op != rop));
        const unsigned long long bd = __builtin_amdgcn_ballot_w64(begins);
        const unsigned long long incl = wave_incl_sum((unsigned long long)len, lane);      // of the lengths over the tile
        const unsigned long long excl = incl - len, whole = (unsigned long long)__shfl((long long)incl, 63);
        // the run in front of a lane that begins one: from the previous beginning of the tile, or the carried one
        const unsigned long long bd_before = bd & below_me;
        const int from = bd_before ? 63 - (int)__builtin_clzll(bd_before) : 0;
        const unsigned long long excl_from = (unsigned long long)__shfl((long long)excl, from);
        const int64_t closed = runs + (int64_t)__builtin_popcountll(bd_before) - 1;      // its index (-1: there is none)
        bool differs = false;
        if (begins && closed >= 0) {
            const unsigned long long length = bd_before ? excl - excl_from : rlen + excl;
            const uint32_t cop = before ? op_prev : rop;
            const uint32_t f = closed < nf ? fin[closed] : 0u;
            differs = closed >= nf || (f & 15u) != cop || (unsigned long long)(f >> 4) != length;
        }
        if (__builtin_amdgcn_ballot_w64(differs)) return true;
        if (bd) {
            const int last = 63 - (int)__builtin_clzll(bd);
            rop = (uint32_t)__shfl((int)op, last);
            rlen = whole - (unsigned long long)__shfl((long long)excl, last);
            runs += (int64_t)__builtin_popcountll(bd);
        } else {
            rlen += whole;
        }
    }
    if (runs != nf) return true;
    if (runs == 0) return false;
    const uint32_t f = fin[runs - 1];
    return (f & 15u) != rop || (unsigned long long)(f >> 4) != rlen;
}

// TEXT: every word of the tile is its lane's -- digits(length) + 1 bytes at a wave prefix sum of those bytes behind `at`, the bytes
// of the tiles before (the same in every lane).  The walk is ONE function over a sink (oc_rec.hpp): oc_size_kernel runs it with
// OcCount, emit_oc_kernel with OcStore, so size and text cannot differ.  Returns the text's length (no NUL).
template <class Sink>
__device__ __forceinline__ uint32_t oc_walk(const uint8_t *cg, int nc, int lane, const Sink &sink)
{
    uint32_t at = 0;
    for (int64_t t0 = 0; t0 < nc; t0 += 64) {
        const bool in = t0 + lane < nc;
        const uint32_t v = in ? ld32(cg + 4 * (t0 + lane)) : 0u;
        const int nd = md_digits(v >> 4);
        const uint32_t bytes = in ? (uint32_t)nd + 1u : 0u, incl = wave_incl_sum(bytes, lane);
        if (in) {
            const uint32_t mine = at + incl - bytes;
            md_put_decimal(sink, mine, v >> 4, nd);
            sink.put(mine + nd, oc_letter(v & 15u));
        }
        at += __shfl(incl, 63);
    }
    return at;
}

// bytes of every read's OC text (0: the read gets no tags or did not change), beside the other size kernels in front of the
// placement, which takes the tag's bytes from it (bam_full_shape)
__global__ __launch_bounds__(64) void oc_size_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    if (k >= p.n_reads) return;
    const int lane = threadIdx.x;
    uint32_t len = 0;
    if (!bam_no_tags(p, k)) {
        const uint8_t *cg, *sq;
        int nc, ci, cj;
        staged_cigar(p.raw + p.raw_off[k] + 4, cg, nc, sq);
        staged_clip_words(cg, nc, ci, cj);
        if (oc_changed(p, k, lane, cg, ci, cj)) len = oc_walk(cg, nc, lane, OcCount{});
    }
    if (lane == 0) p.oc_len[k] = (int32_t)len;
}

// 'O' 'C' 'Z' text NUL at the record's oc_at, behind emit_bam_full_kernel (and emit_md_kernel, emit_cs_kernel) on its stream;
// byte stores: the tag has any alignment
__global__ __launch_bounds__(64) void emit_oc_kernel(BamEmitParams p)
{
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    BamFullShape s;
    if (!bam_tag_shape(p, k, s) || !s.ocb) return;
    uint8_t *o = p.recs + p.rec_off[k] + s.oc_at();
    const int64_t cap = s.ocb - 4;
    if (lane < 3) o[lane] = (uint8_t)"OCZ"[lane];
    oc_walk(s.cg, s.nc, lane, OcStore{o + 3, cap});
    if (lane == 0) o[3 + cap] = 0;
}

// What a group's records take, in order, on stream s: the reference form's two kernels, or (full) the FULL form's with the tags
// that p names -- p.md_len: MD; p.tags' NPORE_TAG_CS / NPORE_TAG_DE: cs / de; p.oc_len: OC -- and (p.eqx_len) the CIGAR's =/X form.
inline void launch_bam_emit(const BamEmitParams &p, bool full, hipStream_t s)
{
    const dim3 reads((unsigned)p.n_reads), wave(64);             // one wavefront per read; the placements: one workgroup
    if (!full) {
        hipLaunchKernelGGL(place_bam_records_kernel, dim3(1), dim3(256), 0, s, p);
        hipLaunchKernelGGL(emit_bam_records_kernel, reads, wave, 0, s, p);
        return;
    }
    const bool cs_de = (p.tags & (NPORE_TAG_CS | NPORE_TAG_DE)) != 0;
    hipLaunchKernelGGL(nm_count_kernel, reads, wave, 0, s, p);
    if (p.md_len) hipLaunchKernelGGL(md_size_kernel, reads, wave, 0, s, p);
    if (cs_de) hipLaunchKernelGGL(cs_size_kernel, reads, wave, 0, s, p);
    if (p.eqx_len) hipLaunchKernelGGL(eqx_size_kernel, reads, wave, 0, s, p);
    if (p.oc_len) hipLaunchKernelGGL(oc_size_kernel, reads, wave, 0, s, p);
    hipLaunchKernelGGL(place_bam_full_kernel, dim3(1), dim3(256), 0, s, p);
    hipLaunchKernelGGL(emit_bam_full_kernel, reads, wave, 0, s, p);
    if (p.md_len) hipLaunchKernelGGL(emit_md_kernel, reads, wave, 0, s, p);
    if (cs_de) hipLaunchKernelGGL(emit_cs_kernel, reads, wave, 0, s, p);
    if (p.eqx_len) hipLaunchKernelGGL(emit_eqx_kernel, reads, wave, 0, s, p);
    if (p.oc_len) hipLaunchKernelGGL(emit_oc_kernel, reads, wave, 0, s, p);
}

}  // namespace npore
