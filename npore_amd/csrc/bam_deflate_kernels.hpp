// bam_deflate_kernels.hpp -- the file pipeline's BAM mode with NPORE_OUT_DEFLATE: the whole BGZF members that lie inside
// a batch's record bytes coded on the device, each ONE dynamic-Huffman block of literals by the rule of deflate_code.hpp.
//
// The batch's records lie contiguous on the device when its last emit_bam_records_kernel is done (bam_emit_kernels.hpp).
// Where the record stream's cuts fall in them follows from the stream position, 8 bytes on the device that the run
// resets when it opens and every batch advances by its bytes: the host enqueues without knowing earlier batches' totals.
// Three kernels behind the batch's last group, on the traceback stream, no host synchronisation between them:
//   plan_deflate_kernel   one wavefront per whole member: histogram and CRC-32 (every lane a 1 020-byte slice; the
//                         slices' CRC registers joined by multiplication with x^(8 * 1 020 * 2^s) modulo the CRC
//                         polynomial, six rounds of a shift-and-xor product), the used symbols ranked by (count,
//                         symbol) by all lanes, then deflate_plan_sorted -- the very code of the host twin -- on lane 0:
//                         code lengths, codes, the block header's bits, the member's exact size;
//   place_deflate_kernel  one workgroup: a scan over the members' sizes -- they lie one after the other, in order --,
//                         the numbers the host needs (members, their bytes, the two fragments), the stream position;
//   emit_deflate_kernel   one wavefront per member: BGZF header, block header, then 64 payload bytes per round: a wave
//                         prefix sum of their code lengths, the codes OR-ed into whole words in LDS, the full words
//                         stored aligned, a word per lane; end-of-block, padding, CRC-32, ISIZE.  A member that falls
//                         back to the stored block is copied.
// The bytes in front of the first cut and behind the last stay raw: the writer joins them with the neighbouring
// batches' and codes that one member on the host (bam_reader.hpp BgzfStoredWriter::add_coded).  Two more wavefronts of the
// emitting kernel copy them behind the last member, so that ONE copy brings the batch down (fetched by three copies, two
// of them a few KB from unaligned places, a batch took the post stage two to three times as long: DESIGN 7).
// All three run beside the next batch's fill kernel and keep to what the other light kernels keep to.
//
// NPORE_OUT_MATCH (DeflateParams::mode = DEFLATE_MODE_MATCH): the same three steps with two other kernels around the placing one:
//   plan_match_kernel     one wavefront per whole member.  First all of plan_deflate_kernel: the literals-only plan, h bytes.
//                         Then the rule's steps 1 to 4 in windows of 64 positions, a lane each: the hash, the bucket's most
//                         recent position of earlier windows from a table of 2^15 16-bit positions in a grow-only device
//                         buffer (set to "none" by the wavefront itself), the nearest equal hash inside the window from a
//                         ballot per lane's hash, the table brought up to date with the window's last position per bucket,
//                         the lane's match length eight bytes at a time.  The greedy chain is wave-uniform: a scalar
//                         position, the lane's length by v_readlane, the token starts as a 64-bit mask; the tokens
//                         (length << 16 | distance, or the literal) go to the member's token buffer in order, their symbols
//                         into the two histograms in LDS.  Then the shared planning code once more, with matches: m bytes,
//                         and the plan is replaced iff m < h and m < 65 285;
//   emit_match_kernel     one wavefront per member: a member whose plan has no tokens goes through emit_deflate_kernel's
//                         code; otherwise 64 tokens per round, each up to 48 bits (length code, its extra bits, distance
//                         code, its extra bits), the same prefix sum and OR into LDS words, up to 96 words a round.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bam_emit_kernels.hpp"
#include "deflate_code.hpp"

namespace npore {

// what the planning kernel leaves of a member for the emitting kernel
struct DeflateMemberPlan {
    uint32_t code[DEFLATE_NLL];        // length << 16 | bits (literals only: the first 257)
    uint32_t dcode[DEFLATE_NDIST];     // the distance codes (a block with matches)
    uint32_t hdr_bits, block_bytes;    // block_bytes 0: the stored block
    uint32_t crc, n_tokens;            // n_tokens > 0: a block with matches, of so many tokens
    uint8_t hdr[DEFLATE_HDR_CAP];      // the block header's bits
};

struct DeflateParams {
    const uint8_t *recs;               // the batch's record bytes (64 readable bytes behind them)
    const unsigned long long *total;   // ... and how many there are
    unsigned long long *stream_pos;    // where recs[0] lies in the run's record stream; place_deflate_kernel advances it
    DeflateMemberPlan *plans;          // [max_members]
    uint32_t *sizes;                   // [max_members] bytes of member k (0: no room)
    int64_t *off;                      // [max_members] where it lies in comp
    uint8_t *comp;                     // the members, one after the other; behind them the head and the tail fragment
    int64_t comp_cap, max_members;     // comp_cap: room for members (2 * 65 280 bytes more lie behind it for the fragments)
    int64_t *info;                     // [4] members, their bytes, bytes in front of the first cut, bytes behind the last
    int mode;                          // DEFLATE_MODE_HUFFMAN or DEFLATE_MODE_MATCH
    uint16_t *htab;                    // DEFLATE_MODE_MATCH: [max_members << 15] a member's bucket -> most recent position
    uint32_t *tokens;                  // DEFLATE_MODE_MATCH: [max_members * 65 280] a member's tokens
};

struct DeflateCuts { int64_t first, n_members, tail; };

// the cuts inside `total` bytes whose first lies at offset pos of the stream
__host__ __device__ __forceinline__ DeflateCuts deflate_cuts(uint64_t pos, int64_t total)
{
    const int64_t P = DEFLATE_MEMBER_PAYLOAD;
    const int64_t first = (P - (int64_t)(pos % (uint64_t)P)) % P;
    if (total < first) return DeflateCuts{total, 0, 0};
    const int64_t n = (total - first) / P;
    return DeflateCuts{first, n, total - first - n * P};
}

// step 1 of the code-length rule by all lanes, for the symbols of w.freq[0 .. NSYM): the rank of a used symbol is the number
// of used symbols with a smaller (count, symbol).  Returns how many are used; w.a / w.sym hold them in order.
template <int NSYM>
__device__ __forceinline__ int wave_rank_symbols(DeflateWork &w, int lane)
{
    static_assert(NSYM <= 5 * 64, "five symbols a lane");
    uint32_t key[5];
    int rank[5];
    int m = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int s = lane + 64 * j;
        const uint32_t f = s < NSYM ? w.freq[s] : 0u;
        key[j] = f ? f << 9 | (uint32_t)s : 0u;
        rank[j] = 0;
        m += __popcll(__ballot(f != 0));
    }
    for (int t = 0; t < NSYM; t++) {
        const uint32_t f = w.freq[t];
        if (!f) continue;
        const uint32_t kt = f << 9 | (uint32_t)t;
#pragma unroll
        for (int j = 0; j < 5; j++) rank[j] += kt < key[j] ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 5; j++)
        if (key[j]) { w.a[rank[j]] = key[j] >> 9; w.sym[rank[j]] = (uint16_t)(key[j] & 0x1FFu); }
    return m;
}

// The literals-only plan of the member at src into pl and size: histogram, CRC-32, code lengths, codes, header.  Returns
// the block's bytes (lane 0; at least 65 285: the member is stored).
__device__ __forceinline__ uint32_t plan_literal_member(DeflateWork &w, const uint8_t *src, DeflateMemberPlan &pl, uint32_t &size, int lane)
{
    constexpr int P = DEFLATE_MEMBER_PAYLOAD, SLICE = P / 64;
    for (int s = lane; s < DEFLATE_NSYM; s += 64) w.freq[s] = s == 256 ? 1u : 0u;
    __syncthreads();
    // histogram and the slice's CRC register (lane 0 carries the initial complement)
    uint32_t c = lane == 0 ? 0xFFFFFFFFu : 0u;
    {
        const uint8_t *q = src + (size_t)lane * SLICE;
        for (int j = 0; j < SLICE; j += 4) {
            uint32_t v;
            __builtin_memcpy(&v, q + j, 4);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t byte = (v >> (8 * b)) & 0xFFu;
                atomicAdd(&w.freq[byte], 1u);
                c = crc_byte(c, byte);
            }
        }
    }
    // the register of slices l .. l + 2d - 1 = that of l .. l + d - 1 times x^(8 * SLICE * d), plus that of the next d
    {
        constexpr uint32_t X0 = crc_xpow_bytes((uint64_t)SLICE), X1 = crc_xpow_bytes(2ull * SLICE), X2 = crc_xpow_bytes(4ull * SLICE),
                           X3 = crc_xpow_bytes(8ull * SLICE), X4 = crc_xpow_bytes(16ull * SLICE), X5 = crc_xpow_bytes(32ull * SLICE);
#pragma unroll
        for (int s = 0; s < 6; s++) {
            uint32_t b = s == 0 ? X0 : s == 1 ? X1 : s == 2 ? X2 : s == 3 ? X3 : s == 4 ? X4 : X5;
            const uint32_t other = (uint32_t)__shfl_down((int)c, 1 << s);
            uint32_t prod = 0;
            for (uint32_t m = 1u << 31; m; m >>= 1) {
                prod ^= b & (0u - (uint32_t)((c & m) != 0));
                b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
            }
            c = prod ^ other;
        }
    }
    __syncthreads();
    const int m = wave_rank_symbols<DEFLATE_NSYM>(w, lane);
    __syncthreads();
    uint32_t block = 0;
    if (lane == 0) {
        deflate_plan_sorted(w, m);
        block = deflate_block_bytes(w);
        const bool stored = block >= (uint32_t)P + 5;
        pl.hdr_bits = w.hdr_bits;
        pl.block_bytes = stored ? 0u : block;
        pl.crc = ~c;
        pl.n_tokens = 0;
        size = stored ? (uint32_t)P + 31u : block + 26u;
        if (!stored) deflate_header(w, pl.hdr);
    }
    __syncthreads();
    for (int s = lane; s < DEFLATE_NSYM; s += 64) pl.code[s] = w.freq[s];
    return block;
}

__global__ __launch_bounds__(64) void plan_deflate_kernel(DeflateParams p)
{
    constexpr int P = DEFLATE_MEMBER_PAYLOAD;
    __shared__ DeflateWork w;
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    const DeflateCuts cuts = deflate_cuts(*p.stream_pos, (int64_t)*p.total);
    if (k >= cuts.n_members || k >= p.max_members) return;
    plan_literal_member(w, p.recs + cuts.first + k * P, p.plans[k], p.sizes[k], lane);
}

// one wavefront per whole member: the literals-only plan, then the matches, their tokens and the plan with them
__global__ __launch_bounds__(64) void plan_match_kernel(DeflateParams p)
{
    constexpr int P = DEFLATE_MEMBER_PAYLOAD;
    __shared__ DeflateWork w;
    __shared__ uint32_t s_pick;
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    const DeflateCuts cuts = deflate_cuts(*p.stream_pos, (int64_t)*p.total);
    if (k >= cuts.n_members || k >= p.max_members) return;
    const uint8_t *src = p.recs + cuts.first + k * P;
    DeflateMemberPlan &pl = p.plans[k];
    const uint32_t h_block = plan_literal_member(w, src, pl, p.sizes[k], lane);
    uint16_t *tab = p.htab + ((size_t)k << DEFLATE_HASH_BITS);
    uint32_t *tok = p.tokens + (size_t)k * P;
    for (int j = lane; j < (2 << DEFLATE_HASH_BITS) / 16; j += 64) reinterpret_cast<uint4 *>(tab)[j] = make_uint4(~0u, ~0u, ~0u, ~0u);     // DEFLATE_NO_POS
    __syncthreads();                                                // (the codes have left w.freq; the table is seen by all lanes)
    for (int s = lane; s < DEFLATE_NLL; s += 64) w.freq[s] = 0;
    if (lane < DEFLATE_NDIST) w.dfreq[lane] = 0;
    __syncthreads();
    uint32_t at = 0, n_tok = 0;                                     // wave-uniform: where the parse stands, tokens so far
    for (uint32_t base = 0; base < (uint32_t)P; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        uint32_t word;
        __builtin_memcpy(&word, src + i, 4);
        const bool hashed = i + 4 <= (uint32_t)P;
        const uint32_t h = hashed ? deflate_hash(word) : 0x10000u + (uint32_t)lane;        // (unhashed: equal to nobody's)
        uint32_t c = hashed ? (uint32_t)tab[h] : DEFLATE_NO_POS;
        // the nearest lane below with the same hash hides the table's entry; a lane above takes the table's entry over
        uint64_t later = 0;
#pragma unroll 1
        for (int s = 0; s < 64; s++) {
            const uint32_t hs = (uint32_t)__builtin_amdgcn_readlane((int)h, s);
            const uint64_t same = __ballot(h == hs);
            const uint64_t below = same & ((1ull << s) - 1);
            if (below && lane == s) c = base + 63u - (uint32_t)__builtin_clzll(below);
            later |= (same >> s) > 1 ? 1ull << s : 0ull;
        }
        if (hashed && !((later >> lane) & 1)) tab[h] = (uint16_t)i;
        // the match length, eight bytes at a time (the bytes behind the member's end are readable and do not count)
        uint32_t len = 0;
        if (c != DEFLATE_NO_POS && i - c <= (uint32_t)DEFLATE_MAX_DIST) {
            const uint32_t cap = min((uint32_t)DEFLATE_MAX_MATCH, (uint32_t)P - i);
            while (len < cap) {
                uint64_t x, y;
                __builtin_memcpy(&x, src + c + len, 8);
                __builtin_memcpy(&y, src + i + len, 8);
                if (x != y) { len += (uint32_t)__builtin_ctzll(x ^ y) >> 3; break; }
                len += 8;
            }
            len = min(len, cap);
            if (len < (uint32_t)DEFLATE_MIN_MATCH) len = 0;
        }
        // the greedy chain through the window
        uint64_t starts = 0;
        while (at < base + 64) {
            const uint32_t l = at - base;
            const uint32_t ll = (uint32_t)__builtin_amdgcn_readlane((int)len, (int)l);
            starts |= 1ull << l;
            at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(at + (ll ? ll : 1u)));
        }
        if ((starts >> lane) & 1) {
            uint32_t t = word & 0xFFu;
            if (len) {
                t = len << 16 | (i - c);
                atomicAdd(&w.freq[deflate_len_symbol(len) & 0xFFFFu], 1u);
                atomicAdd(&w.dfreq[deflate_dist_symbol(i - c) & 0xFFu], 1u);
            } else {
                atomicAdd(&w.freq[t], 1u);
            }
            tok[n_tok + (uint32_t)__popcll(starts & ((1ull << lane) - 1))] = t;
        }
        n_tok += (uint32_t)__popcll(starts);
        __syncthreads();                                            // the table's new entries before the next window reads it
    }
    if (lane == 0) w.freq[256] = 1;
    __syncthreads();
    const int m = wave_rank_symbols<DEFLATE_NLL>(w, lane);
    __syncthreads();
    if (lane == 0) {
        deflate_plan_sorted(w, m, true);
        const uint32_t block = deflate_block_bytes(w);
        const bool pick = block < h_block && block < (uint32_t)P + 5;
        s_pick = pick ? 1u : 0u;
        if (pick) {
            pl.hdr_bits = w.hdr_bits;
            pl.block_bytes = block;
            pl.n_tokens = n_tok;
            p.sizes[k] = block + 26u;
            deflate_header(w, pl.hdr);
        }
    }
    __syncthreads();
    if (s_pick) {
        for (int s = lane; s < DEFLATE_NLL; s += 64) pl.code[s] = w.freq[s];
        if (lane < DEFLATE_NDIST) pl.dcode[lane] = w.dfreq[lane];
    }
}

// one workgroup of 256: the members' places, what the host needs to know, and the stream position behind the batch
__global__ __launch_bounds__(256) void place_deflate_kernel(DeflateParams p)
{
    __shared__ int64_t s_sum[257];
    const int t = threadIdx.x;
    const int64_t total = (int64_t)*p.total;
    const DeflateCuts cuts = deflate_cuts(*p.stream_pos, total);
    const int64_t n = min(cuts.n_members, p.max_members), seg = (n + 255) / 256;
    const int64_t k0 = min(n, t * seg), k1 = min(n, k0 + seg);
    int64_t mine = 0;
    for (int64_t k = k0; k < k1; k++) mine += p.sizes[k];
    s_sum[t + 1] = mine;
    __syncthreads();
    if (t == 0) {
        s_sum[0] = 0;
        for (int q = 1; q <= 256; q++) s_sum[q] += s_sum[q - 1];
    }
    __syncthreads();
    int64_t at = s_sum[t];
    for (int64_t k = k0; k < k1; k++) {
        const int64_t sz = p.sizes[k];
        p.off[k] = at;
        if (at + sz > p.comp_cap) p.sizes[k] = 0;
        at += sz;
    }
    if (t == 0) {
        p.info[0] = cuts.n_members;
        p.info[1] = s_sum[256];
        p.info[2] = cuts.first;
        p.info[3] = cuts.tail;
        *p.stream_pos += (unsigned long long)total;
    }
}

// the two fragments, raw, behind the last member: the wavefronts n_members and n_members + 1 of an emitting kernel
__device__ __forceinline__ void emit_fragments(const DeflateParams &p, int64_t k, int64_t n_members, int lane)
{
    const int64_t total = (int64_t)*p.total, head = p.info[2], tail = p.info[3];
    if (k == n_members && p.info[0] <= p.max_members) wave_copy<0>(p.comp + p.info[1], p.recs, head, false, lane);
    if (k == n_members + 1 && p.info[0] <= p.max_members) wave_copy<0>(p.comp + p.info[1] + head, p.recs + (total - tail), tail, false, lane);
}

// the BGZF header, CRC-32 and ISIZE of member k; returns where the member begins
__device__ __forceinline__ uint8_t *emit_member_frame(const DeflateParams &p, int64_t k, uint32_t size, const DeflateMemberPlan &pl, int lane)
{
    constexpr int P = DEFLATE_MEMBER_PAYLOAD;
    uint8_t *o = p.comp + p.off[k];
    if (lane < 18) o[lane] = lane < 16 ? bgzf_header_byte(lane) : (uint8_t)((size - 1) >> (8 * (lane - 16)));
    const uint32_t block = pl.block_bytes;
    uint8_t *trailer = o + 18 + (block ? block : (uint32_t)P + 5u);
    if (lane < 8) trailer[lane] = (uint8_t)((lane < 4 ? pl.crc : (uint32_t)P) >> (8 * (lane & 3)));
    return o;
}

// What leads a member's data bits: the stream goes out in aligned words; it begins at the last word boundary at or in front
// of the header's last whole byte, the (at most three) header bytes behind that boundary and the header's last bits in the
// first word.  Writes the header's bytes in front of that boundary.
struct DeflateLead { uint32_t *q; uint32_t carry, cbits; };
__device__ __forceinline__ DeflateLead emit_block_header(uint8_t *o, const DeflateMemberPlan &pl, int lane)
{
    const uint32_t hb = pl.hdr_bits >> 3;                           // (>= 4: 17 + 12 bits and five symbols at the least)
    const uint32_t back = (uint32_t)((uintptr_t)(o + 18 + hb) & 3);
    DeflateLead d;
    d.q = reinterpret_cast<uint32_t *>(o + 18 + hb - back);
    for (uint32_t j = lane; j < hb - back; j += 64) o[18 + j] = pl.hdr[j];
    d.carry = 0;
    d.cbits = 8 * back + (pl.hdr_bits & 7);
    for (uint32_t j = 0; j < back; j++) d.carry |= (uint32_t)pl.hdr[hb - back + j] << (8 * j);
    if (pl.hdr_bits & 7) d.carry |= (uint32_t)pl.hdr[hb] << (8 * back);
    return d;
}

// member k as the stored block or as the block of literals (s_code: DEFLATE_NSYM words, s_stage: 34)
__device__ __forceinline__ void emit_literal_member(const DeflateParams &p, int64_t k, uint32_t size, uint32_t *s_code, uint32_t *s_stage, int lane)
{
    constexpr int P = DEFLATE_MEMBER_PAYLOAD;
    const DeflateMemberPlan &pl = p.plans[k];
    const uint8_t *src = p.recs + p.info[2] + k * P;
    uint8_t *o = emit_member_frame(p, k, size, pl, lane);
    if (!pl.block_bytes) {
        if (lane < 5) o[18 + lane] = lane == 0 ? 1 : (uint8_t)((lane < 3 ? (uint32_t)P : ~(uint32_t)P) >> (8 * ((lane - 1) & 1)));
        wave_copy<0>(o + 23, src, P, false, lane);
        return;
    }
    for (int s = lane; s < DEFLATE_NSYM; s += 64) s_code[s] = pl.code[s];
    const DeflateLead lead = emit_block_header(o, pl, lane);
    uint32_t *q = lead.q;
    uint32_t carry = lead.carry, cbits = lead.cbits;
    __syncthreads();
    for (int it = 0; it <= P / 64; it++) {                          // (the last round: end-of-block alone)
        const int sym = it < P / 64 ? (int)src[it * 64 + lane] : lane == 0 ? 256 : -1;
        const uint32_t cd = sym >= 0 ? s_code[sym] : 0u;
        const uint32_t len = cd >> 16;
        uint32_t incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t T = cbits + (uint32_t)__shfl((int)incl, 63), nw = T >> 5;      // T <= 31 + 64 * 15: at most 30 whole words
        if (lane < 34) s_stage[lane] = lane == 0 ? carry : 0u;
        __syncthreads();
        if (len) {
            const uint32_t pos = cbits + incl - len;
            const uint64_t v = (uint64_t)(cd & 0xFFFFu) << (pos & 31);
            atomicOr(&s_stage[pos >> 5], (uint32_t)v);
            if (v >> 32) atomicOr(&s_stage[(pos >> 5) + 1], (uint32_t)(v >> 32));
        }
        __syncthreads();
        if ((uint32_t)lane < nw) q[lane] = s_stage[lane];
        carry = s_stage[nw];
        cbits = T & 31;
        q += nw;
        __syncthreads();
    }
    if ((uint32_t)lane < (cbits + 7) >> 3) reinterpret_cast<uint8_t *>(q)[lane] = (uint8_t)(carry >> (8 * lane));
}

// one wavefront per member
__global__ __launch_bounds__(64) void emit_deflate_kernel(DeflateParams p)
{
    __shared__ uint32_t s_code[DEFLATE_NSYM];
    __shared__ uint32_t s_stage[34];
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    const int64_t n_members = min(p.info[0], p.max_members);
    if (k >= n_members) { emit_fragments(p, k, n_members, lane); return; }
    const uint32_t size = p.sizes[k];
    if (size == 0) return;
    emit_literal_member(p, k, size, s_code, s_stage, lane);
}

// one wavefront per member; DEFLATE_MODE_MATCH
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void emit_match_kernel(DeflateParams p)
{
    constexpr int P = DEFLATE_MEMBER_PAYLOAD, STAGE = 100;          // a round: 31 + 64 * 48 bits at the most, 96 whole words
    __shared__ uint32_t s_code[DEFLATE_NLL];
    __shared__ uint32_t s_dcode[DEFLATE_NDIST];
    __shared__ uint32_t s_stage[STAGE];
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    const int64_t n_members = min(p.info[0], p.max_members);
    if (k >= n_members) { emit_fragments(p, k, n_members, lane); return; }
    const uint32_t size = p.sizes[k];
    if (size == 0) return;
    const DeflateMemberPlan &pl = p.plans[k];
    const uint32_t n_tok = pl.n_tokens;
    if (n_tok == 0) { emit_literal_member(p, k, size, s_code, s_stage, lane); return; }
    const uint32_t *tok = p.tokens + (size_t)k * P;
    uint8_t *o = emit_member_frame(p, k, size, pl, lane);
    for (int s = lane; s < DEFLATE_NLL; s += 64) s_code[s] = pl.code[s];
    if (lane < DEFLATE_NDIST) s_dcode[lane] = pl.dcode[lane];
    const DeflateLead lead = emit_block_header(o, pl, lane);
    uint32_t *q = lead.q;
    uint32_t carry = lead.carry, cbits = lead.cbits;
    __syncthreads();
    for (uint32_t t0 = 0; t0 <= n_tok; t0 += 64) {                  // (token n_tok: end-of-block)
        const uint32_t idx = t0 + (uint32_t)lane;
        uint64_t v = 0;
        uint32_t nb = 0;
        if (idx <= n_tok) {
            const uint32_t t = idx < n_tok ? tok[idx] : 256u;
            if (t >> 16) {
                const uint32_t ls = deflate_len_symbol(t >> 16), ds = deflate_dist_symbol(t & 0xFFFFu);
                const uint32_t lc = s_code[ls & 0xFFFFu], dc = s_dcode[ds & 0xFFu];
                v = lc & 0xFFFFu;
                nb = lc >> 16;
                v |= (uint64_t)(ls >> 24) << nb;
                nb += (ls >> 16) & 0xFFu;
                v |= (uint64_t)(dc & 0xFFFFu) << nb;
                nb += dc >> 16;
                v |= (uint64_t)(ds >> 16) << nb;
                nb += (ds >> 8) & 0xFFu;
            } else {
                const uint32_t cd = s_code[t];
                v = cd & 0xFFFFu;
                nb = cd >> 16;
            }
        }
        uint32_t incl = nb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t T = cbits + (uint32_t)__shfl((int)incl, 63), nw = T >> 5;
        for (int j = lane; j < STAGE; j += 64) s_stage[j] = j == 0 ? carry : 0u;
        __syncthreads();
        if (nb) {                                                   // up to 48 bits from any bit of a word on: three words
            const uint32_t pos = cbits + incl - nb, sh = pos & 31;
            const uint64_t rest = v >> (32 - sh);
            atomicOr(&s_stage[pos >> 5], (uint32_t)(v << sh));
            if ((uint32_t)rest) atomicOr(&s_stage[(pos >> 5) + 1], (uint32_t)rest);
            if (rest >> 32) atomicOr(&s_stage[(pos >> 5) + 2], (uint32_t)(rest >> 32));
        }
        __syncthreads();
        for (uint32_t j = lane; j < nw; j += 64) q[j] = s_stage[j];
        carry = s_stage[nw];
        cbits = T & 31;
        q += nw;
        __syncthreads();
    }
    if ((uint32_t)lane < (cbits + 7) >> 3) reinterpret_cast<uint8_t *>(q)[lane] = (uint8_t)(carry >> (8 * lane));
}

}  // namespace npore
