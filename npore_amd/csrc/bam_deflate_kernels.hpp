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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bam_emit_kernels.hpp"
#include "deflate_code.hpp"

namespace npore {

// what the planning kernel leaves of a member for the emitting kernel
struct DeflateMemberPlan {
    uint32_t code[DEFLATE_NSYM];       // length << 16 | bits
    uint32_t hdr_bits, block_bytes;    // block_bytes 0: the stored block
    uint32_t crc, pad;
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

__global__ __launch_bounds__(64) void plan_deflate_kernel(DeflateParams p)
{
    constexpr int P = DEFLATE_MEMBER_PAYLOAD, SLICE = P / 64;
    __shared__ DeflateWork w;
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    const DeflateCuts cuts = deflate_cuts(*p.stream_pos, (int64_t)*p.total);
    if (k >= cuts.n_members || k >= p.max_members) return;
    const uint8_t *src = p.recs + cuts.first + k * P;
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
    // step 1 of the rule by all lanes: the rank of a used symbol is the number of used symbols with a smaller (count, symbol)
    uint32_t key[5];
    int rank[5];
    int m = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int s = lane + 64 * j;
        const uint32_t f = s < DEFLATE_NSYM ? w.freq[s] : 0u;
        key[j] = f ? f << 9 | (uint32_t)s : 0u;
        rank[j] = 0;
        m += __popcll(__ballot(f != 0));
    }
    for (int t = 0; t < DEFLATE_NSYM; t++) {
        const uint32_t f = w.freq[t];
        if (!f) continue;
        const uint32_t kt = f << 9 | (uint32_t)t;
#pragma unroll
        for (int j = 0; j < 5; j++) rank[j] += kt < key[j] ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 5; j++)
        if (key[j]) { w.a[rank[j]] = key[j] >> 9; w.sym[rank[j]] = (uint16_t)(key[j] & 0x1FFu); }
    __syncthreads();
    DeflateMemberPlan &pl = p.plans[k];
    if (lane == 0) {
        deflate_plan_sorted(w, m);
        const uint32_t block = deflate_block_bytes(w);
        const bool stored = block >= (uint32_t)P + 5;
        pl.hdr_bits = w.hdr_bits;
        pl.block_bytes = stored ? 0u : block;
        pl.crc = ~c;
        pl.pad = 0;
        p.sizes[k] = stored ? (uint32_t)P + 31u : block + 26u;
        if (!stored) deflate_header(w, pl.hdr);
    }
    __syncthreads();
    for (int s = lane; s < DEFLATE_NSYM; s += 64) pl.code[s] = w.freq[s];
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

// one wavefront per member
__global__ __launch_bounds__(64) void emit_deflate_kernel(DeflateParams p)
{
    constexpr int P = DEFLATE_MEMBER_PAYLOAD;
    __shared__ uint32_t s_code[DEFLATE_NSYM];
    __shared__ uint32_t s_stage[34];
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    const int64_t n_members = min(p.info[0], p.max_members);
    if (k >= n_members) {                                           // the two fragments, raw, behind the last member
        const int64_t total = (int64_t)*p.total, head = p.info[2], tail = p.info[3];
        if (k == n_members && p.info[0] <= p.max_members) wave_copy<0>(p.comp + p.info[1], p.recs, head, false, lane);
        if (k == n_members + 1 && p.info[0] <= p.max_members) wave_copy<0>(p.comp + p.info[1] + head, p.recs + (total - tail), tail, false, lane);
        return;
    }
    const uint32_t size = p.sizes[k];
    if (size == 0) return;
    const DeflateMemberPlan &pl = p.plans[k];
    const uint8_t *src = p.recs + p.info[2] + k * P;
    uint8_t *o = p.comp + p.off[k];
    if (lane < 18) o[lane] = lane < 16 ? bgzf_header_byte(lane) : (uint8_t)((size - 1) >> (8 * (lane - 16)));
    const uint32_t block = pl.block_bytes;
    uint8_t *trailer = o + 18 + (block ? block : (uint32_t)P + 5u);
    if (lane < 8) trailer[lane] = (uint8_t)((lane < 4 ? pl.crc : (uint32_t)P) >> (8 * (lane & 3)));
    if (!block) {
        if (lane < 5) o[18 + lane] = lane == 0 ? 1 : (uint8_t)((lane < 3 ? (uint32_t)P : ~(uint32_t)P) >> (8 * ((lane - 1) & 1)));
        wave_copy<0>(o + 23, src, P, false, lane);
        return;
    }
    for (int s = lane; s < DEFLATE_NSYM; s += 64) s_code[s] = pl.code[s];
    // the stream goes out in aligned words: it begins at the last word boundary at or in front of the header's last whole
    // byte, the (at most three) header bytes behind that boundary and the header's last bits in the first word
    const uint32_t hb = pl.hdr_bits >> 3;                           // (>= 4: 17 + 12 bits and five symbols at the least)
    const uint32_t back = (uint32_t)((uintptr_t)(o + 18 + hb) & 3);
    uint32_t *q = reinterpret_cast<uint32_t *>(o + 18 + hb - back);
    for (uint32_t j = lane; j < hb - back; j += 64) o[18 + j] = pl.hdr[j];
    uint32_t carry = 0, cbits = 8 * back + (pl.hdr_bits & 7);
    for (uint32_t j = 0; j < back; j++) carry |= (uint32_t)pl.hdr[hb - back + j] << (8 * j);
    if (pl.hdr_bits & 7) carry |= (uint32_t)pl.hdr[hb] << (8 * back);
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

}  // namespace npore
