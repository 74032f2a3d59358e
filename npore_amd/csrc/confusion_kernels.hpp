// confusion_kernels.hpp -- the count matrices of --recalc_cms from BAM records, on the device (rule: confusion_rec.hpp).
//
// The records arrive as the file pipeline's record heads (unpack_kernels.hpp) extended through the quality bytes; the
// contig is the FASTA resident on the device; the annotation is np_info_wave_kernel's byte planes over the range slices
// of ONE contig (slice_codes_kernel lays the slices out one after the other, each en - st + 1 long, so neighbours
// overlap by one base).  One workgroup of 256 per record, the shape of unpack_records_kernel:
//   * the CIGAR is taken in tiles of 256 operations, one per thread; a prefix sum over the tile gives every operation
//     its reference start, its query start and the rank of its first M-type position;
//   * the threads then take the tile's M-type positions one per lane (rank -> operation by bisection of the prefix sums
//     in LDS): neighbouring lanes read neighbouring bytes of the contig, the 4-bit bases, the qualities and the planes;
//   * the lane on an operation's last position handles the marker; the +k compare is a short serial loop with an early
//     exit that runs only for a start period that divides k.
// Counters (partial sums on chip first, then few global atomics): 32-bit LDS histograms per workgroup for subs, inss, dels, the
// DIAGONAL of nps and the tallies -- nearly every increment --, flushed once at the end as 64-bit global adds of the
// cells that are not zero; the off-diagonal nps cells (an indel at a polymer start) go to 64-bit global atomics
// directly.  Integers only: the result does not depend on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "confusion_rec.hpp"
#include "staged_head.hpp"

namespace npore {

// base codes of the range slices of one contig, back to back: slice k = contig[st_k : st_k + slen_k) at off_k
// (the codes of cig.bases_to_int, 'NACGT-' -> 0..5, which is what calc_confusion_matrices hands get_np_info and what
// unpack_records_kernel writes: a '-' in a contig is a base of its own to the annotation and an N to the counters)
struct SliceCodesParams {
    const char *contig;
    const CmsRange *ranges;      // ann = max_n * off_k
    int n_ranges, max_n;
    uint8_t *codes;
};

__global__ __launch_bounds__(256) void slice_codes_kernel(SliceCodesParams p)
{
    const int k = blockIdx.x;                    // one workgroup per range
    if (k >= p.n_ranges) return;
    const CmsRange r = p.ranges[k];
    const int64_t off = r.ann / p.max_n;
    for (int64_t q = threadIdx.x; q < r.slen; q += 256) {
        const char ch = p.contig[r.st + q];
        p.codes[off + q] = (uint8_t)((ch == 'A' ? 1 : 0) + (ch == 'C' ? 2 : 0) + (ch == 'G' ? 3 : 0) + (ch == 'T' ? 4 : 0) + (ch == '-' ? 5 : 0));
    }
}

struct CmsParams {
    const uint8_t *raw;          // record heads through the qualities, one after the other (block_size word first)
    const int64_t *raw_off;      // [n_reads + 1]
    int64_t n_reads;
    const char *contig;          // the contig all these records lie on
    int64_t clen;
    const CmsRange *ranges;
    const int32_t *layer_off;
    int n_layers;
    const uint8_t *planes;
    int max_n, max_l, min_bq;
    unsigned long long *counts;  // subs[25] | nps[max_n][dim][dim] | inss[dim] | dels[dim] | tallies[CMS_N_TALLIES]
};

constexpr int CMS_MAX_DIM = 128;                                       // max_l <= 127 (npore_ctx_create)
constexpr int CMS_LDS_CELLS = 25 + 2 * CMS_MAX_DIM + 6 * CMS_MAX_DIM + CMS_N_TALLIES;

// LDS layout: subs[25] | inss[dim] | dels[dim] | diag[max_n][dim] | tallies
struct CmsDeviceSink {
    uint32_t *h;
    unsigned long long *nps;
    int dim;
    __device__ __forceinline__ void sub(int r, int c) { atomicAdd(&h[r * 5 + c], 1u); }
    __device__ __forceinline__ void ins(int i) { atomicAdd(&h[25 + i], 1u); }
    __device__ __forceinline__ void del(int i) { atomicAdd(&h[25 + dim + i], 1u); }
    __device__ __forceinline__ void np(int n_idx, int a, int b)
    {
        if (a < 0 || a >= dim || b < 0 || b >= dim) return;
        if (a == b) atomicAdd(&h[25 + 2 * dim + n_idx * dim + a], 1u);
        else atomicAdd(&nps[((int64_t)n_idx * dim + a) * dim + b], 1ull);
    }
    __device__ __forceinline__ void tally(int which) { atomicAdd(&h[25 + 2 * dim + 6 * dim + which], 1u); }
};

__global__ __launch_bounds__(256) void confusion_records_kernel(CmsParams p)
{
    __shared__ uint32_t s_hist[CMS_LDS_CELLS];
    __shared__ uint32_t s_r[257], s_q[257], s_m[257];
    __shared__ uint32_t s_wave[4][3];
    const int64_t rec = blockIdx.x;
    if (rec >= p.n_reads) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int dim = p.max_l + 1;
    const int n_cells = 25 + 2 * dim + 6 * dim + CMS_N_TALLIES;
    for (int c = t; c < n_cells; c += 256) s_hist[c] = 0u;

    const uint8_t *f = p.raw + p.raw_off[rec] + 4;                 // the fixed fields (hostio.hpp RecView)
    const int64_t pos = (int32_t)cms_ld32(f + 4);
    const int64_t l_seq = (int32_t)cms_ld32(f + 16);
    CmsView v;
    staged_cigar(f, v.cg, v.nc, v.sq);
    const int nc = v.nc;
    v.ql = v.sq + (size_t)((l_seq + 1) / 2);
    v.l_seq = l_seq;
    v.contig = p.contig;
    v.clen = p.clen;
    v.ranges = p.ranges;
    v.layer_off = p.layer_off;
    v.n_layers = p.n_layers;
    v.planes = p.planes;
    v.max_n = p.max_n;
    v.max_l = p.max_l;
    v.min_bq = p.min_bq;
    CmsDeviceSink sink{s_hist, p.counts + 25, dim};
    __syncthreads();
    if (t == 0) sink.tally(CMS_T_RECORDS);

    int64_t rbase = pos, qbase = 0;
    int hint = -1;
    for (int c0 = 0; c0 < nc; c0 += 256) {
        const int j = c0 + t;
        uint32_t xr = 0u, xq = 0u, xm = 0u;
        if (j < nc) {
            const uint32_t w = cms_ld32(v.cg + 4 * (size_t)j), op = w & 15u, len = w >> 4;
            xr = cms_op_ref(op) ? len : 0u;
            xq = cms_op_query(op) ? len : 0u;
            xm = cms_op_match(op) ? len : 0u;
            if (cms_adjacent(v.cg, nc, j)) sink.tally(CMS_T_ADJACENT);
        }
        // inclusive prefix sums over the tile: within the wave, then over the four waves
        uint32_t ir = xr, iq = xq, im = xm;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t yr = __shfl_up(ir, d), yq = __shfl_up(iq, d), ym = __shfl_up(im, d);
            if (lane >= d) { ir += yr; iq += yq; im += ym; }
        }
        if (lane == 63) { s_wave[wave][0] = ir; s_wave[wave][1] = iq; s_wave[wave][2] = im; }
        __syncthreads();
        uint32_t br = 0u, bq = 0u, bm = 0u;
        for (int w = 0; w < wave; w++) { br += s_wave[w][0]; bq += s_wave[w][1]; bm += s_wave[w][2]; }
        s_r[t + 1] = br + ir;
        s_q[t + 1] = bq + iq;
        s_m[t + 1] = bm + im;
        if (t == 0) s_r[0] = s_q[0] = s_m[0] = 0u;
        __syncthreads();
        const uint32_t total_m = s_m[256];
        for (uint32_t i = (uint32_t)t; i < total_m; i += 256u) {
            int lo = 0, hi = 256;                                  // the last operation u of the tile with s_m[u] <= i: the M-type one that holds rank i
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_m[mid] <= i) lo = mid; else hi = mid;
            }
            const uint32_t off = i - s_m[lo];
            const bool last = i + 1u == s_m[lo + 1];
            cms_entry(v, sink, c0 + lo, rbase + (int64_t)s_r[lo] + off, qbase + (int64_t)s_q[lo] + off, last, hint);
        }
        rbase += s_r[256];
        qbase += s_q[256];
        __syncthreads();
    }
    __syncthreads();
    // flush: subs | inss | dels to their places, the diagonal into nps, the tallies
    const int64_t n_nps = (int64_t)p.max_n * dim * dim;
    for (int c = t; c < n_cells; c += 256) {
        const uint32_t val = s_hist[c];
        if (val == 0u) continue;
        int64_t at;
        if (c < 25) at = c;
        else if (c < 25 + 2 * dim) at = 25 + n_nps + (c - 25);
        else if (c < 25 + 8 * dim) {
            const int d = c - 25 - 2 * dim, n_idx = d / dim, l = d - n_idx * dim;
            if (n_idx >= p.max_n) continue;
            at = 25 + ((int64_t)n_idx * dim + l) * dim + l;
        } else at = 25 + n_nps + 2 * dim + (c - 25 - 8 * dim);
        atomicAdd(&p.counts[at], (unsigned long long)val);
    }
}

}  // namespace npore
