// purity_kernels.hpp -- Gini purity of pileups from BAM records, on the device (rule: purity_rec.hpp).
//
// Counters live on the device for a WINDOW: at most W positions of the merged ranges of one contig, packed densely
// (window-local index loc = dense - win_lo).  Layout, chosen with the atomics in mind: PLANES, not rows --
//   cnt[plane][W] of uint32, planes 0..4 = A C G T *, 5 = insertions t, 6 = bucket offsets (window's end); v2[W] of uint64.
// The lanes of a wave take 64 neighbouring positions of one record and nearly all of them add to the SAME symbol plane
// only where the read agrees with its neighbours' letters; per plane the wave's adds fall into one or two contiguous
// stretches of at most 256 bytes.  Position-major rows of 32 bytes would give every lane a cache line segment of its own
// (64 lanes over 2 KiB, sixteen 128-byte lines), the shape that is an order of magnitude slower for global atomics.
//
//   purity_records_kernel   one workgroup of 256 per record, the shape of confusion_records_kernel: CIGAR tiles of 256
//                           operations, prefix sums for the reference start and the query start.  The rank over the
//                           reference-consuming entry positions (M-type and D) IS the reference offset -- a record with
//                           N never gets here (cms_gate) --, so one sum serves both.  One entry per lane; 32-bit global
//                           atomic adds into the planes; the lane with a +k marker adds to plane 5 and appends an event
//                           {loc, key} behind a cursor, the cursor add folded over the wave's lanes that have one.
//   the window's end        exclusive scan of plane 5 into plane 6 (three small kernels, written out), scatter of the
//                           events into per-position buckets (the offset is bumped, so it ends as the bucket's END),
//                           purity_pairs_kernel: for every event the number of events of its bucket with an equal key,
//                           added to v2[loc] -- summed per position that is the sum of v^2.  One lane per event walks
//                           its whole bucket, so a bucket may be of any size (quadratic in the insertions of ONE position).
//   purity_finalize_kernel  one lane per position: n, S_b, S_i, the two bins into two 100-cell LDS histograms per
//                           workgroup (flushed as 64-bit global adds), on request the row (n, S_b, t, S_i); leaves the
//                           window zeroed.
// Integers only: nothing depends on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "purity_rec.hpp"
#include "staged_head.hpp"

namespace npore {

struct PurEvent {
    uint32_t loc, pad;
    uint64_t key;
};

constexpr int PUR_PLANES = 7;
constexpr int PUR_D_OVERFLOW = PUR_N_TALLIES;        // device tallies: one more cell, events dropped for want of room (a bug if ever set)
constexpr int PUR_D_TALLIES = PUR_N_TALLIES + 1;

struct PurParams {
    const uint8_t *raw;          // record heads through the qualities, one after the other (block_size word first)
    const int64_t *raw_off;      // [n_reads + 1]
    int64_t n_reads;
    const CmsRange *ranges;      // merged ranges of the contig, ann = dense index
    int n_ranges;
    int64_t win_lo, win_hi;      // dense
    int64_t ref_lo, ref_hi;      // the hull of the window's positions on the contig
    int64_t W;                   // plane stride
    int min_bq;
    uint32_t *cnt;
    PurEvent *events;
    uint32_t *cursor;
    uint32_t ev_cap;
    unsigned long long *tallies; // [PUR_D_TALLIES]
};

struct PurDeviceSink {
    uint32_t *cnt, *tl;
    int64_t W, win_lo;
    bool has;                    // this lane's entry added an insertion: appended by the kernel where the wave meets again
    uint32_t loc;
    uint64_t key;
    __device__ __forceinline__ void sym(int64_t dense, int s) { atomicAdd(&cnt[(int64_t)s * W + (dense - win_lo)], 1u); }
    __device__ __forceinline__ void ins(int64_t dense, uint64_t k)
    {
        loc = (uint32_t)(dense - win_lo);
        atomicAdd(&cnt[5 * W + loc], 1u);
        key = k;
        has = true;
    }
    __device__ __forceinline__ void tally(int which) { atomicAdd(&tl[which], 1u); }
};

__global__ __launch_bounds__(256) void purity_records_kernel(PurParams p)
{
    __shared__ uint32_t s_tl[PUR_D_TALLIES];
    __shared__ uint32_t s_r[257], s_q[257];
    __shared__ uint32_t s_wave[4][2];
    const int64_t rec = blockIdx.x;
    if (rec >= p.n_reads) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < PUR_D_TALLIES) s_tl[t] = 0u;

    const uint8_t *f = p.raw + p.raw_off[rec] + 4;                 // the fixed fields (hostio.hpp RecView)
    const int64_t pos = (int32_t)cms_ld32(f + 4);
    const int64_t l_seq = (int32_t)cms_ld32(f + 16);
    PurView v;
    staged_cigar(f, v.cg, v.nc, v.sq);
    const int nc = v.nc;
    v.ql = v.sq + (size_t)((l_seq + 1) / 2);
    v.l_seq = l_seq;
    v.ranges = p.ranges;
    v.n_ranges = p.n_ranges;
    v.win_lo = p.win_lo;
    v.win_hi = p.win_hi;
    v.min_bq = p.min_bq;
    PurDeviceSink sink{p.cnt, s_tl, p.W, p.win_lo, false, 0u, 0ull};
    __syncthreads();

    int64_t rbase = pos, qbase = 0;
    int hint = -1;
    for (int c0 = 0; c0 < nc; c0 += 256) {
        const int j = c0 + t;
        uint32_t xr = 0u, xq = 0u;
        if (j < nc) {
            const uint32_t w = cms_ld32(v.cg + 4 * (size_t)j), op = w & 15u, len = w >> 4;
            xr = cms_op_ref(op) ? len : 0u;
            xq = cms_op_query(op) ? len : 0u;
        }
        // inclusive prefix sums over the tile: within the wave, then over the four waves
        uint32_t ir = xr, iq = xq;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t yr = __shfl_up(ir, d), yq = __shfl_up(iq, d);
            if (lane >= d) { ir += yr; iq += yq; }
        }
        if (lane == 63) { s_wave[wave][0] = ir; s_wave[wave][1] = iq; }
        __syncthreads();
        uint32_t br = 0u, bq = 0u;
        for (int w = 0; w < wave; w++) { br += s_wave[w][0]; bq += s_wave[w][1]; }
        s_r[t + 1] = br + ir;
        s_q[t + 1] = bq + iq;
        if (t == 0) s_r[0] = s_q[0] = 0u;
        __syncthreads();
        const uint32_t total = s_r[256];
        // (a tile that lies outside the window's hull on the contig has nothing for this window)
        if (rbase < p.ref_hi && rbase + (int64_t)total > p.ref_lo) {
            for (uint32_t i0 = 0u; i0 < total; i0 += 256u) {       // every lane makes every turn: the wave meets at the append
                const uint32_t i = i0 + (uint32_t)t;
                sink.has = false;
                if (i < total) {
                    int lo = 0, hi = 256;                          // the last operation u of the tile with s_r[u] <= i: the one that holds rank i
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (s_r[mid] <= i) lo = mid; else hi = mid;
                    }
                    const uint32_t w = cms_ld32(v.cg + 4 * (size_t)(c0 + lo)), op = w & 15u;
                    const uint32_t off = i - s_r[lo];
                    const bool last = i + 1u == s_r[lo + 1];
                    if (cms_op_match(op)) pur_entry(v, sink, c0 + lo, w, rbase + (int64_t)i, qbase + (int64_t)s_q[lo] + off, last, hint);
                    else if (op == 2u) pur_entry(v, sink, c0 + lo, w, rbase + (int64_t)i, qbase + (int64_t)s_q[lo], last, hint);
                }
                // the append: one cursor add for the wave's lanes that have an event
                const unsigned long long mask = __ballot(sink.has);
                if (mask) {
                    const int leader = __ffsll((long long)mask) - 1;
                    uint32_t base = 0u;
                    if (lane == leader) base = atomicAdd(p.cursor, (uint32_t)__popcll(mask));
                    base = __shfl(base, leader);
                    if (sink.has) {
                        const uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                        if (at < p.ev_cap) p.events[at] = PurEvent{sink.loc, 0u, sink.key};
                        else atomicAdd(&s_tl[PUR_D_OVERFLOW], 1u);
                    }
                }
            }
        }
        rbase += s_r[256];
        qbase += s_q[256];
        __syncthreads();
    }
    __syncthreads();
    if (t < PUR_D_TALLIES && s_tl[t] != 0u) atomicAdd(&p.tallies[t], (unsigned long long)s_tl[t]);
}

// ---- the window's end ---------------------------------------------------------------------------------------------
constexpr int PUR_SCAN_PER_BLOCK = 1024;             // 256 threads, four positions each

// exclusive prefix sums of `in` within blocks of 1024 positions into `out`; the blocks' sums into bsum
__global__ __launch_bounds__(256) void purity_scan_blocks_kernel(const uint32_t *in, uint32_t *out, uint32_t *bsum, int64_t n)
{
    __shared__ uint32_t s_w[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t base = (int64_t)blockIdx.x * PUR_SCAN_PER_BLOCK + 4 * t;
    uint32_t x[4], sum = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) { x[k] = base + k < n ? in[base + k] : 0u; sum += x[k]; }
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (int w = 0; w < wave; w++) run += s_w[w];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + k < n) out[base + k] = run;
        run += x[k];
    }
    if (t == 255) bsum[blockIdx.x] = run;
}

// exclusive prefix sums of the blocks' sums, in place: one workgroup, 256 at a time behind a running total
__global__ __launch_bounds__(256) void purity_scan_top_kernel(uint32_t *bsum, int n_blocks)
{
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_carry;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) s_carry = 0u;
    __syncthreads();
    for (int b0 = 0; b0 < n_blocks; b0 += 256) {
        const uint32_t x = b0 + t < n_blocks ? bsum[b0 + t] : 0u;
        uint32_t inc = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d);
            if (lane >= d) inc += y;
        }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint32_t run = s_carry + inc - x;
        for (int w = 0; w < wave; w++) run += s_w[w];
        if (b0 + t < n_blocks) bsum[b0 + t] = run;
        __syncthreads();
        if (t == 255) s_carry = run + x;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void purity_scan_add_kernel(uint32_t *out, const uint32_t *bsum, int64_t n)
{
    const int64_t base = (int64_t)blockIdx.x * PUR_SCAN_PER_BLOCK + 4 * threadIdx.x;
    const uint32_t add = bsum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (base + k < n) out[base + k] += add;
}

// events into buckets: off[loc] is bumped and ends as the END of the bucket of loc (its size is plane 5)
__global__ __launch_bounds__(256) void purity_scatter_kernel(const PurEvent *events, const uint32_t *cursor, uint32_t cap, uint32_t *off, PurEvent *sorted)
{
    const uint32_t n = *cursor < cap ? *cursor : cap;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const PurEvent e = events[i];
    const uint32_t at = atomicAdd(&off[e.loc], 1u);
    if (at < cap) sorted[at] = e;
}

__global__ __launch_bounds__(256) void purity_pairs_kernel(const PurEvent *sorted, const uint32_t *cursor, uint32_t cap, const uint32_t *t_plane,
                                                            const uint32_t *off, unsigned long long *v2)
{
    const uint32_t n = *cursor < cap ? *cursor : cap;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const PurEvent e = sorted[i];
    const uint32_t b1 = off[e.loc] < cap ? off[e.loc] : cap, cntb = t_plane[e.loc], b0 = b1 >= cntb ? b1 - cntb : 0u;
    uint32_t same = 0u;
    for (uint32_t k = b0; k < b1; k++) same += sorted[k].key == e.key ? 1u : 0u;   // (neighbouring lanes share the bucket: the same addresses)
    atomicAdd(&v2[e.loc], (unsigned long long)same);
}

struct PurFinalParams {
    uint32_t *cnt;
    unsigned long long *v2;
    int64_t W, n;                // plane stride; positions of this window
    unsigned long long *hist;    // [2][PUR_BINS]: bases, insertions
    unsigned long long *tallies;
    int64_t *rows;               // NULL or [n][4]
};

__global__ __launch_bounds__(256) void purity_finalize_kernel(PurFinalParams p)
{
    __shared__ uint32_t s_h[2 * PUR_BINS + 2];       // two histograms, positions covered, positions too deep
    const int t = threadIdx.x;
    if (t < 2 * PUR_BINS + 2) s_h[t] = 0u;
    __syncthreads();
    const int64_t loc = (int64_t)blockIdx.x * 256 + t;
    if (loc < p.n) {
        uint64_t c[5], n = 0, sb = 0;
#pragma unroll
        for (int s = 0; s < 5; s++) {
            c[s] = p.cnt[(int64_t)s * p.W + loc];
            n += c[s];
            sb += c[s] * c[s];
        }
        const uint64_t ti = p.cnt[5 * p.W + loc], v2 = p.v2[loc];
        int64_t row[4] = {0, 0, 0, 0};
        if (n != 0) {
            atomicAdd(&s_h[2 * PUR_BINS], 1u);
            row[0] = (int64_t)n;
            if (n >= (uint64_t)PUR_MAX_DEPTH) {
                atomicAdd(&s_h[2 * PUR_BINS + 1], 1u);
                row[1] = row[2] = row[3] = -1;
            } else {
                const uint64_t si = (n - ti) * (n - ti) + v2;
                atomicAdd(&s_h[pur_bin(sb, n)], 1u);
                atomicAdd(&s_h[PUR_BINS + pur_bin(si, n)], 1u);
                row[1] = (int64_t)sb;
                row[2] = (int64_t)ti;
                row[3] = (int64_t)si;
            }
#pragma unroll
            for (int s = 0; s < 6; s++) p.cnt[(int64_t)s * p.W + loc] = 0u;
            p.v2[loc] = 0ull;
        }
        if (p.rows) {
#pragma unroll
            for (int k = 0; k < 4; k++) p.rows[4 * loc + k] = row[k];
        }
    }
    __syncthreads();
    if (t < 2 * PUR_BINS && s_h[t] != 0u) atomicAdd(&p.hist[t], (unsigned long long)s_h[t]);
    if (t == 254 && s_h[2 * PUR_BINS] != 0u) atomicAdd(&p.tallies[PUR_T_COVERED], (unsigned long long)s_h[2 * PUR_BINS]);
    if (t == 255 && s_h[2 * PUR_BINS + 1] != 0u) atomicAdd(&p.tallies[PUR_T_TOO_DEEP], (unsigned long long)s_h[2 * PUR_BINS + 1]);
}

}  // namespace npore
