// nm_rec.hpp -- the NM tag of a realigned read (BAM out, FULL records): the rule, stated ONCE and compiled for the gfx950
// kernel (bam_emit_kernels.hpp nm_count_kernel) and for the host twin (bam_reader.hpp bam_record_full_into, plain g++),
// the way confusion_rec.hpp and purity_rec.hpp are.  With the rule, the walk over the words that the sequential twins of NM,
// MD (md_rec.hpp) and cs / de (cs_rec.hpp) share, cigar_words_each, so that they agree in the positions as well.
//
// NM is counted over the read's FINAL CIGAR on the two code arrays align() got: the reference bases under the alignment
// and the query bases without the soft clips, 'NACGT-' -> 0 ... 5 and anything else 0.
//   NM = bases under I + bases under D + the positions under M (= and X alike) where the two codes differ or either is 0.
// That is `samtools calmd`'s count with one difference: calmd compares the letters, so an IUPAC letter other than N
// matches itself; here every such letter has become code 0 before align() saw it and counts as N does -- a mismatch.
// N skips reference, S skips query; a position beyond the end of either array (a CIGAR that does not fit its read) has
// code 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NPORE_NM_HD __host__ __device__ __forceinline__
#else
#define NPORE_NM_HD inline
#endif

namespace npore {

// what operation `op` consumes: bit 0 reference, bit 1 query
NPORE_NM_HD uint32_t nm_consumes(uint32_t op)
{
    return (op == 0 || op == 7 || op == 8) ? 3u : (op == 2 || op == 3) ? 1u : (op == 1 || op == 4) ? 2u : 0u;
}
// the whole of an operation's length counts (I, D)
NPORE_NM_HD bool nm_counts_whole(uint32_t op) { return op == 1 || op == 2; }
// the positions of the operation are compared (M, =, X)
NPORE_NM_HD bool nm_compares(uint32_t op) { return op == 0 || op == 7 || op == 8; }
// the code at position `at` of an array of len codes: 0 beyond its end
NPORE_NM_HD uint32_t code_at(const uint8_t *arr, int64_t len, int64_t at) { return at < len ? arr[at] : 0u; }
// one compared position: reference position a of rl, query position b of sl
NPORE_NM_HD bool nm_differs(const uint8_t *ref, int64_t rl, int64_t a, const uint8_t *seq, int64_t sl, int64_t b)
{
    const uint32_t r = code_at(ref, rl, a), q = code_at(seq, sl, b);
    return r != q || r == 0u || q == 0u;
}

// The sequential twins' walk: visit(op, len, a, b) for every one of the n CIGAR words
// `len << 4 | op` at w (little-endian, unaligned) in order, a and b the reference and the query bases consumed in front of it
template <class Visit>
inline void cigar_words_each(const uint8_t *w, int64_t n, Visit visit)
{
    int64_t a = 0, b = 0;
    for (int64_t c = 0; c < n; c++) {
        const uint32_t v = (uint32_t)w[4 * c] | (uint32_t)w[4 * c + 1] << 8 | (uint32_t)w[4 * c + 2] << 16 | (uint32_t)w[4 * c + 3] << 24;
        const uint32_t op = v & 15u, len = v >> 4, use = nm_consumes(op);
        visit(op, len, a, b);
        if (use & 1u) a += len;
        if (use & 2u) b += len;
    }
}

// NM of n CIGAR words at w, sequentially
inline int64_t nm_of_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl)
{
    int64_t nm = 0;
    cigar_words_each(w, n, [&](uint32_t op, uint32_t len, int64_t a, int64_t b) {
        if (nm_counts_whole(op)) nm += len;
        if (nm_compares(op))
            for (uint32_t q = 0; q < len; q++) nm += nm_differs(ref, rl, a + q, seq, sl, b + q) ? 1 : 0;
    });
    return nm;
}

}  // namespace npore
