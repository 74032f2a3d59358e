// staged_head.hpp -- the one reader of a staged record head's CIGAR, for the kernels and for the host.
//
// hostio.hpp (stage_record_head) states the layout: block_size word | fixed fields | name | CIGAR words | 4-bit bases |
// qualities, the CIGAR words being the record's REAL ones (those of its CG tag where it has a long CIGAR) and their
// 32-bit count split over two 16-bit fields: low half in n_cigar_op (f + 12), high half in bin (f + 10).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NPORE_STAGED_HD __host__ __device__ __forceinline__
#else
#define NPORE_STAGED_HD inline
#endif

namespace npore {

// f: the fixed fields of a staged head (behind its block_size word).  cg: its CIGAR words, nc: how many (< 2^29),
// sq: the 4-bit bases behind them
NPORE_STAGED_HD void staged_cigar(const uint8_t *f, const uint8_t *&cg, int &nc, const uint8_t *&sq)
{
    nc = (int)((uint32_t)f[12] | (uint32_t)f[13] << 8 | (uint32_t)f[10] << 16 | (uint32_t)f[11] << 24);
    cg = f + 32 + f[8];
    sq = cg + 4 * (int64_t)nc;
}

}  // namespace npore
