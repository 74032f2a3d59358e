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

// PASS-THROUGH (npore_bam_set_output_pass, `--pass_through`), the rule stated once: a record of a run PASSES iff
// `flag & pass_mask` is non-zero, pass_mask a subset of 0x904 (secondary, supplementary, placed but unmapped; 0, the
// default: nothing passes).  A passing record is selected like a read, gives align() nothing and is written as it came:
// its staged head (STAGE_FULL) is the block_size word and the WHOLE record as it lies in the stream -- n_cigar_op and bin
// untouched, so staged_cigar() is not for it --, and every reader of a staged head asks this predicate first.
constexpr uint32_t PASS_FLAGS = 0x100u | 0x800u | 0x4u;
NPORE_STAGED_HD bool record_passes(uint32_t flag, uint32_t pass_mask) { return (flag & pass_mask) != 0; }
// ... of a staged head's (or a record's) fixed fields f
NPORE_STAGED_HD bool staged_passes(const uint8_t *f, uint32_t pass_mask)
{
    return record_passes((uint32_t)f[14] | (uint32_t)f[15] << 8, pass_mask);
}
// bytes of a passing record's staged head and of its output record: 4 + block_size
NPORE_STAGED_HD int64_t staged_pass_bytes(const uint8_t *f)
{
    return 4 + (int64_t)(int32_t)((uint32_t)f[-4] | (uint32_t)f[-3] << 8 | (uint32_t)f[-2] << 16 | (uint32_t)f[-1] << 24);
}

}  // namespace npore
