// md_rec.hpp -- the MD tag of a realigned read (BAM out, FULL records with NPORE_OUT_MD): the rule, stated ONCE and compiled
// for the gfx950 kernels (bam_emit_kernels.hpp md_size_kernel / emit_md_kernel) and for the host twin (bam_reader.hpp
// md_of_words, plain g++), the way nm_rec.hpp, purity_rec.hpp and confusion_rec.hpp are.
//
// MD is written over the read's FINAL CIGAR words (`len << 4 | op`) on the two code arrays align() got ('NACGT-' -> 0 ... 5,
// anything else 0), with nm_rec.hpp's nm_consumes / nm_compares / nm_differs, so NM and MD cannot disagree (the sequential
// twins also share their walk over the words, nm_rec.hpp cigar_words_each):
//   u = 0                                    compared positions that matched since the last item
//   for every word (op, len), len > 0:
//     M = X : for each position: if nm_differs(...)  emit decimal(u), LETTER[ref code], u = 0
//                                 else                u += 1
//     D     : emit decimal(u), '^', LETTER[ref code] for each of the len positions, u = 0
//     N     : reference advances, nothing emitted;   I S : query advances;   H P : nothing
//   at the end emit decimal(u)
//   LETTER = "NACGTN"; a reference position beyond the array has code 0.
// So (letters not behind '^') + (letters behind '^') + (bases under I) = NM.
// That is `samtools calmd`'s text except where NM already differs from calmd's: an IUPAC letter other than N became code 0
// before align() saw it, so it counts as a mismatch and prints as N (calmd compares the letters and prints the reference's).
//
// The text goes to a SINK, `put(at, byte)` with `at` counted from the text's first byte: MdCount drops the bytes (the size
// is where the walk ends), MdStore keeps them (up to the size it is told).  The device walk (bam_emit_kernels.hpp md_walk) places its bytes in
// parallel, this file's md_walk_words one after the other; both end at the same length with the same bytes.
#pragma once
#include <stdint.h>

#include "nm_rec.hpp"

namespace npore {

struct MdCount {
    NPORE_NM_HD void put(int64_t, uint8_t) const {}
};
struct MdStore {
    uint8_t *dst;
    int64_t cap;                 // the size pass's answer: nothing is stored behind it
    NPORE_NM_HD void put(int64_t at, uint8_t c) const { if (at < cap) dst[at] = c; }
};

NPORE_NM_HD uint8_t md_letter(uint32_t code) { return (uint8_t)"NACGTN"[code < 6u ? code : 0u]; }
// decimal digits of u (1 ... 10)
NPORE_NM_HD int md_digits(uint32_t u)
{
    return u < 10u ? 1 : u < 100u ? 2 : u < 1000u ? 3 : u < 10000u ? 4 : u < 100000u ? 5 : u < 1000000u ? 6 : u < 10000000u ? 7 : u < 100000000u ? 8
           : u < 1000000000u ? 9 : 10;
}
// u as nd = md_digits(u) digits at `at`
template <class Sink>
NPORE_NM_HD void md_put_decimal(const Sink &sink, int64_t at, uint32_t u, int nd)
{
    for (int i = nd - 1; i >= 0; i--) {
        sink.put(at + i, (uint8_t)('0' + u % 10u));
        u /= 10u;
    }
}

// MD of n CIGAR words at w (little-endian, unaligned), sequentially, into the sink: the text's length (no NUL)
template <class Sink>
inline int64_t md_walk_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl, const Sink &sink)
{
    int64_t at = 0;
    uint32_t u = 0;
    auto count = [&]() {
        const int nd = md_digits(u);
        md_put_decimal(sink, at, u, nd);
        at += nd;
        u = 0;
    };
    cigar_words_each(w, n, [&](uint32_t op, uint32_t len, int64_t a, int64_t b) {
        if (nm_compares(op)) {
            for (uint32_t q = 0; q < len; q++) {
                if (!nm_differs(ref, rl, a + q, seq, sl, b + q)) { u++; continue; }
                count();
                sink.put(at++, md_letter(code_at(ref, rl, a + q)));
            }
        } else if (op == 2 && len > 0) {
            count();
            sink.put(at++, (uint8_t)'^');
            for (uint32_t q = 0; q < len; q++) sink.put(at++, md_letter(code_at(ref, rl, a + q)));
        }
    });
    count();
    return at;
}
inline int64_t md_size_of_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl)
{
    return md_walk_words(w, n, ref, rl, seq, sl, MdCount{});
}
// ... the text at dst[cap] (cap: md_size_of_words' answer): returns the text's length
inline int64_t md_into_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl, uint8_t *dst, int64_t cap)
{
    return md_walk_words(w, n, ref, rl, seq, sl, MdStore{dst, cap});
}

}  // namespace npore
