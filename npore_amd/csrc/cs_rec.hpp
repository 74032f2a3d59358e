// cs_rec.hpp -- the cs and de tags of a realigned read (BAM out, FULL records with NPORE_TAG_CS / NPORE_TAG_DE): the rule, stated
// ONCE and compiled for the gfx950 kernels (bam_emit_kernels.hpp cs_size_kernel / emit_cs_kernel) and for the host twin
// (bam_reader.hpp cs_de_tags_of_words, plain g++), the way md_rec.hpp and nm_rec.hpp are.
//
// Both are written over the read's FINAL CIGAR words (`len << 4 | op`, the clip words excluded as for NM and MD) on the two code
// arrays align() got ('NACGT-' -> 0 ... 5, anything else 0), with nm_rec.hpp's nm_consumes / nm_compares / nm_differs, so NM,
// MD, cs and de cannot disagree (the sequential twins also share their walk over the words, nm_rec.hpp cigar_words_each):
//   u = 0                                    compared positions that did not differ since the stretch began
//   for every word (op, len), len > 0 (a word of length 0 does nothing):
//     M = X : for each position: if nm_differs(...)  end the stretch, emit '*', lower[ref code], lower[read code];   X += 1
//                                 else                u += 1 (long form: '=' in front of the stretch's first letter, then
//                                                     UPPER[ref code]);                                               E += 1
//     I     : end the stretch, emit '+', lower[read code] for each of the len positions;                              G += 1
//     D     : end the stretch, emit '-', lower[ref code] for each of the len positions;                               G += 1
//     N     : end the stretch; the reference advances.  `~` is NOT written: a final CIGAR with N cannot come out of align(),
//             only the debug entry points, which take any words, can meet one
//     S     : the query advances;   H P : nothing   (as in md_rec.hpp)
//   at the end, end the stretch
//   "end the stretch", short form: if u > 0 emit ':' decimal(u); both forms: u = 0
//   lower = "nacgtn", UPPER = "NACGTN"; a position beyond either array has code 0.
// A stretch ends at an I / D / N word and at a differing position and at nothing else: neighbouring M-type words continue one.
// So (number of '*') + (letters behind '+') + (letters behind '-') = NM, the ':' counts plus the '*' number the M-type
// positions, and the long form with every `=LETTERS` replaced by `:<their number>` is the short form.
//
//   de = (float)((double)(X + G) / (double)(E + X + G)), 0.0f when E + X + G = 0: minimap2's gap-compressed per-base divergence
//   (every I and D word is one gap open, neighbouring ones included), written 'd' 'e' 'f' and four little-endian bytes.
//
// This is minimap2's cs / de with the one difference NM and MD already have: an IUPAC letter other than N became code 0
// before align() saw it, and code 0 counts as a mismatch (`*nn` for N on N) where minimap2 leaves ambiguous bases out.
// Neither minimap2 nor samtools is needed or used by the tests: they pin the rule by hand-written texts and by a separate
// Python statement (bam.cs_of / bam.de_of).
//
// Size.  An item never has more than three bytes per base it covers: `*ab` covers one position; `:` + decimal(u) <= 3 u and
// `=` + u letters <= 3 u for u >= 1; `+` / `-` + len letters <= 3 len.  So the text has at most 3 * (compared + I + D bases)
// bytes, which is at most 3 * (reference bases + query bases) of a final CIGAR that fits its arrays.
//
// The text goes to a SINK, `put(at, byte)` (md_rec.hpp MdCount / MdStore).  The device walk (bam_emit_kernels.hpp cs_walk)
// places its bytes in parallel, this file's cs_walk_words one after the other; both end at the same length with the same bytes.
#pragma once
#include <stdint.h>

#include "md_rec.hpp"

namespace npore {

// E, X, G of the walk: compared positions that do not differ, that differ, I and D words
struct CsCounts {
    uint32_t e = 0, x = 0, g = 0;
};
NPORE_NM_HD float de_of_counts(uint32_t e, uint32_t x, uint32_t g)
{
    const double den = (double)e + (double)x + (double)g;
    return den > 0.0 ? (float)(((double)x + (double)g) / den) : 0.0f;
}
NPORE_NM_HD uint8_t cs_lower(uint32_t code) { return (uint8_t)"nacgtn"[code < 6u ? code : 0u]; }

// cs of n CIGAR words at w (little-endian, unaligned), sequentially, into the sink: the text's length (no NUL); the counts to c
template <class Sink>
inline int64_t cs_walk_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl, bool lng,
                             const Sink &sink, CsCounts *c = nullptr)
{
    int64_t at = 0;
    uint32_t u = 0;
    CsCounts cnt;
    auto end_stretch = [&]() {
        if (u > 0 && !lng) {
            const int nd = md_digits(u);
            sink.put(at, (uint8_t)':');
            md_put_decimal(sink, at + 1, u, nd);
            at += 1 + nd;
        }
        u = 0;
    };
    cigar_words_each(w, n, [&](uint32_t op, uint32_t len, int64_t a, int64_t b) {
        if (len == 0) return;
        if (nm_compares(op)) {
            for (uint32_t q = 0; q < len; q++) {
                if (nm_differs(ref, rl, a + q, seq, sl, b + q)) {
                    end_stretch();
                    sink.put(at++, (uint8_t)'*');
                    sink.put(at++, cs_lower(code_at(ref, rl, a + q)));
                    sink.put(at++, cs_lower(code_at(seq, sl, b + q)));
                    cnt.x++;
                    continue;
                }
                if (lng) {
                    if (u == 0) sink.put(at++, (uint8_t)'=');
                    sink.put(at++, md_letter(code_at(ref, rl, a + q)));
                }
                u++;
                cnt.e++;
            }
        } else if (op == 1 || op == 2) {
            end_stretch();
            sink.put(at++, (uint8_t)(op == 1 ? '+' : '-'));
            for (uint32_t q = 0; q < len; q++) sink.put(at++, op == 1 ? cs_lower(code_at(seq, sl, b + q)) : cs_lower(code_at(ref, rl, a + q)));
            cnt.g++;
        } else if (op == 3) {
            end_stretch();
        }
    });
    end_stretch();
    if (c) *c = cnt;
    return at;
}
inline int64_t cs_size_of_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl, bool lng,
                                CsCounts *c = nullptr)
{
    return cs_walk_words(w, n, ref, rl, seq, sl, lng, MdCount{}, c);
}
// ... the text at dst[cap] (cap: cs_size_of_words' answer): returns the text's length
inline int64_t cs_into_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl, bool lng, uint8_t *dst,
                             int64_t cap)
{
    return cs_walk_words(w, n, ref, rl, seq, sl, lng, MdStore{dst, cap});
}

}  // namespace npore
