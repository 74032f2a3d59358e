// eqx_rec.hpp -- the =/X form of a realigned read's CIGAR (BAM out, FULL records with NPORE_CIGAR_EQX, `--eqx`): the rule, stated
// ONCE and compiled for the gfx950 kernels (bam_emit_kernels.hpp eqx_size_kernel / emit_eqx_kernel) and for the host twin
// (bam_reader.hpp format_bam_into, plain g++), the way md_rec.hpp and cs_rec.hpp are.
//
// The input is the read's FINAL CIGAR words (`len << 4 | op`, the clip words excluded as for NM, MD and cs) on the two code
// arrays align() got ('NACGT-' -> 0 ... 5, anything else 0), with nm_rec.hpp's nm_consumes / nm_compares / nm_differs, so the
// X words, NM, MD and cs cannot disagree (the sequential twins also share their walk over the words, cigar_words_each):
//   no run is open
//   for every word (op, len), len > 0 (a word of length 0, of any op, is left out):
//     M = X : for each position: its class is X (8) if nm_differs(...), = (7) otherwise -- the input's op is ignored;
//             the open run has that class: it grows by one;  otherwise: close the run, open one of that class with length 1
//     any other op (I D N S H P): close the run, then the word goes out as it is
//   at the end, close the run
//   "close the run": if one is open, the word `its length << 4 | its class` goes out; none is open then
// A run is maximal over a STRETCH: it goes on through neighbouring M-type words, as a cs stretch does (`3=2X3M` over equal
// bases is `8=`), and is ended only by a word of length > 0 that is not compared.  Code 0 on either side, an IUPAC letter and
// a position beyond either array are X, exactly as NM, MD and cs count them.  So
//   - = and X collapsed to M and neighbours merged is the canonical M form of the input;
//   - NM = bases under I + bases under D + bases under X; the bases under = are cs's E, those under X its X;
//   - the reference and the query consumed do not change; no two neighbouring words inside a stretch have the same op.
//
// Size.  Every word that goes out is a word of the input or covers at least one compared position, so there are at most
// (words of the input) + (compared positions) of them -- for a final CIGAR that fits its arrays no more than reference bases +
// query bases, which is what a record's bound allows its words already (hostio.hpp full_record_bound).
//
// The words go to a SINK, `put(index, word)`: EqxCount drops them (the size is where the walk ends), EqxStore keeps them, up
// to the count it is told, at an address of any alignment.  The device walk (bam_emit_kernels.hpp eqx_walk) places a round's
// words in parallel, this file's eqx_walk_words one after the other; both end at the same count with the same words.
#pragma once
#include <stdint.h>

#include <vector>

#include "nm_rec.hpp"

namespace npore {

constexpr uint32_t EQX_EQ = 7u, EQX_X = 8u;      // the two classes: their CIGAR ops

struct EqxCount {
    NPORE_NM_HD void put(int64_t, uint32_t) const {}
};
struct EqxStore {
    uint8_t *dst;                // the CIGAR's place in a record: 36 + l_read_name bytes in, any alignment
    int64_t cap;                 // the size pass's answer: nothing is stored behind it
    NPORE_NM_HD void put(int64_t at, uint32_t w) const
    {
        if (at >= cap) return;
        uint8_t *q = dst + 4 * at;
        q[0] = (uint8_t)w; q[1] = (uint8_t)(w >> 8); q[2] = (uint8_t)(w >> 16); q[3] = (uint8_t)(w >> 24);
    }
};

// the =/X form of n CIGAR words at w (little-endian, unaligned), sequentially, into the sink: the number of words
template <class Sink>
inline int64_t eqx_walk_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl, const Sink &sink)
{
    int64_t at = 0;
    uint32_t cls = 0, run = 0;   // the open run (run == 0: none)
    auto close = [&]() {
        if (run > 0) sink.put(at++, run << 4 | cls);
        run = 0;
    };
    cigar_words_each(w, n, [&](uint32_t op, uint32_t len, int64_t a, int64_t b) {
        if (len == 0) return;
        if (!nm_compares(op)) {
            close();
            sink.put(at++, len << 4 | op);
            return;
        }
        for (uint32_t q = 0; q < len; q++) {
            const uint32_t c = nm_differs(ref, rl, a + q, seq, sl, b + q) ? EQX_X : EQX_EQ;
            if (run > 0 && c != cls) close();
            cls = c;
            run++;
        }
    });
    close();
    return at;
}
// ... as words behind each other, with one word of room behind them (bam_reader.hpp cigar_text_words' convention)
inline std::vector<uint8_t> eqx_of_words(const uint8_t *w, int64_t n, const uint8_t *ref, int64_t rl, const uint8_t *seq, int64_t sl)
{
    const int64_t ops = eqx_walk_words(w, n, ref, rl, seq, sl, EqxCount{});
    std::vector<uint8_t> out((size_t)ops * 4 + 4);
    eqx_walk_words(w, n, ref, rl, seq, sl, EqxStore{out.data(), ops});
    return out;
}

}  // namespace npore
