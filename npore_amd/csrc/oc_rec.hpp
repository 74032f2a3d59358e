// oc_rec.hpp -- the OC tag of a realigned read (BAM out, FULL records with NPORE_TAG_OC, `--oc`): the read's ORIGINAL CIGAR, kept
// on the reads whose alignment the run CHANGED, as the realigners that rewrite CIGARs in place keep it.  The rule, stated ONCE
// and compiled for the gfx950 kernels (bam_emit_kernels.hpp oc_size_kernel / emit_oc_kernel) and for the host twin
// (bam_reader.hpp format_bam_into, plain g++), the way md_rec.hpp and eqx_rec.hpp are.
//
// The input is the read's real CIGAR words in[0, nc) (`len << 4 | op`; those of the CG tag for a long-CIGAR record -- what the
// staged head carries, hostio.hpp stage_record_head), its clip words [0, ci) and [cj, nc) (bam_reader.hpp full_clip_words) and
// its FINAL words fin[0, nf) in M form, before any =/X split.  Two parts:
//
// CHANGED.  The canonical form of in[ci, cj):
//     a word of length 0 is dropped;
//     the ops = (7) and X (8) read as M (0);
//     neighbouring words of equal op are merged, their lengths added in 64 bits.
//   The read is UNCHANGED iff that is fin word for word, with the same count.  (eqx_rec.hpp says that a final CIGAR is the
//   canonical M form of something; this asks whether it is the canonical form of the input.)  So
//     - an input in =/X form that realigns to the same alignment is unchanged, with or without NPORE_CIGAR_EQX;
//     - `3M0I2M` against `5M` is unchanged;
//     - an input `...1I1D...` is changed whenever the final has M there;
//     - nothing else enters: not NPORE_CIGAR_EQX, not MD, not the tags.
//   fin is taken as it stands: a caller's final that is not in canonical M form equals no canonical form.
//
// TEXT.  For a changed read every word of in[0, nc) as it stands: its length in decimal, its letter of "MIDNSHP=X" ('?' for
//   the seven codes a CIGAR does not define).  Clips and words of length 0 included, nothing merged, nothing mapped.  The tag is
//   'O' 'C' 'Z' text NUL -- 4 + text bytes -- behind NM, MD, cs and de and in front of CG:B,I.  The position never changes here, so
//   OC alone restores the record and there is no OP.
//
// Size.  A word's length has at most 9 digits (28 bits), so the text has at most 10 bytes per word: oc_tag_bound (hostio.hpp).
//
// The text goes to a SINK as MD's does (md_rec.hpp MdCount / MdStore, md_digits, md_put_decimal: 10 digits, more than the 9 a
// length needs).  The device walk (bam_emit_kernels.hpp oc_walk) places a tile's words in parallel, this file's oc_walk_words one
// after the other; both end at the same length with the same bytes.  The device decides CHANGED in parallel, too
// (bam_emit_kernels.hpp oc_changed), with the same answer as oc_changed_words.
#pragma once
#include <stdint.h>

#include <string>

#include "md_rec.hpp"

namespace npore {

using OcCount = MdCount;
using OcStore = MdStore;

// the op as the canonical form reads it
NPORE_NM_HD uint32_t oc_canon_op(uint32_t op) { return (op == 7u || op == 8u) ? 0u : op; }
NPORE_NM_HD uint8_t oc_letter(uint32_t op) { return (uint8_t)"MIDNSHP=X???????"[op & 15u]; }
NPORE_NM_HD uint32_t oc_word(const uint8_t *w, int64_t c)      // little-endian, unaligned
{
    return (uint32_t)w[4 * c] | (uint32_t)w[4 * c + 1] << 8 | (uint32_t)w[4 * c + 2] << 16 | (uint32_t)w[4 * c + 3] << 24;
}

// CHANGED, sequentially: the canonical form of in[ci, cj) against the nf words at fin
inline bool oc_changed_words(const uint8_t *in, int64_t ci, int64_t cj, const uint8_t *fin, int64_t nf)
{
    int64_t runs = 0;            // runs of the canonical form begun; the last one is open
    uint32_t rop = 0;
    uint64_t rlen = 0;
    auto differs = [&]() {       // the open run against the final word in its place
        if (runs > nf) return true;
        const uint32_t f = oc_word(fin, runs - 1);
        return (f & 15u) != rop || (uint64_t)(f >> 4) != rlen;
    };
    for (int64_t c = ci; c < cj; c++) {
        const uint32_t v = oc_word(in, c), op = oc_canon_op(v & 15u), len = v >> 4;
        if (len == 0) continue;
        if (runs > 0 && op == rop) { rlen += len; continue; }
        if (runs > 0 && differs()) return true;
        runs++;
        rop = op;
        rlen = len;
    }
    if (runs > 0 && differs()) return true;
    return runs != nf;
}

// TEXT of the nc words at `in`, sequentially, into the sink: its length (no NUL)
template <class Sink>
inline int64_t oc_walk_words(const uint8_t *in, int64_t nc, const Sink &sink)
{
    int64_t at = 0;
    for (int64_t c = 0; c < nc; c++) {
        const uint32_t v = oc_word(in, c);
        const int nd = md_digits(v >> 4);
        md_put_decimal(sink, at, v >> 4, nd);
        sink.put(at + nd, oc_letter(v & 15u));
        at += nd + 1;
    }
    return at;
}
// ... the whole tag -- 'O' 'C' 'Z' text NUL -- appended to `out`: sized and then written
inline void oc_tag_of_words(const uint8_t *in, int64_t nc, std::string &out)
{
    const int64_t size = oc_walk_words(in, nc, OcCount{});
    const size_t at = out.size();
    out.append("OCZ").append((size_t)size + 1, '\0');
    oc_walk_words(in, nc, OcStore{reinterpret_cast<uint8_t *>(&out[at + 3]), size});
}

}  // namespace npore
