// purity_rec.hpp -- Gini purity of pileups straight from BAM records: the rule, stated ONCE and compiled for the gfx950
// kernels (purity_kernels.hpp) and for a host twin (tests/model/purity_rec.cpp, plain g++), the way confusion_rec.hpp is.
// It is the walk of confusion_rec.hpp with another sink: counters per reference position instead of per matrix cell.  No
// pileup text exists at any point, no FASTA and no n-polymer annotation are needed.
//
// What the reference's src/purity.py computes from column 5 of `samtools mpileup` (upper-cased) is, per column, the
// multiset of the symbols A C G T * and the multiset of the inserted strings.  Here:
//   * a record passes cms_gate (confusion_rec.hpp): its span overlaps a range, it is not dropped by exclude_flags, its
//     CIGAR holds no N / P and consumes exactly l_seq bases;
//   * every reference position `a` under M / = / X is a BASE ENTRY with the read's letter: A C G T count, any other
//     letter (N included) drops the entry (PUR_T_AMBIGUOUS: the reference's loop stops a column at such a character);
//     an entry whose quality is below min_bq is dropped (PUR_T_LOWQ; 0xFF = missing passes);
//   * every position under D is a `*` ENTRY -- the difference from the confusion rule.  It has no quality of its own: it
//     takes the quality of the read base consumed last before the deletion (none: it passes), so a deletion is kept or
//     dropped together with the entry that carries its -k marker; the marker itself counts nothing;
//   * the base entry on the LAST position of an M-type operation carries +k when the next non-transparent operation is I
//     (cms_marker): a counted entry with +k adds one insertion of its k letters at `a`; a dropped entry takes the
//     insertion with it; an I with no base entry to sit on (behind a D, or leading) is not counted (PUR_T_INS_NO_ENTRY,
//     the choice of CMS_T_ADJACENT for the same reason);
//   * strand is ignored (the reference upper-cases the column).
// Per position: n entries counted (`*` included), S_b = sum of c_b^2 over the five symbols, t insertions,
// S_i = (n - t)^2 + sum of v^2 over the distinct inserted strings.  n = 0 gives nothing.
//
// Inserted strings are compared by a 64-bit KEY (pur_key): for k <= 14, k in the top byte and the 4-bit BAM codes below
// it (injective); for longer strings 0xFF in the top byte and a 56-bit hash of k and all codes -- two DIFFERENT long
// strings at one position whose hashes collide are merged into one (PUR_T_INS_HASHED counts the long ones).
//
// Bins are integer-exact (pur_bin): the reference files a score x = S / n^2 under int(x * 100 - 0.00001); here
// bin = (10^7 S - n^2) / (10^5 n^2) in unsigned 64-bit integers (0 where the numerator would be negative), which
// overflows nowhere for n < 2^20 (PUR_MAX_DEPTH); a deeper position is not binned (PUR_T_TOO_DEEP).  The exact value lies
// at least 1 / (10^5 n^2) from a bin's edge, so this equals the floating-point expression at any realistic depth.
#pragma once
#include <stdint.h>

#include "confusion_rec.hpp"

namespace npore {

enum : int {
    PUR_T_RECORDS = 0,       // records walked            (0..3 are cms_gate's return values)
    PUR_T_FLAGGED = 1,       // records dropped by exclude_flags
    PUR_T_REFSKIP = 2,       // records with N / P in the CIGAR
    PUR_T_MALFORMED = 3,     // records whose CIGAR and l_seq disagree
    PUR_T_INS_NO_ENTRY = 4,  // I operations without a base entry to sit on
    PUR_T_AMBIGUOUS = 5,     // base entries with a letter outside ACGT
    PUR_T_LOWQ = 6,          // entries (`*` among them) below min_bq
    PUR_T_COUNTED = 7,       // entries counted, `*` included
    PUR_T_STAR = 8,          // ... of them `*`
    PUR_T_INS = 9,           // insertions counted
    PUR_T_INS_HASHED = 10,   // ... of them longer than 14 letters (compared by hash)
    PUR_T_COVERED = 11,      // positions with n > 0
    PUR_T_TOO_DEEP = 12,     // positions with n >= 2^20: not binned
    PUR_T_WINDOWS = 13,      // (device) counter windows that held something
    PUR_T_BATCHES = 14,      // (device) batches of records
    PUR_T_KERNEL_NS = 15,    // (device) time of the kernels alone, by events
    PUR_N_TALLIES = 16
};

constexpr int64_t PUR_MAX_DEPTH = 1ll << 20;
constexpr int PUR_BINS = 100;
constexpr int PUR_STAR = 4;                      // symbols: A C G T *

// The ranges of one contig, MERGED: ascending and disjoint, CmsRange.ann = the dense index of the range's first position
// (the positions of the ranges packed one behind the other), slen = en - st.  One layer for cms_gate.
struct PurView {
    const uint8_t *cg;
    int nc;
    const uint8_t *sq, *ql;
    int64_t l_seq;
    const CmsRange *ranges;
    int n_ranges;
    int64_t win_lo, win_hi;    // dense positions [win_lo, win_hi) are this pass's; the others are another window's
    int min_bq;
};

NPORE_CMS_HD uint64_t pur_mix(uint64_t h, uint64_t x)      // (splitmix64's finaliser over a running state)
{
    h += 0x9E3779B97F4A7C15ull + x;
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    return h ^ (h >> 31);
}
// the key of the k inserted letters sq[q0 .. q0 + k)
NPORE_CMS_HD uint64_t pur_key(const uint8_t *sq, int64_t q0, uint32_t k)
{
    if (k <= 14u) {
        uint64_t key = (uint64_t)k << 56;
        for (uint32_t i = 0; i < k; i++) key |= (uint64_t)cms_nibble(sq, q0 + i) << (4 * i);
        return key;
    }
    uint64_t h = pur_mix(0, k), w = 0;
    for (uint32_t i = 0; i < k; i++) {                      // sixteen codes to a word
        w |= (uint64_t)cms_nibble(sq, q0 + i) << (4 * (i & 15u));
        if ((i & 15u) == 15u || i + 1 == k) { h = pur_mix(h, w); w = 0; }
    }
    return (0xFFull << 56) | (h >> 8);
}

// the bin of S / n^2, 0 < n < PUR_MAX_DEPTH, S <= n^2
NPORE_CMS_HD int pur_bin(uint64_t S, uint64_t n)
{
    const uint64_t n2 = n * n, num = 10000000ull * S;
    return num < n2 ? 0 : (int)((num - n2) / (100000ull * n2));
}

// the dense index of the first / last position of [pos, end) that lies in a range; -1: none does
NPORE_CMS_HD int64_t pur_first_dense(const CmsRange *r, int n, int64_t pos, int64_t end)
{
    int l = 0, h = n;                      // first range with en > pos
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (r[mid].en > pos) h = mid; else l = mid + 1;
    }
    if (l >= n || r[l].st >= end) return -1;
    return r[l].ann + ((pos > r[l].st ? pos : r[l].st) - r[l].st);
}
NPORE_CMS_HD int64_t pur_last_dense(const CmsRange *r, int n, int64_t pos, int64_t end)
{
    int l = 0, h = n;                      // last range with st < end
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (r[mid].st < end) l = mid + 1; else h = mid;
    }
    if (l == 0 || r[l - 1].en <= pos) return -1;
    return r[l - 1].ann + ((end < r[l - 1].en ? end : r[l - 1].en) - 1 - r[l - 1].st);
}

// I operations of a record without a base entry to sit on (a matter of the record, not of a position: counted once per
// kept record, by whoever gates it)
NPORE_CMS_HD int pur_ins_no_entry(const uint8_t *cg, int nc)
{
    int n = 0;
    for (int j = 0; j < nc; j++)
        if ((cms_ld32(cg + 4 * (int64_t)j) & 15u) == 1u && cms_adjacent(cg, nc, j)) n++;
    return n;
}
// ... and its I operations of length > 0 altogether: an upper bound of the insertions it can add
NPORE_CMS_HD int pur_ins_ops(const uint8_t *cg, int nc)
{
    int n = 0;
    for (int j = 0; j < nc; j++) {
        const uint32_t w = cms_ld32(cg + 4 * (int64_t)j);
        if ((w & 15u) == 1u && (w >> 4) != 0u) n++;
    }
    return n;
}

// The entry of operation j (M-type or D, word w) at contig position a.  q: the read index of the entry's own base (M-type)
// or of the base that FOLLOWS the deletion (D); last: on the operation's last position.  hint: the range found last.
// Sink: sym(dense, symbol), ins(dense, key), tally(which).
template <class Sink>
NPORE_CMS_HD void pur_entry(const PurView &v, Sink &s, int j, uint32_t w, int64_t a, int64_t q, bool last, int &hint)
{
    int g;
    if (hint >= 0 && hint < v.n_ranges && v.ranges[hint].st <= a && a < v.ranges[hint].en) g = hint;
    else g = cms_find_range(v.ranges, 0, v.n_ranges, a);
    if (g < 0) return;
    hint = g;
    const int64_t dense = v.ranges[g].ann + (a - v.ranges[g].st);
    if (dense < v.win_lo || dense >= v.win_hi) return;
    const bool star = (w & 15u) == 2u;
    const int64_t qi = star ? q - 1 : q;
    if (qi >= v.l_seq || (!star && qi < 0)) return;
    if (qi >= 0) {
        const uint32_t ql = v.ql[qi];
        if (ql != 0xFFu && (int)ql < v.min_bq) { s.tally(PUR_T_LOWQ); return; }
    }
    if (star) {
        s.tally(PUR_T_COUNTED);
        s.tally(PUR_T_STAR);
        s.sym(dense, PUR_STAR);
        return;
    }
    const int code = cms_read_code(cms_nibble(v.sq, qi));
    if (code < 1) { s.tally(PUR_T_AMBIGUOUS); return; }
    s.tally(PUR_T_COUNTED);
    s.sym(dense, code - 1);
    if (!last) return;
    uint32_t k = 0;
    int64_t qskip = 0;
    if (cms_marker(v.cg, v.nc, j, k, qskip) != 1) return;
    const int64_t q0 = qi + 1 + qskip;
    if (q0 + (int64_t)k > v.l_seq) return;
    s.tally(PUR_T_INS);
    if (k > 14u) s.tally(PUR_T_INS_HASHED);
    s.ins(dense, pur_key(v.sq, q0, k));
}

}  // namespace npore
