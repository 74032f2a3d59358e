// confusion_rec.hpp -- basecaller error profile straight from BAM records: the counting rule, stated ONCE and compiled
// for the gfx950 kernel (confusion_kernels.hpp: one workgroup per record) and for a host twin (tests/model/confusion_rec.cpp,
// plain g++), the way std_stream.hpp is.  No pileup text exists at any point.
//
// What confusion.hpp counts from column 5 of `samtools mpileup` is, for all but one corner, a sum of independent
// contributions of the entries of the pileup columns, and an entry belongs to exactly one record.  So the records are
// walked along their CIGARs against the contig instead:
//   * every reference position `a` under an M / = / X operation is a BASE ENTRY (read base, quality);
//   * positions under D give nothing (the `*` of a pileup);
//   * the base entry on the LAST position of its M / = / X operation carries a marker when the next operation is I (+k,
//     with the k inserted read bases) or D (-k); S, H and operations of length 0 are stepped over on the way;
//   * an I or D with no base entry to sit on (behind another I / D, or leading) gives nothing and is tallied
//     (CMS_T_ADJACENT): pileup programs differ by version exactly there, and where they hang the marker on a `*` entry the
//     reference's was_ins / was_del state makes the counts depend on the ORDER of the reads of the column.  This rule is
//     free of order;
//   * a record whose CIGAR holds N or P is left out whole (CMS_T_REFSKIP: the reference's loop drops the rest of a line on
//     `>` / `<`), so is one whose CIGAR does not consume exactly l_seq bases (CMS_T_MALFORMED) or that fails the flags.
// A base entry is counted when its quality is at least min_bq (0xFF = missing passes; a dropped entry takes its marker
// with it), its letter is one of A C G T N (anything else: CMS_T_AMBIGUOUS), and `a` lies in a range (ctg, st, en) of the
// caller, st <= a < en.  Then, with the n-polymer annotation of the SLICE refs[ctg][st:en+1] at index a - st + 1 (a
// polymer cut by a range border counts as calc_confusion_matrices counts it), it adds what confusion_count_line adds for
// an entry between two entries without markers: subs always; inss[0], dels[0] and the diagonal nps[n-1][L][L] of every
// start period without a marker; the period loop and the dels / inss fall-back of confusion.hpp:79-118 with one.
// Position-true: a position nobody covers adds nothing (the text route's shift behind a coverage gap is not reproduced).
//
// The annotation is read as one byte plane per period and slice, L | start << 7 (annot_wave.hpp ANNOT_PLANES).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NPORE_CMS_HD __host__ __device__ __forceinline__
#else
#define NPORE_CMS_HD inline
#endif

namespace npore {

enum : int {
    CMS_T_RECORDS = 0,     // records walked
    CMS_T_FLAGGED = 1,     // records dropped by exclude_flags
    CMS_T_REFSKIP = 2,     // records with N / P in the CIGAR
    CMS_T_MALFORMED = 3,   // records whose CIGAR and l_seq disagree (SEQ `*` among them)
    CMS_T_ADJACENT = 4,    // I / D operations without a base entry to sit on
    CMS_T_AMBIGUOUS = 5,   // base entries with a letter outside ACGTN
    CMS_T_LOWQ = 6,        // base entries below min_bq
    CMS_T_COUNTED = 7,     // base entries counted
    CMS_T_BATCHES = 8,     // (device) batches of records
    CMS_T_KERNEL_NS = 9,   // (device) time of the counting kernels alone, by events
    CMS_N_TALLIES = 16
};

// A range of one contig and where its slice's annotation lies: plane n - 1 at planes + ann + (n - 1) * slen, slen =
// len(refs[ctg][st:en+1]).  The ranges of a contig come in LAYERS: within a layer ascending and disjoint (overlapping
// ranges of the caller -- each counts its positions on its own, as the sum over ranges does -- go to different layers).
struct CmsRange {
    int64_t st, en, ann, slen;
};

// a caller's range [start, stop) on a contig of clen bases: clipped to the contig, its slice contig[st : en + 1] measured.
// false: nothing of it lies on the contig
NPORE_CMS_HD bool cms_clip(int64_t start, int64_t stop, int64_t clen, CmsRange &r)
{
    r.st = start < 0 ? 0 : start;
    r.en = stop < clen ? stop : clen;
    r.ann = 0;
    r.slen = (r.en + 1 < clen ? r.en + 1 : clen) - r.st;
    return r.st < r.en;
}

struct CmsView {
    const uint8_t *cg;     // CIGAR words (little-endian, unaligned)
    int nc;
    const uint8_t *sq;     // 4-bit bases
    const uint8_t *ql;     // qualities
    int64_t l_seq;
    const char *contig;    // upper-cased
    int64_t clen;
    const CmsRange *ranges;
    const int32_t *layer_off;   // [n_layers + 1]
    int n_layers;
    const uint8_t *planes;
    int max_n, max_l, min_bq;
};

NPORE_CMS_HD uint32_t cms_ld32(const uint8_t *q)
{
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
}
NPORE_CMS_HD bool cms_op_match(uint32_t op) { return op == 0 || op == 7 || op == 8; }
NPORE_CMS_HD bool cms_op_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
NPORE_CMS_HD bool cms_op_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
// stepped over when looking for an operation's neighbour
NPORE_CMS_HD bool cms_op_transparent(uint32_t w) { return (w >> 4) == 0 || (w & 15u) == 4 || (w & 15u) == 5; }

NPORE_CMS_HD int cms_ref_code(char c)     // base_to_int of the contig: 'NACGT' -> 0..4, anything else 0
{
    return (c == 'A' ? 1 : 0) + (c == 'C' ? 2 : 0) + (c == 'G' ? 3 : 0) + (c == 'T' ? 4 : 0);
}
NPORE_CMS_HD int cms_read_code(uint32_t nib)     // "=ACMGRSVTWYHKDBN"[nib] -> 'NACGT' code, -1: not one of them
{
    return nib == 1 ? 1 : nib == 2 ? 2 : nib == 4 ? 3 : nib == 8 ? 4 : nib == 15 ? 0 : -1;
}
NPORE_CMS_HD char cms_read_char(uint32_t nib)
{
    return "=ACMGRSVTWYHKDBN"[nib & 15u];
}
NPORE_CMS_HD uint32_t cms_nibble(const uint8_t *sq, int64_t i)
{
    const uint32_t b = sq[i >> 1];
    return (i & 1) ? (b & 15u) : (b >> 4);
}

// What the record gate needs of a CIGAR: reference and query lengths, whether it holds N / P.
struct CmsSpan {
    int64_t rl, ql;
    bool refskip;
};
NPORE_CMS_HD CmsSpan cms_span(const uint8_t *cg, int nc)
{
    CmsSpan s{0, 0, false};
    for (int c = 0; c < nc; c++) {
        const uint32_t w = cms_ld32(cg + 4 * (int64_t)c), op = w & 15u;
        if (cms_op_ref(op)) s.rl += w >> 4;
        if (cms_op_query(op)) s.ql += w >> 4;
        if (op == 3 || op == 6) s.refskip = true;
    }
    return s;
}

// index of the range of [lo, hi) that holds a, or -1
NPORE_CMS_HD int cms_find_range(const CmsRange *r, int lo, int hi, int64_t a)
{
    int l = lo, h = hi;                    // last range with st <= a
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (r[mid].st <= a) l = mid + 1; else h = mid;
    }
    return (l > lo && a < r[l - 1].en) ? l - 1 : -1;
}
NPORE_CMS_HD bool cms_overlaps(const CmsRange *r, const int32_t *layer_off, int n_layers, int64_t pos, int64_t end)
{
    for (int y = 0; y < n_layers; y++) {
        const int lo = layer_off[y], hi = layer_off[y + 1];
        int l = lo, h = hi;                // first range with en > pos
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (r[mid].en > pos) h = mid; else l = mid + 1;
        }
        if (l < hi && r[l].st < end) return true;
    }
    return false;
}

// 0: the record is walked; -1: it is none of the ranges' records (its reference span overlaps no range: no tally); else the
// tally it goes to.  flag, pos, l_seq: the record's fixed fields.
NPORE_CMS_HD int cms_gate(uint32_t flag, int64_t pos, int64_t l_seq, const uint8_t *cg, int nc, uint32_t exclude_flags,
                          const CmsRange *ranges, const int32_t *layer_off, int n_layers)
{
    const CmsSpan s = cms_span(cg, nc);
    if (pos < 0 || s.rl <= 0 || pos + s.rl >= (1ll << 31) || !cms_overlaps(ranges, layer_off, n_layers, pos, pos + s.rl)) return -1;
    if (flag & exclude_flags) return CMS_T_FLAGGED;
    if (s.refskip) return CMS_T_REFSKIP;
    if (s.ql != l_seq) return CMS_T_MALFORMED;
    return 0;
}

// the marker of the base entry on the last position of operation j: 0 none, 1 = +k, 2 = -k.  qskip: the read bases of the
// S operations stepped over on the way (none in a well-formed record, where S stands only at the ends: the inserted
// bases of a +k marker begin qskip + 1 behind the entry's own base)
NPORE_CMS_HD int cms_marker(const uint8_t *cg, int nc, int j, uint32_t &k, int64_t &qskip)
{
    qskip = 0;
    for (int c = j + 1; c < nc; c++) {
        const uint32_t w = cms_ld32(cg + 4 * (int64_t)c);
        if (cms_op_transparent(w)) {
            if ((w & 15u) == 4) qskip += w >> 4;
            continue;
        }
        k = w >> 4;
        return (w & 15u) == 1 ? 1 : (w & 15u) == 2 ? 2 : 0;
    }
    return 0;
}
// operation j is an I / D (of length > 0) with no base entry to sit on
NPORE_CMS_HD bool cms_adjacent(const uint8_t *cg, int nc, int j)
{
    const uint32_t w = cms_ld32(cg + 4 * (int64_t)j);
    if (((w & 15u) != 1 && (w & 15u) != 2) || (w >> 4) == 0) return false;
    for (int c = j - 1; c >= 0; c--) {
        const uint32_t v = cms_ld32(cg + 4 * (int64_t)c);
        if (cms_op_transparent(v)) continue;
        return !cms_op_match(v & 15u);
    }
    return true;
}

// What a counted entry at contig position a adds (confusion.hpp:72-118 for an entry whose neighbours carry no marker).
// Sink: sub(ref, read), ins(i), del(i), np(n_idx, from, to), tally(which).  rg: the range that holds a; qins: where the
// inserted bases of a +k marker begin in the read.
template <class Sink>
NPORE_CMS_HD void cms_count(const CmsView &v, Sink &s, const CmsRange &rg, int64_t a, int code, int marker, uint32_t k, int64_t qins)
{
    s.tally(CMS_T_COUNTED);
    s.sub(cms_ref_code(v.contig[a]), code);
    const int64_t idx = a - rg.st + 1;
    const uint8_t *pl = v.planes + rg.ann + idx;
    const bool have = idx < rg.slen;                    // (zeros past the slice, like L_at)
    if (marker != 1) s.ins(0);
    if (marker != 2) s.del(0);
    bool cnv = false;
    const int64_t kk = (int64_t)k;
    for (int n = 1; n <= v.max_n; n++) {
        const uint32_t byte = have ? pl[(int64_t)(n - 1) * rg.slen] : 0u;
        if (!(byte & 128u)) continue;                   // not a start: L == 0 or L_IDX != 0
        const int l = (int)(byte & 127u);
        if (marker == 0) {
            s.np(n - 1, l, l);
        } else if (marker == 2) {
            if (kk % n == 0 && kk <= (int64_t)l * n) {
                cnv = true;
                s.np(n - 1, l, (int)(l - kk / n));
            } else {
                s.np(n - 1, l, l);
            }
        } else {
            bool same = false;
            if (kk % n == 0) {
                // contig[a+1 : a+1+n] * (k / n) == the inserted letters (Python slices clip at the contig's end).  The clip
                // (ulen < n) cannot run on a true annotation -- a start at slice index a - st + 1 has L >= 3 whole repeats
                // of n bases inside the slice -- and a clipped unit never compares equal (ulen * (k / n) < k); it is kept
                // so that the statement equals confusion_count_line on ANY planes (tests: a hand-made plane, host twin)
                const int64_t u0 = a + 1, ulen = u0 >= v.clen ? 0 : (u0 + n <= v.clen ? n : v.clen - u0);
                same = ulen * (kk / n) == kk && qins + kk <= v.l_seq;
                int64_t u = 0;
                for (int64_t q = 0; same && q < kk; q++) {
                    same = cms_read_char(cms_nibble(v.sq, qins + q)) == v.contig[u0 + u];
                    u = u + 1 == ulen ? 0 : u + 1;
                }
            }
            if (same) {
                cnv = true;
                const int64_t to = l + kk / n;
                s.np(n - 1, l, (int)(to < v.max_l ? to : v.max_l));
            } else {
                s.np(n - 1, l, l);
            }
        }
    }
    if (!cnv && marker == 2) s.del((int)(kk < v.max_l ? kk : v.max_l));
    if (!cnv && marker == 1) s.ins((int)(kk < v.max_l ? kk : v.max_l));
}

// The base entry of operation j at contig position a, read index qi (last: on the operation's last position).
// hint: the range of the first layer found last (the positions a lane visits lie close together).
template <class Sink>
NPORE_CMS_HD void cms_entry(const CmsView &v, Sink &s, int j, int64_t a, int64_t qi, bool last, int &hint)
{
    if (a < 0 || a >= v.clen || qi < 0 || qi >= v.l_seq) return;
    for (int y = 0; y < v.n_layers; y++) {
        const int lo = v.layer_off[y], hi = v.layer_off[y + 1];
        int g;
        if (y == 0 && hint >= lo && hint < hi && v.ranges[hint].st <= a && a < v.ranges[hint].en) g = hint;
        else g = cms_find_range(v.ranges, lo, hi, a);
        if (g < 0) continue;
        if (y == 0) hint = g;
        const uint32_t q = v.ql[qi];
        if (q != 0xFFu && (int)q < v.min_bq) { s.tally(CMS_T_LOWQ); continue; }
        const int code = cms_read_code(cms_nibble(v.sq, qi));
        if (code < 0) { s.tally(CMS_T_AMBIGUOUS); continue; }
        uint32_t k = 0;
        int64_t qskip = 0;
        const int marker = last ? cms_marker(v.cg, v.nc, j, k, qskip) : 0;
        cms_count(v, s, v.ranges[g], a, code, marker, k, qi + 1 + qskip);
    }
}

}  // namespace npore
