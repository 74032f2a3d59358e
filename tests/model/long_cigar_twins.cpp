// tests/model/long_cigar_twins.cpp -- TEST INFRASTRUCTURE.
// The host twins of the recount (confusion_rec.cpp) and of the purity route (purity_rec.cpp) for records with long CIGARs:
// the same walks over the same rules (npore_amd/csrc/confusion_rec.hpp, purity_rec.hpp), built with plain g++, but every
// record's CIGAR is its REAL one -- rec_cigar (csrc/hostio.hpp): the words of the CG:B,I tag where the record carries the
// placeholder `<l_seq>S<reflen>N`.  The two older twins read the record's own CIGAR words and stay as they are; on a file
// without long CIGARs all four give the same.  Same arguments and results as cms_twin_count / pur_twin.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "../../npore_amd/csrc/bam_reader.hpp"
#include "../../npore_amd/csrc/purity_rec.hpp"

using namespace npore;

namespace {
struct CmsHostSink {
    int64_t *subs, *nps, *inss, *dels, *tallies;
    int dim;
    void sub(int r, int c) { subs[r * 5 + c]++; }
    void ins(int i) { inss[i]++; }
    void del(int i) { dels[i]++; }
    void np(int n_idx, int a, int b)
    {
        if (a >= 0 && a < dim && b >= 0 && b < dim) nps[((int64_t)n_idx * dim + a) * dim + b]++;
    }
    void tally(int which) { tallies[which]++; }
};
struct PurHostSink {
    int64_t *cnt;                                   // [P][5], dense offset by the contig's base
    int64_t base;
    std::vector<std::pair<int64_t, uint64_t>> *events;
    int64_t *tallies;
    void sym(int64_t dense, int s) { cnt[5 * (base + dense) + s]++; }
    void ins(int64_t dense, uint64_t key) { events->emplace_back(base + dense, key); }
    void tally(int which) { tallies[which]++; }
};
}  // namespace

extern "C" {

const char *long_cigar_twins_last_error(void) { return g_err.c_str(); }

// contigs / ctg_off[n_refs + 1]: the upper-cased contig of every BAM reference, back to back.  ranges: (ref_id, start, stop,
// ann)[n_ranges], ann = where the planes of the range's slice begin in `planes` (plane n - 1 at ann + (n - 1) * slen).
int cms_cg_twin_count(const char *path, const char *contigs, const int64_t *ctg_off, int n_refs, int64_t n_ranges, const int32_t *ref_id,
                   const int64_t *start, const int64_t *stop, const int64_t *ann, const uint8_t *planes, int max_n, int max_l,
                   int min_bq, uint32_t exclude_flags, int64_t *subs, int64_t *nps, int64_t *inss, int64_t *dels, int64_t *tallies)
try {
    std::unique_ptr<npore_bam> b(bam_open(path, 2, 1, nullptr));
    if (!b) return NPORE_E_INVALID;
    if ((int)b->ref_names.size() != n_refs) return fail(NPORE_E_INVALID, "contigs do not match the BAM header");
    std::vector<std::vector<CmsRange>> ranges((size_t)n_refs);
    for (int64_t k = 0; k < n_ranges; k++) {
        if (ref_id[k] < 0 || ref_id[k] >= n_refs) continue;
        CmsRange r;
        if (!cms_clip(start[k], stop[k], ctg_off[ref_id[k] + 1] - ctg_off[ref_id[k]], r)) continue;
        r.ann = ann[k];
        ranges[(size_t)ref_id[k]].push_back(r);
    }
    CmsHostSink sink{subs, nps, inss, dels, tallies, max_l + 1};
    for (size_t i = 0; i < b->rec_off.size(); i++) {
        const RecView r = rec_view(b->data + b->rec_off[i]);
        const int32_t rid = r.ref_id();
        if (rid < 0 || rid >= n_refs || ranges[(size_t)rid].empty()) continue;
        const std::vector<CmsRange> &rs = ranges[(size_t)rid];
        std::vector<int32_t> layer_off(rs.size() + 1);
        for (size_t y = 0; y <= rs.size(); y++) layer_off[y] = (int32_t)y;
        const RecCigar cg = rec_cigar(r);         // the CG tag's words for a long-CIGAR record
        const int g = cms_gate((uint32_t)r.flag(), r.pos(), r.l_seq(), cg.w, (int)cg.n, exclude_flags, rs.data(), layer_off.data(),
                               (int)rs.size());
        if (g > 0) tallies[g]++;
        if (g != 0) continue;
        tallies[CMS_T_RECORDS]++;
        CmsView v;
        v.cg = cg.w;
        v.nc = (int)cg.n;
        v.sq = r.seq();
        v.ql = r.qual();
        v.l_seq = r.l_seq();
        v.contig = contigs + ctg_off[rid];
        v.clen = ctg_off[rid + 1] - ctg_off[rid];
        v.ranges = rs.data();
        v.layer_off = layer_off.data();
        v.n_layers = (int)rs.size();
        v.planes = planes;
        v.max_n = max_n;
        v.max_l = max_l;
        v.min_bq = min_bq;
        int64_t a = r.pos(), q = 0;
        int hint = -1;
        for (int j = 0; j < v.nc; j++) {
            const uint32_t w = cg.op((uint32_t)j), op = w & 15u, len = w >> 4;
            if (cms_adjacent(v.cg, v.nc, j)) tallies[CMS_T_ADJACENT]++;
            if (cms_op_match(op))
                for (uint32_t t = 0; t < len; t++) cms_entry(v, sink, j, a + t, q + t, t + 1 == len, hint);
            if (cms_op_ref(op)) a += len;
            if (cms_op_query(op)) q += len;
        }
    }
    return NPORE_OK;
} catch (const std::exception &e) {
    return fail(NPORE_E_NOMEM, e.what());
}

// ranges (ref_id, start, stop)[n_ranges]; rows [n_pos][4] = (n, S_b, t, S_i) per merged position, contigs in header order
int pur_cg_twin(const char *path, int64_t n_ranges, const int32_t *ref_id, const int64_t *start, const int64_t *stop, int min_bq,
             uint32_t exclude_flags, int64_t *base_hist, int64_t *ins_hist, int64_t *rows, int64_t n_pos, int64_t *tallies)
try {
    std::unique_ptr<npore_bam> b(bam_open(path, 2, 1, nullptr));
    if (!b) return NPORE_E_INVALID;
    const int n_refs = (int)b->ref_names.size();
    std::vector<std::vector<CmsRange>> ranges((size_t)n_refs);
    for (int64_t k = 0; k < n_ranges; k++) {
        if (ref_id[k] < 0 || ref_id[k] >= n_refs) continue;
        CmsRange r;
        if (cms_clip(start[k], stop[k], b->ref_lens[(size_t)ref_id[k]], r)) ranges[(size_t)ref_id[k]].push_back(r);
    }
    std::vector<int64_t> base((size_t)n_refs, 0);
    int64_t P = 0;
    for (int c = 0; c < n_refs; c++) {
        std::vector<CmsRange> &rs = ranges[(size_t)c], merged;
        std::sort(rs.begin(), rs.end(), [](const CmsRange &a, const CmsRange &b2) { return a.st != b2.st ? a.st < b2.st : a.en < b2.en; });
        for (const CmsRange &r : rs) {
            if (!merged.empty() && r.st <= merged.back().en) merged.back().en = std::max(merged.back().en, r.en);
            else merged.push_back(r);
        }
        base[(size_t)c] = P;
        int64_t off = 0;
        for (CmsRange &r : merged) { r.ann = off; r.slen = r.en - r.st; off += r.slen; }
        P += off;
        rs = merged;
    }
    if (P != n_pos) return fail(NPORE_E_INVALID, "rows: the merged ranges have another number of positions");
    std::vector<int64_t> cnt((size_t)P * 5 + 1, 0);
    std::vector<std::pair<int64_t, uint64_t>> events;
    for (size_t i = 0; i < b->rec_off.size(); i++) {
        const RecView r = rec_view(b->data + b->rec_off[i]);
        const int32_t rid = r.ref_id();
        if (rid < 0 || rid >= n_refs || ranges[(size_t)rid].empty()) continue;
        const std::vector<CmsRange> &rs = ranges[(size_t)rid];
        const int32_t one_layer[2] = {0, (int32_t)rs.size()};
        const RecCigar cg = rec_cigar(r);         // the CG tag's words for a long-CIGAR record
        const int g = cms_gate((uint32_t)r.flag(), r.pos(), r.l_seq(), cg.w, (int)cg.n, exclude_flags, rs.data(), one_layer, 1);
        if (g > 0) tallies[g]++;
        if (g != 0) continue;
        tallies[PUR_T_RECORDS]++;
        tallies[PUR_T_INS_NO_ENTRY] += pur_ins_no_entry(cg.w, (int)cg.n);
        PurView v;
        v.cg = cg.w;
        v.nc = (int)cg.n;
        v.sq = r.seq();
        v.ql = r.qual();
        v.l_seq = r.l_seq();
        v.ranges = rs.data();
        v.n_ranges = (int)rs.size();
        v.win_lo = 0;
        v.win_hi = P;
        v.min_bq = min_bq;
        PurHostSink sink{cnt.data(), base[(size_t)rid], &events, tallies};
        int64_t a = r.pos(), q = 0;
        int hint = -1;
        for (int j = 0; j < v.nc; j++) {
            const uint32_t w = cg.op((uint32_t)j), op = w & 15u, len = w >> 4;
            if (cms_op_match(op))
                for (uint32_t t = 0; t < len; t++) pur_entry(v, sink, j, w, a + t, q + t, t + 1 == len, hint);
            else if (op == 2u)
                for (uint32_t t = 0; t < len; t++) pur_entry(v, sink, j, w, a + t, q, t + 1 == len, hint);
            if (cms_op_ref(op)) a += len;
            if (cms_op_query(op)) q += len;
        }
    }
    // per position: t and the sum of v^2 over the distinct keys
    std::sort(events.begin(), events.end());
    std::vector<int64_t> t((size_t)P + 1, 0), v2((size_t)P + 1, 0);
    for (size_t i = 0; i < events.size();) {
        size_t j = i;
        while (j < events.size() && events[j] == events[i]) j++;
        t[(size_t)events[i].first] += (int64_t)(j - i);
        v2[(size_t)events[i].first] += (int64_t)((j - i) * (j - i));
        i = j;
    }
    for (int64_t p = 0; p < P; p++) {
        int64_t n = 0, sb = 0;
        for (int s = 0; s < 5; s++) { n += cnt[(size_t)(5 * p + s)]; sb += cnt[(size_t)(5 * p + s)] * cnt[(size_t)(5 * p + s)]; }
        if (n == 0) continue;
        tallies[PUR_T_COVERED]++;
        rows[4 * p] = n;
        if (n >= PUR_MAX_DEPTH) {
            tallies[PUR_T_TOO_DEEP]++;
            rows[4 * p + 1] = rows[4 * p + 2] = rows[4 * p + 3] = -1;
            continue;
        }
        const int64_t si = (n - t[(size_t)p]) * (n - t[(size_t)p]) + v2[(size_t)p];
        rows[4 * p + 1] = sb;
        rows[4 * p + 2] = t[(size_t)p];
        rows[4 * p + 3] = si;
        base_hist[pur_bin((uint64_t)sb, (uint64_t)n)]++;
        ins_hist[pur_bin((uint64_t)si, (uint64_t)n)]++;
    }
    return NPORE_OK;
} catch (const std::exception &e) {
    return fail(NPORE_E_NOMEM, e.what());
}

}  // extern "C"
