// tests/model/purity_rec.cpp -- TEST INFRASTRUCTURE.
// The host twin of the device purity route: the rule of npore_amd/csrc/purity_rec.hpp built with plain g++ (no GPU, no HIP
// header in reach) over the records of a BAM file read by the product's reader (bam_reader.hpp, resident handle), one
// record after the other, one position after the other, all positions of all contigs in one "window".
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
struct HostSink {
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

const char *pur_twin_last_error(void) { return g_err.c_str(); }
uint64_t pur_twin_key(const uint8_t *sq, int64_t q0, uint32_t k) { return pur_key(sq, q0, k); }
int pur_twin_bin(uint64_t S, uint64_t n) { return pur_bin(S, n); }

// ranges (ref_id, start, stop)[n_ranges]; rows [n_pos][4] = (n, S_b, t, S_i) per merged position, contigs in header order
int pur_twin(const char *path, int64_t n_ranges, const int32_t *ref_id, const int64_t *start, const int64_t *stop, int min_bq,
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
        const int g = cms_gate((uint32_t)r.flag(), r.pos(), r.l_seq(), r.cigar(), r.n_cigar(), exclude_flags, rs.data(), one_layer, 1);
        if (g > 0) tallies[g]++;
        if (g != 0) continue;
        tallies[PUR_T_RECORDS]++;
        tallies[PUR_T_INS_NO_ENTRY] += pur_ins_no_entry(r.cigar(), r.n_cigar());
        PurView v;
        v.cg = r.cigar();
        v.nc = r.n_cigar();
        v.sq = r.seq();
        v.ql = r.qual();
        v.l_seq = r.l_seq();
        v.ranges = rs.data();
        v.n_ranges = (int)rs.size();
        v.win_lo = 0;
        v.win_hi = P;
        v.min_bq = min_bq;
        HostSink sink{cnt.data(), base[(size_t)rid], &events, tallies};
        int64_t a = r.pos(), q = 0;
        int hint = -1;
        for (int j = 0; j < v.nc; j++) {
            const uint32_t w = r.cig(j), op = w & 15u, len = w >> 4;
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
