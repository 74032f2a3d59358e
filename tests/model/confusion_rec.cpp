// tests/model/confusion_rec.cpp -- TEST INFRASTRUCTURE.
// The host twin of the device recount of the confusion matrices: the counting rule of npore_amd/csrc/confusion_rec.hpp built
// with plain g++ (no GPU, no HIP header in reach) over the records of a BAM file read by the product's reader
// (bam_reader.hpp, resident handle), one record after the other, one position after the other.  The annotation comes from
// the caller (the oracle's get_np_info, as byte planes); every range is a layer of its own here.
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../npore_amd/csrc/bam_reader.hpp"
#include "../../npore_amd/csrc/confusion_rec.hpp"

using namespace npore;

namespace {
struct HostSink {
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
}  // namespace

extern "C" {

const char *cms_twin_last_error(void) { return g_err.c_str(); }

// contigs / ctg_off[n_refs + 1]: the upper-cased contig of every BAM reference, back to back.  ranges: (ref_id, start, stop,
// ann)[n_ranges], ann = where the planes of the range's slice begin in `planes` (plane n - 1 at ann + (n - 1) * slen).
int cms_twin_count(const char *path, const char *contigs, const int64_t *ctg_off, int n_refs, int64_t n_ranges, const int32_t *ref_id,
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
    HostSink sink{subs, nps, inss, dels, tallies, max_l + 1};
    for (size_t i = 0; i < b->rec_off.size(); i++) {
        const RecView r = rec_view(b->data + b->rec_off[i]);
        const int32_t rid = r.ref_id();
        if (rid < 0 || rid >= n_refs || ranges[(size_t)rid].empty()) continue;
        const std::vector<CmsRange> &rs = ranges[(size_t)rid];
        std::vector<int32_t> layer_off(rs.size() + 1);
        for (size_t y = 0; y <= rs.size(); y++) layer_off[y] = (int32_t)y;
        const int g = cms_gate((uint32_t)r.flag(), r.pos(), r.l_seq(), r.cigar(), r.n_cigar(), exclude_flags, rs.data(), layer_off.data(),
                               (int)rs.size());
        if (g > 0) tallies[g]++;
        if (g != 0) continue;
        tallies[CMS_T_RECORDS]++;
        CmsView v;
        v.cg = r.cigar();
        v.nc = r.n_cigar();
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
            const uint32_t w = r.cig(j), op = w & 15u, len = w >> 4;
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

}  // extern "C"
