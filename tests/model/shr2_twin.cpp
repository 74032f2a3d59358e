// tests/model/shr2_twin.cpp -- TEST INFRASTRUCTURE.
// The host twin of the fill (pull_model.cpp: the product's cell recurrence, cell by cell) with the two hooks of
// cell.hpp's two-candidate block defined: for every cell whose column carries a second SHR candidate it notes the
// anti-diagonal (the block's incoming SHR value is 100 b, exactly), the band column, the chunk-local reference column
// and what the block decided -- whether the first candidate was taken, whether the second was, and both candidate
// values.  tests/offpath_cases.py maps the notes to wave roles and steps of the text.
#include <cstdint>
#include <vector>

namespace {
struct Shr2Note { int32_t bl, c, j, take0, take1, equal; };
std::vector<Shr2Note> g_notes;
float g_entry = 0.f;
inline void shr2_note(int c, int j, bool act1, bool take0, bool take1, float cand0, float cand1)
{
    if (act1) g_notes.push_back(Shr2Note{(int32_t)(g_entry / 100.0f + 0.5f), c, j, take0, take1, cand0 == cand1});
}
}  // namespace
#define NPORE_SHR2_ENTRY(shrv_in) (g_entry = (shrv_in))
#define NPORE_SHR2_NOTE(c, j, act1, take0, take1, cand0, cand1) shr2_note(c, j, act1, take0, take1, cand0, cand1)

#include "pull_model.cpp"

// the notes of one read (six int32 each: anti-diagonal of its chunk, band column, local reference column, first taken,
// second taken, candidate values equal), in the order the cells were computed: chunk after chunk, row after row
extern "C" int64_t shr2_twin_notes(const uint8_t *ref, int64_t ref_len, const uint8_t *seq, int64_t seq_len, const char *cigar,
                                   int64_t cig_len, const float *sub_scores, const float *np_scores, int max_n, int max_l,
                                   float indel_start, float indel_extend, int max_b_rows, int r, int32_t *out, int64_t cap)
{
    g_notes.clear();
    std::vector<char> buf((size_t)(ref_len + seq_len + 16));
    int32_t status = 0;
    if (pull_model_align(ref, ref_len, seq, seq_len, cigar, cig_len, sub_scores, np_scores, max_n, max_l, indel_start,
                         indel_extend, max_b_rows, r, buf.data(), (int64_t)buf.size(), &status) < 0)
        return -1;
    const int64_t n = (int64_t)g_notes.size();
    for (int64_t k = 0; k < n && k < cap; k++) {
        const Shr2Note &x = g_notes[k];
        int32_t *o = out + 6 * k;
        o[0] = x.bl; o[1] = x.c; o[2] = x.j; o[3] = x.take0; o[4] = x.take1; o[5] = x.equal;
    }
    return n;
}
