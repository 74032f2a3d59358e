// stage_twin.cpp -- the host side of the staged record heads (csrc/hostio.hpp stage_record_head) and their one reader
// (csrc/staged_head.hpp staged_cigar) compiled by g++ for tests/test_long_cigar.py: what the kernels are handed for the
// records of two BAM files, compared.
#include "../../npore_amd/csrc/bam_reader.hpp"
#include "../../npore_amd/csrc/staged_head.hpp"

#include <memory>
#include <vector>

using namespace npore;

extern "C" {

// The records of the two files pairwise, with and without qualities: the staged heads must have the same size and the same
// bytes behind the block_size word, and staged_cigar must hand back rec_cigar's words and the bases behind them.
// Returns the number of records compared, -1 - k when record k fails, INT64_MIN when a file cannot be read or the files
// hold different numbers of records.  ops (may be null): per record the operations of its staged CIGAR.
int64_t stage_twin_compare(const char *path_a, const char *path_b, int64_t *ops, int64_t cap)
{
    std::unique_ptr<npore_bam> a(bam_open(path_a, 2, 1, nullptr)), b(bam_open(path_b, 2, 1, nullptr));
    if (!a || !b || a->rec_off.size() != b->rec_off.size()) return INT64_MIN;
    for (size_t i = 0; i < a->rec_off.size(); i++)
        for (int quals = 0; quals < 2; quals++) {
            const uint8_t *ra = a->data + a->rec_off[i], *rb = b->data + b->rec_off[i];
            const int64_t na = staged_head_bytes(ra, quals != 0), nb = staged_head_bytes(rb, quals != 0);
            if (na != nb) return -1 - (int64_t)i;
            std::vector<uint8_t> sa((size_t)na + 8, 0xEE), sb((size_t)nb + 8, 0xEE);      // (8 guard bytes: nothing is written behind the head)
            stage_record_head(ra, quals != 0, sa.data());
            stage_record_head(rb, quals != 0, sb.data());
            if (std::memcmp(sa.data() + 4, sb.data() + 4, (size_t)na + 4)) return -1 - (int64_t)i;
            const uint8_t *cg, *sq;
            int nc;
            staged_cigar(sb.data() + 4, cg, nc, sq);
            const RecView r = rec_view(rb);
            const RecCigar rc = rec_cigar(r);
            const int64_t tail = (int64_t)((quals ? r.aux() : r.qual()) - r.seq());
            if ((uint32_t)nc != rc.n || std::memcmp(cg, rc.w, 4 * (size_t)nc) || sq + tail != sb.data() + na || std::memcmp(sq, r.seq(), (size_t)tail))
                return -1 - (int64_t)i;
            if (ops && (int64_t)i < cap) ops[i] = nc;
        }
    return (int64_t)a->rec_off.size();
}

}  // extern "C"
