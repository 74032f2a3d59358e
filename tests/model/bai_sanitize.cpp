// tests/model/bai_sanitize.cpp -- TEST INFRASTRUCTURE.
// The .bai reader (csrc/hostio.hpp bai_linear_offsets) and the two places that trust it (csrc/bam_reader.hpp: the
// one-pass open, bam_set_share) on files that are no .bai, as a stand-alone program for AddressSanitizer and UBSan
// (tests/test_bai_trust.py builds it with g++ -fsanitize=address,undefined and runs it with a cap on the size of one
// allocation, so that a vector sized by an unchecked count is an error).
//
//     bai_sanitize BAM CASES
//
// CASES: per case  int32 length | the bytes.  Every case is written beside the BAM as BAM.bai and must be refused:
// bai_linear_offsets says false, a one-pass handle takes no contig for empty and remembers no index, bam_set_share of
// both ranks of two says NPORE_E_UNSUPPORTED.  Prints the number of cases; exit status 1 names the first that is not.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../npore_amd/csrc/bam_reader.hpp"

using namespace npore;

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: bai_sanitize BAM CASES\n"); return 2; }
    const std::string bam = argv[1], bai = bam + ".bai";
    MappedFile cases;
    if (!cases.open(argv[2])) { std::fprintf(stderr, "cannot read '%s'\n", argv[2]); return 2; }
    int n = 0;
    for (size_t q = 0; q + 4 <= cases.n; n++) {
        const int32_t len = rdi32(cases.p + q);
        q += 4;
        if (len < 0 || q + (size_t)len > cases.n) { std::fprintf(stderr, "bad case file\n"); return 2; }
        FILE *fh = std::fopen(bai.c_str(), "wb");
        if (!fh || std::fwrite(cases.p + q, 1, (size_t)len, fh) != (size_t)len || std::fclose(fh) != 0) { std::fprintf(stderr, "cannot write '%s'\n", bai.c_str()); return 2; }
        q += (size_t)len;
        std::vector<uint64_t> offs;
        std::vector<uint8_t> has;
        const bool parses = bai_linear_offsets(bai.c_str(), offs, &has);
        std::unique_ptr<npore_bam> b(bam_open(bam.c_str(), 2, 3, nullptr));
        if (!b) { std::printf("case %d: the BAM does not open: %s\n", n, g_err.c_str()); return 1; }
        // (a file that parses is still no index of this BAM where its n_ref is not the header's: the callers' rule)
        if (parses && has.size() == b->ref_names.size()) { std::printf("case %d (%d bytes): bai_linear_offsets accepts it\n", n, len); return 1; }
        if (!b->has_reads_index.empty()) { std::printf("case %d (%d bytes): the handle trusts the index\n", n, len); return 1; }
        for (uint8_t h : b->ref_has_reads)
            if (!h) { std::printf("case %d (%d bytes): a contig taken for empty\n", n, len); return 1; }
        for (int rank = 0; rank < 2; rank++) {
            const int rc = bam_set_share(b.get(), rank, 2, bai.c_str());
            if (rc != NPORE_E_UNSUPPORTED || b->has_share) { std::printf("case %d (%d bytes): bam_set_share(%d of 2) = %d\n", n, len, rank, rc); return 1; }
        }
    }
    std::remove(bai.c_str());
    std::printf("%d\n", n);
    return 0;
}
