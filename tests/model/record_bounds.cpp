// tests/model/record_bounds.cpp -- TEST INFRASTRUCTURE.
// A stand-alone program for tests/test_bam_fuzz.py, built with plain g++: the record buffer's bound of one read, from the
// library's own function (csrc/hostio.hpp record_bound) and its two makers of a final's extent, as the file pipeline and the
// debug entry call it (csrc/file_pipeline.hpp plan_staged_heads), so what the test proves sufficient is the product's sum.  The file named on the command line holds seven int64 per read: l_read_name (the NUL counted), rl and sl (the reference positions and
// the unclipped bases of the packed read), l_seq, the kept aux bytes without and with the option oc (which drops the input's own
// OC: filter_aux), and the words of the input's real CIGAR.  Prints per read one line of 48 sums, one per option set, in the
// order of bam_fuzz_cases.OPTION_SETS: md slowest, then cs (none, short, long), de, eqx, oc fastest -- the bound of a batch's own
// final (own_final_extent).  A second file, if named, holds per read an int64 count and that many uint32 words of a caller's
// final: behind the lines above, per read one more line of 48 sums, the bound of those words (words_final_extent).  Exit code 0:
// all through; 2: bad input or an option set the rules refuse.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../npore_amd/csrc/hostio.hpp"

using namespace npore;

// the 48 sums of one read, its final of extent e
static bool print_sums(const int64_t *h, const FinalExtent &e)
{
    const int cs_bits[3] = {0, NPORE_TAG_CS, NPORE_TAG_CS | NPORE_TAG_CS_LONG};
    for (int md = 0; md < 2; md++)
        for (int cs = 0; cs < 3; cs++)
            for (int de = 0; de < 2; de++)
                for (int eqx = 0; eqx < 2; eqx++)
                    for (int oc = 0; oc < 2; oc++) {
                        RecSpec rec;
                        const int tags = cs_bits[cs] | (de ? NPORE_TAG_DE : 0) | (eqx ? NPORE_CIGAR_EQX : 0) | (oc ? NPORE_TAG_OC : 0);
                        if (!rec_spec_of(NPORE_OUT_BAM, NPORE_OUT_FULL | NPORE_OUT_EOF | (md ? NPORE_OUT_MD : 0), tags, 0, rec)) return false;
                        const RecMeasures m{h[0], h[3], h[2], rec.oc() ? h[5] : h[4], h[6], 0};
                        std::printf("%lld%c", (long long)record_bound(rec, m, e), (md && cs == 2 && de && eqx && oc) ? '\n' : ' ');
                    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2 && argc != 3) return 2;
    FILE *fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<int64_t> all;
    int64_t h[7];
    while (std::fread(h, sizeof h, 1, fh) == 1) all.insert(all.end(), h, h + 7);
    std::fclose(fh);
    for (size_t p = 0; p < all.size(); p += 7) {
        const int64_t name = all[p], rl = all[p + 1], sl = all[p + 2], l_seq = all[p + 3], aux = all[p + 4], aux_oc = all[p + 5], words = all[p + 6];
        if (name < 1 || rl < 0 || sl < 0 || l_seq < sl || aux < 0 || aux_oc < 0 || aux_oc > aux || words < 0) return 2;
        if (!print_sums(&all[p], own_final_extent(rl, sl))) return 2;
    }
    if (argc == 2) return 0;
    if (!(fh = std::fopen(argv[2], "rb"))) return 2;
    std::vector<uint8_t> fin;
    for (size_t p = 0; p < all.size(); p += 7) {
        int64_t n = -1;
        if (std::fread(&n, sizeof n, 1, fh) != 1 || n < 0 || n > (1 << 24)) return 2;
        fin.resize((size_t)n * 4 + 4);
        if (n && std::fread(fin.data(), 4, (size_t)n, fh) != (size_t)n) return 2;
        if (!print_sums(&all[p], words_final_extent(fin.data(), n))) return 2;
    }
    std::fclose(fh);
    return 0;
}
