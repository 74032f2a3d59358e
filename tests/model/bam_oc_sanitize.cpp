// tests/model/bam_oc_sanitize.cpp -- TEST INFRASTRUCTURE.
// A stand-alone program for tests/test_bam_oc.py, built with g++ -fsanitize=address,undefined: the cases of the file named on the
// command line -- per case four int64 (input words nc, clip range ci and cj, final words nf), then the 4 * nc and the 4 * nf word
// bytes -- go through csrc/oc_rec.hpp's sequential code: oc_changed_words, then oc_walk_words with the counting sink and with the
// storing sink told exactly that count, once into a heap block of exactly that many bytes at an ODD address (a byte written behind
// it is the sanitizer's to report; the tag has any alignment) and once into a block with eight guard bytes behind the text (which
// must stay as they were); then oc_tag_of_words behind a string that holds something already.  Every input lies in a block of
// exactly its size.  Prints per case one line: `0` or `1` (changed), a blank, the OC text.  Exit code 0: all through; 1: count and
// stored length or bytes disagree or a guard byte changed; 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../npore_amd/csrc/oc_rec.hpp"

using namespace npore;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<uint8_t> all;
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, fh)) > 0;) all.insert(all.end(), buf, buf + n);
    std::fclose(fh);
    for (size_t p = 0; p < all.size();) {
        int64_t h[4];
        if (p + 32 > all.size()) return 2;
        std::memcpy(h, all.data() + p, 32);
        p += 32;
        const int64_t nc = h[0], ci = h[1], cj = h[2], nf = h[3];
        if (nc < 0 || nf < 0 || ci < 0 || cj < ci || cj > nc || p + (size_t)(4 * nc + 4 * nf) > all.size()) return 2;
        std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)(4 * nc)]), fin(new uint8_t[(size_t)(4 * nf)]);
        std::memcpy(in.get(), all.data() + p, (size_t)(4 * nc));
        std::memcpy(fin.get(), all.data() + p + 4 * nc, (size_t)(4 * nf));
        p += (size_t)(4 * nc + 4 * nf);
        const bool changed = oc_changed_words(in.get(), ci, cj, fin.get(), nf);
        const int64_t size = oc_walk_words(in.get(), nc, OcCount{});
        if (size < 0) return 1;
        std::unique_ptr<uint8_t[]> odd(new uint8_t[(size_t)size + 1]), guarded(new uint8_t[(size_t)size + 8]);
        uint8_t *exact = odd.get() + 1;                          // ends where the allocation ends
        std::memset(exact, 0, (size_t)size);
        std::memset(guarded.get(), 0, (size_t)size);
        std::memset(guarded.get() + size, 0xA5, 8);
        if (oc_walk_words(in.get(), nc, OcStore{exact, size}) != size) return 1;
        if (oc_walk_words(in.get(), nc, OcStore{guarded.get(), size}) != size) return 1;
        std::string tag = "xy";
        oc_tag_of_words(in.get(), nc, tag);
        if ((int64_t)tag.size() != 2 + 4 + size || tag.compare(0, 5, "xyOCZ") != 0 || tag.back() != '\0') return 1;
        if (std::memcmp(tag.data() + 5, exact, (size_t)size) != 0 || std::memcmp(guarded.get(), exact, (size_t)size) != 0) return 1;
        for (int q = 0; q < 8; q++)
            if (guarded[size + q] != 0xA5) return 1;
        for (int64_t c = 0; c < size; c++)
            if (exact[c] == 0) return 1;                         // every byte of the announced length was written
        std::printf("%d ", changed ? 1 : 0);
        std::fwrite(exact, 1, (size_t)size, stdout);
        std::fputc('\n', stdout);
    }
    return 0;
}
