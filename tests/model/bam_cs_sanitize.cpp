// tests/model/bam_cs_sanitize.cpp -- TEST INFRASTRUCTURE.
// A stand-alone program for tests/test_bam_cs.py, built with g++ -fsanitize=address,undefined: the cases of the file named on
// the command line -- per case three int64 (CIGAR words n, reference codes rl, query codes sl), then the 4 * n word bytes, the
// rl and the sl code bytes -- go through csrc/cs_rec.hpp's sequential twin in both forms: cs_size_of_words, then cs_into_words
// with cap exactly that size, once into a heap block of exactly that size (a byte written behind it is the sanitizer's to
// report) and once into a block with eight guard bytes behind the text (which must stay as they were); every input lies in a
// block of exactly its size.  Prints per case one line: the short text, the long text, E, X, G and de's bits, tab-separated.
// Exit code 0: all through; 1: size and text disagree or a guard byte changed; 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../npore_amd/csrc/cs_rec.hpp"

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
        int64_t h[3];
        if (p + 24 > all.size()) return 2;
        std::memcpy(h, all.data() + p, 24);
        p += 24;
        const int64_t n = h[0], rl = h[1], sl = h[2];
        if (n < 0 || rl < 0 || sl < 0 || p + (size_t)(4 * n + rl + sl) > all.size()) return 2;
        std::unique_ptr<uint8_t[]> w(new uint8_t[(size_t)(4 * n)]), ref(new uint8_t[(size_t)rl]), seq(new uint8_t[(size_t)sl]);
        std::memcpy(w.get(), all.data() + p, (size_t)(4 * n));
        std::memcpy(ref.get(), all.data() + p + 4 * n, (size_t)rl);
        std::memcpy(seq.get(), all.data() + p + 4 * n + rl, (size_t)sl);
        p += (size_t)(4 * n + rl + sl);
        CsCounts c[2];
        for (int lng = 0; lng < 2; lng++) {
            const int64_t size = cs_size_of_words(w.get(), n, ref.get(), rl, seq.get(), sl, lng != 0, &c[lng]);
            if (size < 0) return 1;
            std::unique_ptr<uint8_t[]> exact(new uint8_t[(size_t)size]), guarded(new uint8_t[(size_t)size + 8]);
            std::memset(exact.get(), 0, (size_t)size);
            std::memset(guarded.get(), 0, (size_t)size);
            std::memset(guarded.get() + size, 0xA5, 8);
            if (cs_into_words(w.get(), n, ref.get(), rl, seq.get(), sl, lng != 0, exact.get(), size) != size) return 1;
            if (cs_into_words(w.get(), n, ref.get(), rl, seq.get(), sl, lng != 0, guarded.get(), size) != size) return 1;
            for (int64_t q = 0; q < size; q++)
                if (exact[q] == 0 || exact[q] != guarded[q]) return 1;       // every byte of the announced size was written
            for (int q = 0; q < 8; q++)
                if (guarded[size + q] != 0xA5) return 1;
            std::fwrite(exact.get(), 1, (size_t)size, stdout);
            std::fputc('\t', stdout);
        }
        if (c[0].e != c[1].e || c[0].x != c[1].x || c[0].g != c[1].g) return 1;
        const float de = de_of_counts(c[0].e, c[0].x, c[0].g);
        uint32_t bits;
        std::memcpy(&bits, &de, 4);
        std::printf("%u\t%u\t%u\t%u\n", c[0].e, c[0].x, c[0].g, bits);
    }
    return 0;
}
