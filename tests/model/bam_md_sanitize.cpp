// tests/model/bam_md_sanitize.cpp -- TEST INFRASTRUCTURE.
// A stand-alone program for tests/test_bam_md.py, built with g++ -fsanitize=address,undefined: the cases of the file named on
// the command line -- per case three int64 (CIGAR words n, reference codes rl, query codes sl), then the 4 * n word bytes, the
// rl and the sl code bytes -- go through csrc/md_rec.hpp's sequential twin: md_size_of_words, then md_into_words into a heap
// block of exactly that size, every input in a block of exactly its size, so that a byte read or written outside any of them
// is the sanitizer's to report.  Prints one MD text per line.  Exit code 0: all through; 1: size and text disagree; 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../npore_amd/csrc/md_rec.hpp"

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
        const int64_t size = md_size_of_words(w.get(), n, ref.get(), rl, seq.get(), sl);
        if (size < 1) return 1;
        std::unique_ptr<uint8_t[]> text(new uint8_t[(size_t)size]);
        std::memset(text.get(), 0, (size_t)size);
        if (md_into_words(w.get(), n, ref.get(), rl, seq.get(), sl, text.get(), size) != size) return 1;
        for (int64_t q = 0; q < size; q++)
            if (text[q] == 0) return 1;                      // every byte of the announced size was written
        std::fwrite(text.get(), 1, (size_t)size, stdout);
        std::fputc('\n', stdout);
    }
    return 0;
}
