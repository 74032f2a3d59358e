// tests/model/bam_eqx_sanitize.cpp -- TEST INFRASTRUCTURE.
// A stand-alone program for tests/test_bam_eqx.py, built with g++ -fsanitize=address,undefined: the cases of the file named on
// the command line -- per case three int64 (CIGAR words n, reference codes rl, query codes sl), then the 4 * n word bytes, the
// rl and the sl code bytes -- go through csrc/eqx_rec.hpp's sequential twin: eqx_walk_words with the counting sink, then with
// the storing sink told exactly that count, once into a heap block of exactly 4 * count bytes at an ODD address inside its
// allocation's last bytes (a byte written behind it is the sanitizer's to report; the CIGAR field of a record has any
// alignment) and once into a block with eight guard bytes behind the words (which must stay as they were); then eqx_of_words,
// which must give the same words; every input lies in a block of exactly its size.  Prints per case one line: the =/X form as
// CIGAR text.  Exit code 0: all through; 1: count and words disagree or a guard byte changed; 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../npore_amd/csrc/eqx_rec.hpp"

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
        const int64_t ops = eqx_walk_words(w.get(), n, ref.get(), rl, seq.get(), sl, EqxCount{});
        if (ops < 0) return 1;
        const size_t bytes = (size_t)ops * 4;
        std::unique_ptr<uint8_t[]> odd(new uint8_t[bytes + 1]), guarded(new uint8_t[bytes + 8]);
        uint8_t *exact = odd.get() + 1;                          // ends where the allocation ends
        std::memset(exact, 0, bytes);
        std::memset(guarded.get(), 0, bytes);
        std::memset(guarded.get() + bytes, 0xA5, 8);
        if (eqx_walk_words(w.get(), n, ref.get(), rl, seq.get(), sl, EqxStore{exact, ops}) != ops) return 1;
        if (eqx_walk_words(w.get(), n, ref.get(), rl, seq.get(), sl, EqxStore{guarded.get(), ops}) != ops) return 1;
        const std::vector<uint8_t> twin = eqx_of_words(w.get(), n, ref.get(), rl, seq.get(), sl);
        if (twin.size() != bytes + 4 || std::memcmp(twin.data(), exact, bytes) != 0 || std::memcmp(guarded.get(), exact, bytes) != 0) return 1;
        for (int q = 0; q < 8; q++)
            if (guarded[bytes + q] != 0xA5) return 1;
        for (int64_t c = 0; c < ops; c++) {
            uint32_t v;
            std::memcpy(&v, exact + 4 * c, 4);
            if ((v >> 4) == 0 || (v & 15u) > 8u) return 1;       // every word of the announced count was written
            std::printf("%u%c", v >> 4, "MIDNSHP=X"[v & 15u]);
        }
        std::fputc('\n', stdout);
    }
    return 0;
}
