// asan_inflate_wave.cpp -- the host twin of the device DEFLATE decoder (npore_amd/csrc/inflate_wave.hpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer, on the whole corpus of tests/inflate_device_cases.py, before any of it
// goes to a GPU.  A stand-alone program: host code only, no HIP, no Python in the process (scripts/asan_inflate_wave.sh
// writes the corpus file, builds this with -fsanitize=address,undefined and runs it).
//
// Corpus file: per launch  "IWL1" | n | in_bytes | out_bytes (int64 each) | in_off[n] in_len[n] out_off[n] out_len[n] (int64) |
// expect[n] (int32: 1 must inflate, 0 must be refused, -1 either) | the input buffer.
// Every launch runs twice: as placed, in heap buffers of exactly in_bytes / out_bytes (the bytes between the streams'
// outputs must stay 0xA5), and stream by stream in heap blocks of exactly in_len / out_len bytes, so that one byte read
// or written outside a stream's own ranges is a sanitizer report.  Both must give the same status and bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../npore_amd/csrc/inflate_wave.hpp"

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    long launches = 0, streams = 0, inflated = 0, failures = 0;
    char magic[4];
    while (std::fread(magic, 1, 4, f) == 4) {
        int64_t head[3];
        if (std::memcmp(magic, "IWL1", 4) != 0 || !read_exact(f, head, sizeof head)) { std::fprintf(stderr, "bad corpus file\n"); return 2; }
        const int64_t n = head[0], in_bytes = head[1], out_bytes = head[2];
        std::vector<int64_t> meta((size_t)n * 4);
        std::vector<int32_t> expect((size_t)n), st_placed((size_t)n), st_alone((size_t)n);
        uint8_t *in = static_cast<uint8_t *>(std::malloc((size_t)in_bytes ? (size_t)in_bytes : 1));
        uint8_t *out = static_cast<uint8_t *>(std::malloc((size_t)out_bytes ? (size_t)out_bytes : 1));
        if (!in || !out || !read_exact(f, meta.data(), (size_t)n * 32) || !read_exact(f, expect.data(), (size_t)n * 4) || !read_exact(f, in, (size_t)in_bytes)) {
            std::fprintf(stderr, "bad corpus file\n");
            return 2;
        }
        const int64_t *in_off = meta.data(), *in_len = in_off + n, *out_off = in_len + n, *out_len = out_off + n;
        std::memset(out, 0xA5, (size_t)out_bytes);
        npore::inflate_wave_host(in, in_off, in_len, out, out_off, out_len, n, st_placed.data());
        std::vector<uint8_t> own((size_t)out_bytes, 0);
        for (int64_t k = 0; k < n; k++) std::memset(own.data() + out_off[k], 1, (size_t)out_len[k]);
        for (int64_t i = 0; i < out_bytes; i++)
            if (!own[(size_t)i] && out[i] != 0xA5) { std::fprintf(stderr, "launch %ld: byte %lld outside every stream was written\n", launches, (long long)i); failures++; break; }
        for (int64_t k = 0; k < n; k++) {
            uint8_t *a = static_cast<uint8_t *>(std::malloc((size_t)in_len[k] ? (size_t)in_len[k] : 1));
            uint8_t *b = static_cast<uint8_t *>(std::malloc((size_t)out_len[k] ? (size_t)out_len[k] : 1));
            std::memcpy(a, in + in_off[k], (size_t)in_len[k]);
            const int64_t zero = 0;
            npore::inflate_wave_host(a, &zero, &in_len[k], b, &zero, &out_len[k], 1, &st_alone[(size_t)k]);
            const int s = st_alone[(size_t)k];
            if (s != st_placed[(size_t)k] || (s == 1 && std::memcmp(b, out + out_off[k], (size_t)out_len[k]) != 0) || (expect[(size_t)k] >= 0 && s != expect[(size_t)k])) {
                std::fprintf(stderr, "launch %ld stream %lld: status alone %d, placed %d, expected %d\n", launches, (long long)k, s, st_placed[(size_t)k], expect[(size_t)k]);
                failures++;
            }
            streams++;
            inflated += s == 1;
            std::free(a);
            std::free(b);
        }
        std::free(in);
        std::free(out);
        launches++;
    }
    std::fclose(f);
    std::printf("%ld launches, %ld streams, %ld inflated, %ld failures\n", launches, streams, inflated, failures);
    return failures ? 1 : 0;
}
