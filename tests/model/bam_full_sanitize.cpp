// tests/model/bam_full_sanitize.cpp -- TEST INFRASTRUCTURE.
// A stand-alone program for tests/test_bam_full.py, built with g++ -fsanitize=address,undefined: the records of the file
// named on the command line (block_size-framed, one after the other, no header) go through the host side of the FULL
// records -- the aux filter, the staging function in all three forms and bam_record_full_into -- each record in a heap
// block of exactly its size and every output in a block of exactly the size the sizing call announced, so that a byte
// read or written outside either is the sanitizer's to report.  Exit code 0: all records through; 2: bad input.
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../npore_amd/csrc/bam_reader.hpp"
#include "../../npore_amd/csrc/staged_head.hpp"

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
    long long records = 0, kept = 0;
    for (size_t p = 0, nx = 0; p < all.size(); p = nx) {
        if (frame_record(all.data(), all.size(), p, nx) != Frame::WHOLE) return 2;
        std::unique_ptr<uint8_t[]> rec(new uint8_t[nx - p]);                 // exactly the record
        std::memcpy(rec.get(), all.data() + p, nx - p);
        if (!record_is_sound(rec.get())) return 2;
        const RecView r = rec_view(rec.get());
        // the filter: count, then fill a block of that size
        const int64_t na = filter_aux(r.aux(), r.end(), nullptr);
        std::unique_ptr<uint8_t[]> aux(new uint8_t[(size_t)na]);
        if (filter_aux(r.aux(), r.end(), aux.get()) != na) return 1;
        kept += na;
        // the staging function, every form
        for (int form : {STAGE_HEAD, STAGE_QUALS, STAGE_FULL}) {
            const int64_t ns = staged_head_bytes(rec.get(), form);
            std::unique_ptr<uint8_t[]> st(new uint8_t[(size_t)ns]);
            stage_record_head(rec.get(), form, st.get());
            const uint8_t *cg, *sq;
            int nc;
            staged_cigar(st.get() + 4, cg, nc, sq);
            if (form == STAGE_FULL && (sq + ((int64_t)r.l_seq() + 1) / 2 + r.l_seq() + na != st.get() + ns ||
                                       std::memcmp(st.get() + ns - na, aux.get(), (size_t)na) != 0))
                return 1;
        }
        // the record: the read's code arrays all N, a final CIGAR of its own lengths
        const RecCigar cg = rec_cigar(r);
        int64_t lead, trail;
        rec_clips(cg, lead, trail);
        const int64_t rl = rec_ref_len(cg), sl = std::max<int64_t>(0, (int64_t)r.l_seq() - lead - trail);
        std::vector<uint8_t> refs((size_t)rl, 0), seqs((size_t)sl, 0);
        const std::string fin = std::to_string(sl) + "I" + std::to_string(rl) + "D";
        const int64_t nm = nm_of_text(fin.data(), (int64_t)fin.size(), refs.data(), rl, seqs.data(), sl);
        if (nm != rl + sl) return 1;
        const int64_t size = bam_record_full_into(r, fin.data(), (int64_t)fin.size(), 0, nm, nullptr);
        if (size <= 0) return 1;
        std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)size]);
        if (bam_record_full_into(r, fin.data(), (int64_t)fin.size(), 0, nm, out.get()) != size) return 1;
        if (rdi32(out.get()) != size - 4) return 1;
        records++;
    }
    std::printf("%lld records, %lld kept aux bytes\n", records, kept);
    return 0;
}
