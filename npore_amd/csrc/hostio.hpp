// hostio.hpp -- BAM ingest and SAM emit around the batched align(), host side, native.
//
// Counterpart of the reference's compiled I/O layer for this path: pysam's fetch + the per-read
// accessors used by get_read_data (reference src/bam.pyx:18-47), the glue of realign_read
// (src/bam.pyx:51-84: expand_cigar / bases_to_int before align(), standardisation and the SAM
// line after it) -- for a whole batch of reads on all host cores instead of one read per
// Python call.  npore_amd/bam.py keeps a pure-Python restatement of the same logic; the tests
// compare the two record by record.
//
// BAM = BGZF (independent deflate blocks of <= 64 KiB, each announcing its compressed size in a
// gzip extra field and its inflated size in its trailer) around a simple binary record stream,
// so the blocks are located with one pass over the file and inflated in parallel.
//
// This header holds the pieces (BGZF, FASTA, record accessors, the handles); bam_reader.hpp the readers built from
// them.  Neither includes a HIP header: both compile for a CPU alone (tests/model/bam_walk.cpp does).
#pragma once
#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include "crc32.hpp"
#include "inflate.hpp"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/npore_amd.h"
#include "glue.hpp"
#include "staged_head.hpp"
#include "nm_rec.hpp"

namespace npore {

// default worker count: these loops are memory-bound byte shuffles, more than 64 threads only add start-up cost
// CPUs this process may actually use: the affinity mask, cut down by a cgroup CPU quota if there is one (a container
// on a 256-CPU host with a 16-CPU quota sees 256 CPUs; 64 threads there only thrash and grow 64 malloc arenas)
inline int usable_cpus()
{
    static const int n = [] {
        int cpus = (int)std::max(1u, std::thread::hardware_concurrency());
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) cpus = std::max(1, CPU_COUNT(&set));
        if (FILE *fh = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {                    // cgroup v2: "<quota|max> <period>"
            char q[32] = {0};
            long long period = 0;
            if (std::fscanf(fh, "%31s %lld", q, &period) == 2 && period > 0 && std::strcmp(q, "max") != 0)
                cpus = std::min<long long>(cpus, std::max<long long>(1, (std::atoll(q) + period - 1) / period));
            std::fclose(fh);
        } else if (FILE *f1 = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
            long long quota = -1, period = 0;
            if (std::fscanf(f1, "%lld", &quota) != 1) quota = -1;
            std::fclose(f1);
            if (FILE *f2 = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (std::fscanf(f2, "%lld", &period) != 1) period = 0;
                std::fclose(f2);
            }
            if (quota > 0 && period > 0) cpus = std::min<long long>(cpus, std::max<long long>(1, (quota + period - 1) / period));
        }
        return cpus;
    }();
    return n;
}
inline int host_threads(int threads)
{
    return threads > 0 ? threads : std::min(64, usable_cpus());
}

// the calling thread's last failure (npore_last_error); fail() notes it and hands the code back
inline thread_local std::string g_err;
inline int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

// uninitialised byte buffer (a std::vector would zero hundreds of megabytes per batch)
// NPORE_ALLOC_TRACE=1: one line on stderr per device / page-locked allocation (what a cold run pays once)
inline bool alloc_trace_on() { static const bool on = std::getenv("NPORE_ALLOC_TRACE") != nullptr; return on; }
struct AllocTrace {
    const char *what;
    size_t bytes;
    std::chrono::steady_clock::time_point t0;
    AllocTrace(const char *w, size_t n) : what(w), bytes(n) { if (alloc_trace_on()) t0 = std::chrono::steady_clock::now(); }
    ~AllocTrace()
    {
        if (!alloc_trace_on()) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::fprintf(stderr, "alloc %-14s %12zu bytes %8.2f ms\n", what, bytes, ms);
    }
};

struct RawBuf {
    char *p = nullptr;
    size_t cap = 0;
    RawBuf() = default;
    RawBuf(const RawBuf &) = delete;
    RawBuf &operator=(const RawBuf &) = delete;
    ~RawBuf() { release(); }
    void release()
    {
        std::free(p);
        p = nullptr;
        cap = 0;
    }
    bool ensure(size_t n)
    {
        if (n <= cap) return true;
        release();
        n += n / 4;            // head-room: batches of a run differ a little in size
        p = alloc(n);
        cap = p ? n : 0;
        return p != nullptr;
    }
    static char *alloc(size_t n)
    {
        char *q = static_cast<char *>(std::malloc(n));
        // a large buffer is touched for the first time by all threads at once (the FASTA's bases, an inflated window,
        // a batch's SAM text): with 2 MB pages that is one page fault per 2 MB instead of 512 (where the kernel
        // offers transparent huge pages on request; a no-op elsewhere)
        if (q && n >= (size_t)32 << 20 && std::getenv("NPORE_NO_THP") == nullptr) {
            const uintptr_t a = ((uintptr_t)q + ((size_t)2 << 20) - 1) & ~(uintptr_t)(((size_t)2 << 20) - 1);
            const uintptr_t e = ((uintptr_t)q + n) & ~(uintptr_t)(((size_t)2 << 20) - 1);
            if (e > a) (void)::madvise(reinterpret_cast<void *>(a), e - a, MADV_HUGEPAGE);
        }
        return q;
    }
};

// Write the cache lines of [p, p + n) back to memory.  A page-locked buffer that host threads have just filled is
// still spread over the caches of the cores that wrote it, and the DMA engine then reads it at a fraction of the
// PCIe rate (measured: 3-5 GB/s, against 50 GB/s for the same buffer once it has aged out of the caches); with the
// lines written back first the upload runs at the link's rate.  clwb keeps the (now clean) line for the host's own
// later reads; clflushopt / clflush where the CPU has no clwb.
#if defined(__x86_64__)
#include <cpuid.h>
inline int cache_writeback_kind()
{
    static const int kind = [] {
        unsigned a = 0, b = 0, c = 0, d = 0;
        if (!__get_cpuid_count(7, 0, &a, &b, &c, &d)) return 0;
        return (b & (1u << 24)) ? 2 : (b & (1u << 23)) ? 1 : 0;      // CLWB, CLFLUSHOPT
    }();
    return kind;
}
inline void cache_writeback(const void *p, size_t n)
{
    if (!n) return;
    const int kind = cache_writeback_kind();
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)63, a1 = reinterpret_cast<uintptr_t>(p) + n;
    for (uintptr_t a = a0; a < a1; a += 64) {
        if (kind == 2) asm volatile(".byte 0x66, 0x0f, 0xae, 0x30" ::"a"(a) : "memory");        // clwb (%rax)
        else if (kind == 1) asm volatile(".byte 0x66, 0x0f, 0xae, 0x38" ::"a"(a) : "memory");   // clflushopt (%rax)
        else asm volatile("clflush (%0)" ::"r"(a) : "memory");
    }
    asm volatile("sfence" ::: "memory");
}
#else
inline void cache_writeback(const void *, size_t) {}
#endif

template <class F>
inline void parallel_for(int64_t n, int threads, F &&body)   // body(i) for i in [0, n), dynamic
{
    const int nt = (int)std::min<int64_t>(host_threads(threads), n);
    std::atomic<int64_t> next{0};
    // an exception of a body (an allocation that fails) must not leave its thread: the first one is kept, the other
    // workers stop taking indices, and the caller sees it after the join (the C ABI's entry points catch it there)
    std::exception_ptr failed;
    std::atomic<bool> stop{false};
    std::mutex failed_m;
    auto work = [&] {
        try {
            for (;;) {
                const int64_t i = next.fetch_add(1);
                if (i >= n || stop.load(std::memory_order_relaxed)) break;
                body(i);
            }
        } catch (...) {
            std::lock_guard<std::mutex> lk(failed_m);
            if (!failed) failed = std::current_exception();
            stop.store(true);
        }
    };
    if (nt <= 1) { work(); if (failed) std::rethrow_exception(failed); return; }
    std::vector<std::thread> pool;
    try {
        for (int t = 0; t < nt; t++) pool.emplace_back(work);
    } catch (...) {                                     // (no more threads to be had: the ones started do the work)
        if (pool.empty()) work();
    }
    for (auto &t : pool) t.join();
    if (failed) std::rethrow_exception(failed);
}

// a whole file, read-only: mapped (pages come in as the worker threads touch them, nothing is copied or zeroed)
struct MappedFile {
    const uint8_t *p = nullptr;
    size_t n = 0;
    bool ok = false;
    MappedFile() = default;
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
    ~MappedFile() { if (p && n) ::munmap(const_cast<uint8_t *>(p), n); }
    bool open(const char *path)
    {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { ::close(fd); return false; }
        n = (size_t)st.st_size;
        if (n) {
            void *q = ::mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
            if (q == MAP_FAILED) { ::close(fd); n = 0; return false; }
            p = static_cast<const uint8_t *>(q);
        }
        ::close(fd);
        return ok = true;
    }
};

inline uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline int32_t rdi32(const uint8_t *p) { return (int32_t)rd32(p); }

// Inflate a BGZF file.  Falls back to member-by-member gzip decoding if a member lacks the BC field.
struct ByteSpan {
    const uint8_t *p;
    size_t n;
    size_t size() const { return n; }
    const uint8_t *data() const { return p; }
    const uint8_t &operator[](size_t i) const { return p[i]; }
};

// deflate payload in the file; its place in the stream; where the member itself (its gzip header) begins in the file --
// the compressed half of a virtual offset
struct BgzfBlock { uint64_t in_off, in_len, out_off, out_len, mem_off; };

// header of the BGZF member at p[0 .. avail): payload offset and member size; false = not the header of a BGZF member
// (need = bytes wanted, when more input could help; 0 when none can)
inline bool bgzf_header(const uint8_t *p, size_t avail, size_t &pay_off, size_t &bsize, size_t &need)
{
    need = 18;
    if (avail < 18) return false;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) { need = 0; return false; }
    const size_t xlen = rd16(p + 10), xend = 12 + xlen;
    need = xend;
    if (xend > avail) return false;
    bsize = 0;
    for (size_t q = 12; q + 4 <= xend;) {
        const size_t slen = rd16(p + q + 2);
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= xend) bsize = (size_t)rd16(p + q + 4) + 1;
        q += 4 + slen;
    }
    if (!bsize || bsize < xlen + 20) { need = 0; return false; }
    pay_off = xend;
    return true;
}

// the whole member at p[0 .. avail): payload offset / length, inflated length, member size; false = not a complete BGZF
// member (need as above)
inline bool bgzf_member(const uint8_t *p, size_t avail, size_t &pay_off, size_t &pay_len, size_t &isize, size_t &bsize, size_t &need)
{
    if (!bgzf_header(p, avail, pay_off, bsize, need)) return false;
    need = bsize;
    if (bsize > avail) return false;
    pay_len = bsize - pay_off - 8;
    isize = rd32(p + bsize - 4);
    return true;
}

inline bool inflate_block(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, int force = 0)
{
    if (!out_len) return true;
    // force: 1 = this library's decoder only, 2 = zlib only (tests); 0 = the decoder, zlib for what it declines
    if (force != 2 && inflate_raw_fast(in, in_len, out, out_len)) return true;
    if (force == 1) return false;
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<Bytef *>(in);
    zs.avail_in = (uInt)in_len;
    zs.next_out = out;
    zs.avail_out = (uInt)out_len;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == out_len;
    inflateEnd(&zs);
    return ok;
}

// Whether the BGZF readers compare every member's CRC-32 with the one in its trailer (htslib does: the reference's reader
// raises on a damaged member whose bytes still inflate).  On unless NPORE_BGZF_CRC=0.
inline bool bgzf_check_crc()
{
    static const bool on = [] { const char *e = std::getenv("NPORE_BGZF_CRC"); return !(e && e[0] == '0'); }();
    return on;
}

// several blocks by one thread, side by side (inflate.hpp: as many dependent chains in one loop); zlib for what the decoder
// declines.  Returns the number of blocks that did not inflate.  crc: every job's payload is followed by its member's
// trailer (CRC-32 of the inflated bytes, little-endian), and a block whose bytes do not have it counts as not inflated.
inline int inflate_blocks(const FastInflate::Job *jobs, int n, int force = 0, bool crc = false)
{
    int bad = 0;
    auto crc_ok = [&](int k) {
        return !crc || crc32_fast(0u, jobs[k].out, jobs[k].out_len) == rd32(jobs[k].in + jobs[k].in_len);
    };
    if (force == 2) {
        for (int k = 0; k < n; k++) bad += !(inflate_block(jobs[k].in, jobs[k].in_len, jobs[k].out, jobs[k].out_len, 2) && crc_ok(k));
        return bad;
    }
    bool ok_small[64];
    std::vector<char> ok_big;
    bool *ok = ok_small;
    if (n > 64) { ok_big.resize((size_t)n); ok = reinterpret_cast<bool *>(ok_big.data()); }
    inflate_raw_fast_many(jobs, n, ok);
    for (int k = 0; k < n; k++) {
        if (!ok[k] && (force == 1 || !inflate_block(jobs[k].in, jobs[k].in_len, jobs[k].out, jobs[k].out_len, 2))) bad++;
        else if (!crc_ok(k)) bad++;
    }
    return bad;
}

inline bool bgzf_inflate(const ByteSpan &raw, int threads, RawBuf &out, size_t &out_size, std::string &err)
{
    typedef BgzfBlock Blk;
    std::vector<Blk> blocks;
    size_t p = 0, total = 0;
    bool is_bgzf = true;
    while (p + 18 <= raw.size()) {
        size_t po, pl, isz, bs, need;
        if (!bgzf_member(raw.data() + p, raw.size() - p, po, pl, isz, bs, need)) { is_bgzf = false; break; }
        blocks.push_back({p + po, pl, total, isz, p});
        total += isz;
        p += bs;
    }
    if (is_bgzf && p == raw.size()) {
        if (!out.ensure(total + 1)) { err = "out of memory"; return false; }
        out_size = total;
        std::atomic<int> bad{0};
        const int64_t per = 8;                                  // blocks per task
        parallel_for(((int64_t)blocks.size() + per - 1) / per, threads, [&](int64_t t) {
            FastInflate::Job jobs[8];
            int n = 0;
            uint8_t *const o = reinterpret_cast<uint8_t *>(out.p);
            for (size_t i = (size_t)(t * per); i < std::min(blocks.size(), (size_t)((t + 1) * per)); i++)
                jobs[n++] = {raw.data() + blocks[i].in_off, blocks[i].in_len, o + blocks[i].out_off, blocks[i].out_len};
            bad += inflate_blocks(jobs, n, 0, bgzf_check_crc());      // (the trailer follows the payload in the mapping)
        });
        if (bad) { err = "corrupt BGZF block"; return false; }
        return true;
    }
    // plain (multi-member) gzip
    std::vector<uint8_t> acc;
    p = 0;
    std::vector<uint8_t> chunk(1 << 20);
    while (p < raw.size()) {
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, 31) != Z_OK) { err = "zlib init failed"; return false; }
        zs.next_in = const_cast<Bytef *>(raw.data() + p);
        zs.avail_in = (uInt)std::min<size_t>(raw.size() - p, 0x7fffffffu);
        int rc;
        do {
            zs.next_out = chunk.data();
            zs.avail_out = (uInt)chunk.size();
            rc = inflate(&zs, Z_NO_FLUSH);
            if (rc != Z_OK && rc != Z_STREAM_END) { inflateEnd(&zs); err = "not a gzip/BGZF stream"; return false; }
            acc.insert(acc.end(), chunk.data(), chunk.data() + (chunk.size() - zs.avail_out));
        } while (rc != Z_STREAM_END);
        p += zs.total_in;
        inflateEnd(&zs);
        if (zs.total_in == 0) break;
    }
    if (!out.ensure(acc.size() + 1)) { err = "out of memory"; return false; }
    std::memcpy(out.p, acc.data(), acc.size());
    out_size = acc.size();
    return true;
}

// A file read with pread(): the streamed BAM mode never maps the file, so that what it has read does not stay in
// this process's resident set.
struct PreadFile {
    int fd = -1;
    uint64_t size = 0;
    PreadFile() = default;
    PreadFile(const PreadFile &) = delete;
    PreadFile &operator=(const PreadFile &) = delete;
    ~PreadFile() { if (fd >= 0) ::close(fd); }
    bool open(const char *path)
    {
        fd = ::open(path, O_RDONLY);
        struct stat st;
        if (fd < 0 || ::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return false;
        size = (uint64_t)st.st_size;
        return true;
    }
    bool read(uint64_t off, void *dst, size_t n) const
    {
        char *d = static_cast<char *>(dst);
        while (n) {
            const ssize_t k = ::pread(fd, d, n, (off_t)off);
            if (k <= 0) return false;
            d += k; off += (uint64_t)k; n -= (size_t)k;
        }
        return true;
    }
};

// block table of a BGZF file, read sequentially in 8 MB pieces; false = not BGZF throughout
inline bool bgzf_scan(const PreadFile &f, std::vector<BgzfBlock> &blocks, uint64_t &total)
{
    // From member header to member header: the last four bytes of one member (its inflated length) and the header of the
    // next lie side by side, so the table costs one read of a few dozen bytes per member -- not one pass over the file
    // (1.45 GB of page cache took 0.18 s of a 0.83 s run that way).
    total = 0;
    const size_t HEAD = 64;
    std::vector<uint8_t> buf(4 + HEAD);
    uint64_t fp = 0;                                            // the member whose header is at buf[4 ..)
    size_t have = (size_t)std::min<uint64_t>(HEAD, f.size);
    if (have && !f.read(0, buf.data() + 4, have)) return false;
    while (fp < f.size) {
        size_t po, bs, need;
        if (!bgzf_header(buf.data() + 4, have, po, bs, need)) {
            if (need <= have || fp + need > f.size) return false;          // not a BGZF member, or cut short
            buf.resize(4 + need);                                           // a longer extra field than we guessed
            if (!f.read(fp + have, buf.data() + 4 + have, need - have)) return false;
            have = need;
            if (!bgzf_header(buf.data() + 4, have, po, bs, need)) return false;
        }
        if (fp + bs > f.size) return false;                     // the file ends inside a member
        const uint64_t nx = fp + bs;
        have = (size_t)std::min<uint64_t>(HEAD, f.size - nx);
        if (buf.size() < 4 + HEAD) buf.resize(4 + HEAD);
        if (!f.read(nx - 4, buf.data(), 4 + have)) return false;
        const size_t isz = rd32(buf.data());
        blocks.push_back({fp + po, bs - po - 8, total, isz, fp});
        total += isz;
        fp = nx;
    }
    return true;
}

// inflate blocks [b0, b1) of the table back to back into dst (their out_off relative to blocks[b0].out_off)
inline bool bgzf_inflate_range(const PreadFile &f, const std::vector<BgzfBlock> &blocks, size_t b0, size_t b1, uint8_t *dst, int threads)
{
    if (b0 >= b1) return true;
    std::atomic<int> bad{0};
    const uint64_t o0 = blocks[b0].out_off;
    const int64_t per = 8;                                      // blocks per task
    // every task reads the compressed bytes of its own blocks (a few hundred KB, into a buffer its thread keeps): the
    // copy out of the page cache runs on all threads like the inflation, and no window-sized buffer is allocated and
    // faulted in per call.  (Rounds 3 - 4 read the whole range with one pread on the calling thread first: 40 MB per
    // 64 MB window of a BAM with real qualities, a serial 10 - 20 ms in front of every window.)
    parallel_for(((int64_t)(b1 - b0) + per - 1) / per, threads, [&](int64_t t) {
        static thread_local std::vector<uint8_t> comp;
        const size_t i0 = b0 + (size_t)t * per, i1 = std::min(b1, b0 + (size_t)(t + 1) * per);
        // (+ 8: the last block's trailer -- CRC-32, inflated length --; the table was made from whole members)
        const uint64_t in0 = blocks[i0].in_off, in1 = blocks[i1 - 1].in_off + blocks[i1 - 1].in_len + 8;
        if (comp.size() < (size_t)(in1 - in0) + 64) comp.resize((size_t)(in1 - in0) + 64);
        if (!f.read(in0, comp.data(), (size_t)(in1 - in0))) { bad += (int)(i1 - i0); return; }
        FastInflate::Job jobs[8];
        int n = 0;
        for (size_t i = i0; i < i1; i++)
            jobs[n++] = {comp.data() + (blocks[i].in_off - in0), blocks[i].in_len, dst + (blocks[i].out_off - o0), blocks[i].out_len};
        bad += inflate_blocks(jobs, n, 0, bgzf_check_crc());
    });
    return bad == 0;
}
// ... or by whoever the caller names (BamWindowSource's hook: the same arguments, the same result; what fail() was given on
// the calling thread says why not).  The HIP unit's DeviceInflater (inflate_kernels.hpp) is one; this file knows none.
using BgzfInflateFn = std::function<bool(const PreadFile &, const std::vector<BgzfBlock> &, size_t, size_t, uint8_t *, int)>;

// Virtual offsets of a .bai index's LINEAR index (SAM specification 5.2: per reference, for every 16 kb window the
// virtual file offset -- compressed offset of a BGZF block << 16 | offset inside the inflated block -- of the first
// alignment that overlaps the window), all references, ascending, without duplicates and zeros.  Each one is where a
// record starts: the cut points at which a coordinate-sorted BAM can be dealt to several readers without a pass over it.
inline bool bai_linear_offsets(const char *path, std::vector<uint64_t> &out, std::vector<uint8_t> *ref_has_reads = nullptr)
{
    MappedFile mf;
    if (!mf.open(path) || mf.n < 8 || std::memcmp(mf.p, "BAI\1", 4) != 0) return false;
    const uint8_t *p = mf.p;
    const size_t n = mf.n;
    size_t q = 4;
    // every count is bounded by the bytes that are left before anything is sized by it or looped over: a reference takes
    // eight bytes at least (n_bin, n_intv), a bin eight (its id, n_chunk), a chunk sixteen, a linear entry eight
    auto have = [&](size_t k) { return k <= n - q; };
    const int32_t n_ref = (int32_t)rd32(p + q); q += 4;
    if (n_ref < 0 || (size_t)n_ref > (n - q) / 8) return false;
    out.clear();
    std::vector<uint8_t> has((size_t)n_ref, 0);
    for (int32_t r = 0; r < n_ref; r++) {
        if (!have(4)) return false;
        const int32_t n_bin = (int32_t)rd32(p + q); q += 4;
        if (n_bin < 0 || (size_t)n_bin > (n - q) / 8) return false;
        if (n_bin > 0) has[(size_t)r] = 1;
        for (int32_t b = 0; b < n_bin; b++) {
            if (!have(8)) return false;
            const int32_t n_chunk = (int32_t)rd32(p + q + 4); q += 8;
            if (n_chunk < 0 || (size_t)n_chunk > (n - q) / 16) return false;
            q += (size_t)n_chunk * 16;
        }
        if (!have(4)) return false;
        const int32_t n_intv = (int32_t)rd32(p + q); q += 4;
        if (n_intv < 0 || (size_t)n_intv > (n - q) / 8) return false;
        for (int32_t k = 0; k < n_intv; k++) {
            const uint64_t v = (uint64_t)rd32(p + q) | ((uint64_t)rd32(p + q + 4) << 32);
            q += 8;
            if (v) {
                out.push_back(v);
                has[(size_t)r] = 1;
            }
        }
    }
    if (ref_has_reads) ref_has_reads->swap(has);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return true;
}

}  // namespace npore

namespace npore {
// The bytes of a batch of records: pointers into the resident stream, or (streamed handle) into `buf`, which holds
// the runs of consecutive BGZF blocks the batch's records lie in, inflated for this batch (bam_fetch).
struct RecFetch {
    RawBuf buf;
    std::vector<const uint8_t *> ptr;
};
// what the BAM writer's index bookkeeping needs of one written record (bam_reader.hpp BgzfStoredWriter)
struct BamRecMeta {
    int32_t ref, pos;
    int64_t span;                         // reference length
    int64_t bytes;                        // the record with its block_size word
};
// The record a run writes, from the setters through to the emit launch; the default: the reference's records.  Only
// rec_spec_of makes another, so a spec without `full` has everything else zero wherever it is read.
struct RecSpec {
    bool full = false;                    // NPORE_OUT_FULL: FULL records (bam_reader.hpp FULL RECORD) ...
    bool md = false;                      // ... NPORE_OUT_MD: with the MD tag behind NM
    int tags = 0;                         // ... the setters' word: NPORE_TAG_* (cs / de behind that, OC behind those) and NPORE_CIGAR_EQX
    uint32_t pass_mask = 0;               // ... records with one of these flag bits pass through (staged_head.hpp)
    int cs_de() const { return tags & (NPORE_TAG_CS | NPORE_TAG_CS_LONG | NPORE_TAG_DE); }      // the tags of the word (0: neither cs nor de)
    bool eqx() const { return (tags & NPORE_CIGAR_EQX) != 0; }                                  // its other bit: the final CIGAR in =/X form
    bool oc() const { return (tags & NPORE_TAG_OC) != 0; }                                      // ... and OC:Z on the reads that changed (oc_rec.hpp)
};
// THE rules of the output options: defined bits only, CS_LONG beside CS, md / tags / pass on FULL records, FULL records in BAM
inline bool rec_spec_of(int format, int flags, int tags, int pass, RecSpec &out)
{
    const int all_flags = NPORE_OUT_EOF | NPORE_OUT_PART | NPORE_OUT_DEFLATE | NPORE_OUT_MATCH | NPORE_OUT_FULL | NPORE_OUT_MD;
    const bool full = (flags & NPORE_OUT_FULL) != 0;
    if ((flags & ~all_flags) || (tags & ~(NPORE_TAG_CS | NPORE_TAG_CS_LONG | NPORE_TAG_DE | NPORE_CIGAR_EQX | NPORE_TAG_OC)) || (pass & ~(int)PASS_FLAGS) ||
        ((tags & NPORE_TAG_CS_LONG) && !(tags & NPORE_TAG_CS)) || (!full && ((flags & NPORE_OUT_MD) || tags || pass)) ||
        (full && format != NPORE_OUT_BAM))
        return false;
    out = RecSpec{full, (flags & NPORE_OUT_MD) != 0, tags, (uint32_t)pass};
    return true;
}
}  // namespace npore

// ---- handles ---------------------------------------------------------------------------------
struct npore_bam {
    std::unique_ptr<npore::MappedFile> raw_map;   // the file itself when it already is an inflated BAM stream
    npore::RawBuf data_buf;               // inflated stream
    const uint8_t *data = nullptr;
    size_t data_size = 0;
    std::string text;                     // header text
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lens;
    std::vector<uint8_t> ref_has_reads;
    // ONE-PASS handle: the .bai that ref_has_reads was taken from ("" = from no index).  An index is a CLAIM about the
    // file: a record the one-pass walk meets on a contig that this one declared empty ends the run (BamRecordWalker)
    std::string has_reads_index;
    uint64_t first_record = 0;            // where the header ends in the inflated stream (0: not known)
    // STREAMED mode (large files): the inflated stream is never held as a whole.  The handle keeps the BGZF block
    // table and, per record, what selection needs (below); the bytes of a batch of records are inflated on demand
    // from the blocks that hold them (RecFetch).  data == nullptr then.
    bool streamed = false;
    std::unique_ptr<npore::PreadFile> file;
    std::vector<npore::BgzfBlock> blocks;
    std::vector<int32_t> m_ref, m_pos, m_span;     // per record: reference id, position, reference span
    std::vector<uint16_t> m_flag;
    std::vector<int64_t> rec_off;         // offset of each record's block_size field (in the inflated stream)
    std::vector<std::vector<int64_t>> by_ref;   // record indices per reference id, file order
    std::vector<uint8_t> ref_sorted;      // ... which is ascending in position (regions then need no full scan)
    std::vector<int64_t> ref_max_len;     // longest reference span of a record on that reference
    npore::RecFetch api_fetch;            // records of the last npore_bam_format_sam call (the const entry points keep theirs local)
    npore::RawBuf sam;                    // text of the last formatted batch
    npore::RawBuf w_finals;               // final CIGARs of the last batch (work buffer, reused)
    // ONE-PASS handle, several processes (npore_bam_set_share): the contiguous stretch of the record stream this process
    // walks, as offsets into the inflated stream; share_begin is where a record starts (a virtual offset of the file's
    // .bai linear index), share_end where the next process's stretch begins (UINT64_MAX: the end of the file)
    bool has_share = false;
    uint64_t share_begin = 0, share_end = UINT64_MAX;
    size_t share_block = 0;               // the BGZF block share_begin lies in
    // npore_bam_set_output: what the NEXT file run on the handle writes (0 = SAM text, 1 = BAM records in stored BGZF
    // members), where its .bai goes ("" = none), NPORE_OUT_* flags, the records (out_rec: the three setters build it);
    // out_info: what that run wrote (npore_bam_output_info)
    int out_format = 0, out_flags = 0;
    npore::RecSpec out_rec;
    std::string out_bai;
    int64_t out_info[4] = {0, 0, 0, 0};
    int64_t inflate_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the device inflation of the last run on the handle (npore_bam_inflate_info)
    npore::RawBuf recs;                   // record bytes of the last npore_bam_format_bam
    double stage_ms[4] = {0, 0, 0, 0};    // last npore_bam_realign_batch: pack, align, standardise, format
    double file_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // last npore_bam_realign_file (npore_bam_file_timing)
};

struct npore_fasta {
    std::vector<std::string> names;
    npore::RawBuf bases;                  // all contigs back to back, upper-cased
    std::vector<int64_t> off;             // [n + 1] contig k = bases[off[k] .. off[k+1])
    uint64_t serial = 0;                  // unique per opened FASTA of the process (a context's device copy is keyed by it, not by the address)
    int64_t len(size_t k) const { return off[k + 1] - off[k]; }
    const char *seq(size_t k) const { return bases.p + off[k]; }
};

namespace npore {

// fixed part of a BAM alignment record, after block_size
struct RecView {
    const uint8_t *p;          // start of the fixed fields
    int32_t block_size;
    int32_t ref_id() const { return rdi32(p); }
    int32_t pos() const { return rdi32(p + 4); }
    int l_read_name() const { return p[8]; }
    int mapq() const { return p[9]; }
    int n_cigar() const { return rd16(p + 12); }
    int flag() const { return rd16(p + 14); }
    int32_t l_seq() const { return rdi32(p + 16); }
    const char *name() const { return reinterpret_cast<const char *>(p + 32); }
    const uint8_t *cigar() const { return p + 32 + l_read_name(); }
    const uint8_t *seq() const { return cigar() + 4 * (size_t)n_cigar(); }
    const uint8_t *qual() const { return seq() + ((size_t)l_seq() + 1) / 2; }
    const uint8_t *aux() const { return qual() + l_seq(); }
    const uint8_t *end() const { return p + block_size; }
    uint32_t cig(int k) const { return rd32(cigar() + 4 * (size_t)k); }
};

inline RecView rec_view(const uint8_t *q) { return RecView{q + 4, rdi32(q)}; }

inline RecView rec_of(const RecFetch &f, int64_t k) { return rec_view(f.ptr[(size_t)k]); }

inline bool bam_fetch(const npore_bam &b, const int64_t *idx, int64_t n, int threads, RecFetch &f, std::string &err)
{
    f.ptr.resize((size_t)n);
    if (!b.streamed) {
        for (int64_t k = 0; k < n; k++) f.ptr[(size_t)k] = b.data + b.rec_off[(size_t)idx[k]];
        return true;
    }
    // blocks touched by the records (a record may straddle blocks), as sorted runs of consecutive blocks
    auto block_of = [&](uint64_t off) {      // last block with out_off <= off and out_len > 0 covering it
        size_t lo = 0, hi = b.blocks.size();
        while (hi - lo > 1) { const size_t mid = (lo + hi) >> 1; if (b.blocks[mid].out_off <= off) lo = mid; else hi = mid; }
        return lo;
    };
    const int64_t n_rec = (int64_t)b.rec_off.size();
    std::vector<std::pair<size_t, size_t>> need((size_t)n);      // [first, last] block of each record
    for (int64_t k = 0; k < n; k++) {
        const uint64_t a = (uint64_t)b.rec_off[(size_t)idx[k]];
        const uint64_t e = idx[k] + 1 < n_rec ? (uint64_t)b.rec_off[(size_t)idx[k] + 1] : (uint64_t)b.data_size;
        need[(size_t)k] = {block_of(a), block_of(e ? e - 1 : 0)};
    }
    std::vector<std::pair<size_t, size_t>> runs(need);
    std::sort(runs.begin(), runs.end());
    size_t m = 0;
    for (size_t k = 0; k < runs.size(); k++) {
        if (m && runs[k].first <= runs[m - 1].second + 1) runs[m - 1].second = std::max(runs[m - 1].second, runs[k].second);
        else runs[m++] = runs[k];
    }
    runs.resize(m);
    std::vector<uint64_t> base(m + 1, 0);
    for (size_t k = 0; k < m; k++)
        base[k + 1] = base[k] + (b.blocks[runs[k].second].out_off + b.blocks[runs[k].second].out_len - b.blocks[runs[k].first].out_off);
    if (!f.buf.ensure((size_t)base[m] + 8)) { err = "out of memory"; return false; }
    for (size_t k = 0; k < m; k++)
        if (!bgzf_inflate_range(*b.file, b.blocks, runs[k].first, runs[k].second + 1, reinterpret_cast<uint8_t *>(f.buf.p) + base[k], threads)) {
            err = "corrupt BGZF block";
            return false;
        }
    for (int64_t k = 0; k < n; k++) {
        const size_t r = (size_t)(std::upper_bound(runs.begin(), runs.end(), std::make_pair(need[(size_t)k].first, (size_t)-1)) - runs.begin()) - 1;
        f.ptr[(size_t)k] = reinterpret_cast<const uint8_t *>(f.buf.p) + base[r] +
                           ((uint64_t)b.rec_off[(size_t)idx[k]] - b.blocks[runs[r].first].out_off);
    }
    return true;
}

// ---- the real CIGAR of a record ------------------------------------------------------------------------------------
// BAM keeps n_cigar_op in 16 bits; a read with more operations carries the placeholder CIGAR `<l_seq>S<reflen>N` and its
// real CIGAR in the tag CG:B,I (SAM specification 4.2.2).  A record has such a LONG CIGAR when all of this holds (htslib
// applies the same rule when it reads a record): n_cigar_op >= 1, refID >= 0, pos >= 0; the first operation is S with
// length l_seq; the tags hold CG of type B with subtype I or i; its count n satisfies n_cigar_op <= n < 2^29; the array
// lies inside the record.  Then the n words of the array are the record's CIGAR -- in every other case the record's own
// stands.  Everything that walks a CIGAR for the MEANING of the alignment (clips, lengths, pack, recount, purity, the
// writers) takes it from rec_cigar(); record_is_sound, the framing and seq() / qual() / aux() read the stored fields.
// The tags are walked only behind a first operation `l_seq S`: ordinary records pay one compare.
struct RecCigar {
    const uint8_t *w;          // the words, little-endian, unaligned
    uint32_t n;
    uint32_t op(uint32_t k) const { return rd32(w + 4 * (size_t)k); }
};

// bytes of the value of a tag of type `typ` at q (behind the three bytes of tag and type); 0: unknown type or the value
// leaves [q, end)
inline size_t aux_value_bytes(const uint8_t *q, const uint8_t *end, char typ)
{
    size_t w = 0;
    switch (typ) {
        case 'c': case 'C': case 'A': w = 1; break;
        case 's': case 'S': w = 2; break;
        case 'i': case 'I': case 'f': w = 4; break;
        case 'Z': case 'H': { const uint8_t *z = q; while (z < end && *z) z++; w = (size_t)(z - q) + 1; break; }
        case 'B': {
            if ((size_t)(end - q) < 5) return 0;
            const char sub = (char)q[0];
            const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            if (!es) return 0;
            w = 5 + (size_t)rd32(q + 1) * es;
            break;
        }
        default: return 0;
    }
    return w <= (size_t)(end - q) ? w : 0;
}

inline RecCigar rec_cigar(const RecView &r)
{
    const RecCigar own{r.cigar(), (uint32_t)r.n_cigar()};
    if (own.n < 1 || r.cig(0) != (((uint32_t)r.l_seq() << 4) | 4u) || r.l_seq() >= (1 << 28) || r.ref_id() < 0 || r.pos() < 0) return own;
    const uint8_t *q = r.aux(), *end = r.end();
    while (q + 3 <= end) {
        const bool is_cg = q[0] == 'C' && q[1] == 'G';
        const char typ = (char)q[2];
        q += 3;
        const size_t w = aux_value_bytes(q, end, typ);
        if (!w) return own;                                // a tag that cannot be stepped over: nothing behind it is read
        if (is_cg) {
            if (typ != 'B' || (q[0] != 'I' && q[0] != 'i')) return own;
            const uint32_t n = rd32(q + 1);
            return (n >= own.n && n < (1u << 29)) ? RecCigar{q + 5, n} : own;
        }
        q += w;
    }
    return own;
}

// reference length consumed: M, D, N, =, X  (pysam reference_length)
inline int64_t rec_ref_len(const RecCigar &cg)
{
    int64_t n = 0;
    for (uint32_t k = 0; k < cg.n; k++) {
        const uint32_t c = cg.op(k), op = c & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) n += c >> 4;
    }
    return n;
}
inline int64_t rec_ref_len(const RecView &r) { return rec_ref_len(rec_cigar(r)); }

// soft-clipped bases at either end (a hard clip may precede / follow them), src/bam.pyx:42-44 via
// pysam query_alignment_sequence
inline void rec_clips(const RecCigar &cg, int64_t &lead, int64_t &trail)
{
    const uint32_t nc = cg.n;
    lead = trail = 0;
    if (nc >= 1 && (cg.op(0) & 15u) == 4) lead = cg.op(0) >> 4;
    if (nc > 1 && (cg.op(0) & 15u) == 5 && (cg.op(1) & 15u) == 4) lead = cg.op(1) >> 4;
    if (nc > 1 && (cg.op(nc - 1) & 15u) == 4) trail = cg.op(nc - 1) >> 4;
    if (nc > 2 && (cg.op(nc - 1) & 15u) == 5 && (cg.op(nc - 2) & 15u) == 4) trail = cg.op(nc - 2) >> 4;
}
inline void rec_clips(const RecView &r, int64_t &lead, int64_t &trail) { rec_clips(rec_cigar(r), lead, trail); }

// ---- the tags a FULL record keeps (bam_reader.hpp FULL RECORD) ----------------------------------------------------------
// The input's aux bytes [q, end) in input order without the tags the realignment makes stale -- NM MD cs de dv CG, by
// their case-sensitive two-letter names, and with drop_oc (a run under NPORE_TAG_OC, RecSpec::oc()) OC as well: the run
// writes its own on the reads it changed, so no record carries two, and the device never parses tags -- copied to dst
// (nullptr: only counted); returns their bytes.  A tag that cannot be stepped over (aux_value_bytes returns 0) ends the
// list: it and everything behind it are dropped (rec_cigar's rule), and so are fewer than three bytes behind the last tag.
inline bool aux_tag_is_stale(const uint8_t *q, bool drop_oc)
{
    static const char stale[6][3] = {"NM", "MD", "cs", "de", "dv", "CG"};
    for (const char *t : stale)
        if (q[0] == (uint8_t)t[0] && q[1] == (uint8_t)t[1]) return true;
    return drop_oc && q[0] == 'O' && q[1] == 'C';
}
inline int64_t filter_aux(const uint8_t *q, const uint8_t *end, uint8_t *dst, bool drop_oc)
{
    int64_t n = 0;
    while (q + 3 <= end) {
        const size_t w = aux_value_bytes(q + 3, end, (char)q[2]);
        if (!w) break;
        if (!aux_tag_is_stale(q, drop_oc)) {
            if (dst) std::memcpy(dst + n, q, 3 + w);
            n += (int64_t)(3 + w);
        }
        q += 3 + w;
    }
    return n;
}
// ... of no run: the six stale tags alone (the model programs under tests/; every caller in the library names its run's)
inline int64_t filter_aux(const uint8_t *q, const uint8_t *end, uint8_t *dst) { return filter_aux(q, end, dst, false); }

// ---- staged heads: what the device gets of a record ------------------------------------------------------------------
// The kernels that read records (unpack, BAM emit, recount, purity) get each record's HEAD as it lies in the BAM stream
// -- block_size word | 32 bytes of fixed fields | name | CIGAR words | 4-bit bases | (STAGE_QUALS on) qualities |
// (STAGE_FULL) the kept aux bytes (filter_aux: the filter runs here, the device never parses tags) -- with ONE
// difference: the CIGAR words are the record's real ones (rec_cigar: those of the CG tag for a long-CIGAR record, in the
// place of the placeholder), and their count is 32-bit: its low half in the n_cigar_op field, its high half in the `bin`
// field, which no kernel reads (the emit kernel recomputes the bin).  stage_record_head() writes both halves for every
// record; staged_cigar() (staged_head.hpp) is the one reader, on the device and on the host.
enum : int { STAGE_HEAD = 0, STAGE_QUALS = 1, STAGE_FULL = 2 };      // (0 / 1: what `bool with_quals` used to say)
constexpr uint32_t PASS_NONE = 0;      // the mask under which nothing passes (staged_head.hpp record_passes)
inline int64_t staged_head_bytes(const RecView &r, const RecCigar &cg, int form, bool drop_oc)
{
    return 4 + 32 + (int64_t)r.l_read_name() + 4 * (int64_t)cg.n + (int64_t)((form != STAGE_HEAD ? r.aux() : r.qual()) - r.seq()) +
           (form == STAGE_FULL ? filter_aux(r.aux(), r.end(), nullptr, drop_oc) : 0);
}
// A READ's head -- nothing passes here: the recount, the purity run, and a run's reads below (drop_oc: filter_aux's, STAGE_FULL only)
inline int64_t staged_head_bytes(const uint8_t *rec, int form, bool drop_oc)
{
    const RecView r = rec_view(rec);
    return staged_head_bytes(r, rec_cigar(r), form, drop_oc);
}
// rec: the record, block_size word first; dst: staged_head_bytes(rec, form, drop_oc) bytes
inline void stage_record_head(const uint8_t *rec, int form, uint8_t *dst, bool drop_oc)
{
    const RecView r = rec_view(rec);
    const RecCigar cg = rec_cigar(r);
    const size_t fixed = 4 + 32 + (size_t)r.l_read_name(), tail = (size_t)((form != STAGE_HEAD ? r.aux() : r.qual()) - r.seq());
    if (cg.w == r.cigar()) std::memcpy(dst, rec, fixed + 4 * (size_t)cg.n + tail);
    else {
        std::memcpy(dst, rec, fixed);
        std::memcpy(dst + fixed, cg.w, 4 * (size_t)cg.n);
        std::memcpy(dst + fixed + 4 * (size_t)cg.n, r.seq(), tail);
    }
    if (form == STAGE_FULL) filter_aux(r.aux(), r.end(), dst + fixed + 4 * (size_t)cg.n + tail, drop_oc);
    dst[4 + 10] = (uint8_t)(cg.n >> 16); dst[4 + 11] = (uint8_t)(cg.n >> 24);      // bin: the count's high half
    dst[4 + 12] = (uint8_t)cg.n; dst[4 + 13] = (uint8_t)(cg.n >> 8);
}
// ... of no run (the counting paths, whose forms keep no aux, and the model programs under tests/)
inline int64_t staged_head_bytes(const uint8_t *rec, int form) { return staged_head_bytes(rec, form, false); }
inline void stage_record_head(const uint8_t *rec, int form, uint8_t *dst) { stage_record_head(rec, form, dst, false); }
// A RUN's record under its spec (there is no default: a run names what it writes).  A record that passes (staged_head.hpp
// record_passes; STAGE_FULL only) is staged verbatim -- the block_size word and the whole record as it lies in the stream, every
// tag, a long CIGAR still placeholder + CG tag, n_cigar_op and bin untouched; every other record is a read: its head.  How
// many bytes either takes, and where in a batch it starts: file_pipeline.hpp plan_staged_heads
inline void stage_record(const uint8_t *rec, int form, uint8_t *dst, const RecSpec &spec)
{
    if (form == STAGE_FULL && staged_passes(rec + 4, spec.pass_mask)) std::memcpy(dst, rec, (size_t)staged_pass_bytes(rec + 4));
    else stage_record_head(rec, form, dst, spec.oc());
}

// ---- the record buffer's bound: what one read's record takes at the most, term by term ---------------------------------
// The reference's record over `words` final CIGAR words and `sl` unclipped bases: fixed fields, name, words, bases,
// qualities, HP (+ 16: placeholder and CG tag head of a long final CIGAR).  The FULL record instead carries all l_seq
// bases, up to four clip words and the kept aux, and NM for HP.  MD: three bytes per reference position covered is the
// worst text, `0^A` repeated -- `0A` takes two per compared position --, and each of its `counts` numbers has at most 10
// digits (a batch's own finals cover the read's reference: one closing count; a caller's words may not: one per word).
// cs: no item of the text has more than three bytes per base it covers (cs_rec.hpp, Size); de: 7.  A record that passes
// takes exactly its staged_pass_bytes (staged_head.hpp) -- an ML-like array of tens of kilobytes included.
// OC (oc_rec.hpp): the tag's four bytes and, for each of the input's `words` real CIGAR words, its letter and a length of at most
// 28 bits, which has at most 9 digits -- ten bytes a word; only a changed read has the tag, the bound is taken for every read.
// =/X form (eqx_rec.hpp, Size): a word per compared position more than the final has at the most, four bytes each.
inline int64_t ref_record_bound(int64_t name, int64_t words, int64_t sl) { return 36 + name + 4 * words + 16 + (sl + 1) / 2 + sl + 7 + 16; }
inline int64_t full_record_bound(int64_t name, int64_t words, int64_t l_seq, int64_t aux) { return 36 + name + 4 * words + 32 + (l_seq + 1) / 2 + l_seq + aux + 7 + 16; }
inline int64_t md_tag_bound(int64_t ref_covered, int64_t counts) { return 4 + 3 * ref_covered + 11 * counts; }
inline int64_t cs_de_tags_bound(int64_t bases_covered) { return 4 + 3 * bases_covered + 7; }
inline int64_t oc_tag_bound(int64_t words) { return 4 + 10 * words; }

// The bound is record_bound() and nothing else: the named terms above have no other caller.  Its inputs are a record's own
// measures and the EXTENT of its final CIGAR -- what the final's words number and cover, which is all the terms ask of them.
struct RecMeasures {
    int64_t name, l_seq, sl;              // l_read_name (the NUL counted), all bases, the unclipped ones
    int64_t aux, in_words;                // the kept aux bytes (filter_aux under the run's spec), the words of the input's real CIGAR
    int64_t pass_bytes;                   // > 0: the record passes and takes these bytes (staged_pass_bytes), whatever else says
};
struct FinalExtent {
    int64_t words, ref_covered, md_counts, bases_covered;      // bases_covered: reference positions + read bases, as cs_de_tags_bound takes them
    int64_t eqx_extra;                    // words the =/X form may have beyond `words`
};
// ... of a batch's own final: it covers the read's rl reference positions and sl bases exactly, so it has no more words than
// rl + sl, closes one MD count, and its =/X form has no more than one word per position and base either (eqx_rec.hpp, Size)
inline FinalExtent own_final_extent(int64_t rl, int64_t sl) { return FinalExtent{rl + sl, rl, 1, rl + sl, 0}; }
// ... of a caller's n final words at w (little-endian, unaligned): they may run past the reference or the read and close a count
// at every word; the =/X form has at most a word per compared position more
inline FinalExtent words_final_extent(const uint8_t *w, int64_t n)
{
    FinalExtent e{n, 0, n + 1, 0, 0};
    for (int64_t q = 0; q < n; q++) {
        const uint32_t v = rd32(w + 4 * q), use = nm_consumes(v & 15u);
        if (use & 1u) e.ref_covered += v >> 4;
        if (use) e.bases_covered += v >> 4;
        if (nm_compares(v & 15u)) e.eqx_extra += v >> 4;
    }
    return e;
}
inline int64_t record_bound(const RecSpec &rec, const RecMeasures &m, const FinalExtent &e)
{
    if (m.pass_bytes > 0) return m.pass_bytes;
    if (!rec.full) return ref_record_bound(m.name, e.words, m.sl);
    int64_t bound = full_record_bound(m.name, e.words, m.l_seq, m.aux);
    if (rec.md) bound += md_tag_bound(e.ref_covered, e.md_counts);
    if (rec.cs_de()) bound += cs_de_tags_bound(e.bases_covered);
    if (rec.eqx()) bound += 4 * e.eqx_extra;
    if (rec.oc()) bound += oc_tag_bound(m.in_words);
    return bound;
}

// integer HP tag or 0 (src/bam.pyx:46)
inline int64_t rec_hp(const RecView &r)
{
    const uint8_t *q = r.aux(), *end = r.end();
    while (q + 3 <= end) {
        const bool is_hp = q[0] == 'H' && q[1] == 'P';
        const char typ = (char)q[2];
        q += 3;
        int64_t val = 0;
        size_t w = 0;
        if (q + 4 > end && typ != 'c' && typ != 'C' && typ != 'A' && typ != 'Z' && typ != 'H' && !(q + 2 <= end && (typ == 's' || typ == 'S')))
            return 0;                   // not enough bytes left for a 4-byte value
        if (q >= end) return 0;
        switch (typ) {
            case 'c': val = (int8_t)q[0]; w = 1; break;
            case 'C': val = q[0]; w = 1; break;
            case 's': val = (int16_t)rd16(q); w = 2; break;
            case 'S': val = rd16(q); w = 2; break;
            case 'i': val = rdi32(q); w = 4; break;
            case 'I': val = rd32(q); w = 4; break;
            case 'A': w = 1; break;
            case 'f': w = 4; break;
            case 'Z': case 'H': { const uint8_t *z = q; while (z < end && *z) z++; w = (size_t)(z - q) + 1; break; }
            case 'B': {
                if (q + 5 > end) return 0;
                const char sub = (char)q[0];
                const uint32_t cnt = rd32(q + 1);
                const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                w = 5 + (size_t)cnt * es;
                break;
            }
            default: return 0;
        }
        if (q + w > end) return 0;      // truncated tag
        if (is_hp && (typ == 'c' || typ == 'C' || typ == 's' || typ == 'S' || typ == 'i' || typ == 'I')) return val;
        q += w;
    }
    return 0;
}

static const char SEQ16[] = "=ACMGRSVTWYHKDBN";
static const char CIGOPS[] = "MIDNSHP=XB";

inline uint8_t base_code(char c)   // src/cig.pyx:212-229: 'NACGT-' -> 0..5, anything else 0 (upper case only)
{
    switch (c) { case 'A': return 1; case 'C': return 2; case 'G': return 3; case 'T': return 4; case '-': return 5; default: return 0; }
}

// base_code over a run of characters: compares and masks only, so the compiler vectorises it
inline void base_codes(const char *src, uint8_t *dst, int64_t n)
{
    for (int64_t q = 0; q < n; q++) {
        const char c = src[q];
        dst[q] = (uint8_t)((c == 'A' ? 1 : 0) + (c == 'C' ? 2 : 0) + (c == 'G' ? 3 : 0) + (c == 'T' ? 4 : 0) + (c == '-' ? 5 : 0));
    }
}

// base codes of n bases of a BAM record's 4-bit packed sequence from base `first` on: two per table lookup
inline void nibble_codes(const uint8_t *packed, int64_t first, uint8_t *dst, int64_t n)
{
    static const struct Tab {
        uint16_t pair[256];
        Tab() { for (int b = 0; b < 256; b++) pair[b] = (uint16_t)(base_code(SEQ16[b >> 4]) | (base_code(SEQ16[b & 15]) << 8)); }
    } tab;
    int64_t q = 0, t = first;
    if (n > 0 && (t & 1)) { dst[q++] = (uint8_t)(tab.pair[packed[t >> 1]] >> 8); t++; }
    const uint8_t *src = packed + (t >> 1);
    const int64_t pairs = (n - q) >> 1;
    for (int64_t j = 0; j < pairs; j++) {
        const uint16_t v = tab.pair[src[j]];
        dst[q + 2 * j] = (uint8_t)v;
        dst[q + 2 * j + 1] = (uint8_t)(v >> 8);
    }
    q += 2 * pairs;
    if (q < n) dst[q] = (uint8_t)tab.pair[src[pairs]];
}

// FASTA -> contig names + upper-cased bases, on all cores: the file is cut into pieces at line starts; a first
// pass counts the bases every piece contributes to the contig open at its start and to the contigs whose
// headers it contains, a second pass copies the lines to their final place.  Lines are trimmed of blanks, tabs
// and '\r' at both ends; a header's name is the text after '>' up to the first blank; bases before the first
// header are ignored.
inline bool fasta_parse(const ByteSpan &raw, int threads, npore_fasta &f)
{
    struct Piece {
        size_t beg = 0, end = 0;
        int64_t pre = 0;                              // bases before the piece's first header
        std::vector<std::pair<std::string, int64_t>> hdrs;   // (name, bases until the next header / piece end)
        int64_t pre_ctg = -1, pre_at = 0;             // destination of `pre`
        int64_t first_ctg = 0;                        // contig index of hdrs[0]
    };
    const size_t N = raw.n;
    const uint8_t *d = raw.p;
    const int nt = host_threads(threads);
    size_t np = std::max<size_t>(1, std::min<size_t>((size_t)nt * 4, N >> 18));
    std::vector<Piece> pc(np);
    size_t at = 0;
    for (size_t k = 0; k < np; k++) {
        pc[k].beg = at;
        size_t e = (k + 1 == np) ? N : std::max(at, N / np * (k + 1));
        if (e < N) {
            const void *nl = std::memchr(d + e, '\n', N - e);
            e = nl ? (size_t)(static_cast<const uint8_t *>(nl) - d) + 1 : N;
        }
        pc[k].end = at = e;
    }
    auto blank = [](uint8_t c) { return c == ' ' || c == '\t' || c == '\r'; };
    // calls on_header(name_begin, name_end) / on_bases(begin, end) for every line of [beg, end)
    auto walk = [&](size_t beg, size_t end, auto &&on_header, auto &&on_bases) {
        size_t p = beg;
        while (p < end) {
            const void *nl = std::memchr(d + p, '\n', end - p);
            const size_t e = nl ? (size_t)(static_cast<const uint8_t *>(nl) - d) : end;
            size_t le = e, ls = p;
            while (le > p && blank(d[le - 1])) le--;
            while (ls < le && (d[ls] == ' ' || d[ls] == '\t')) ls++;
            if (ls < le && d[ls] == '>') {
                size_t w = ls + 1;
                while (w < le && d[w] != ' ' && d[w] != '\t') w++;
                on_header(ls + 1, w);
            } else if (le > ls) {
                on_bases(ls, le);
            }
            p = e + 1;
        }
    };
    parallel_for((int64_t)np, threads, [&](int64_t k) {
        Piece &q = pc[(size_t)k];
        walk(q.beg, q.end,
             [&](size_t a, size_t b) { q.hdrs.emplace_back(std::string(reinterpret_cast<const char *>(d + a), b - a), 0); },
             [&](size_t a, size_t b) { (q.hdrs.empty() ? q.pre : q.hdrs.back().second) += (int64_t)(b - a); });
    });
    std::vector<int64_t> sizes;
    for (Piece &q : pc) {
        q.pre_ctg = (int64_t)sizes.size() - 1;
        if (q.pre_ctg >= 0) { q.pre_at = sizes.back(); sizes.back() += q.pre; }
        q.first_ctg = (int64_t)sizes.size();
        for (auto &h : q.hdrs) { f.names.push_back(std::move(h.first)); sizes.push_back(h.second); }
    }
    f.off.assign(sizes.size() + 1, 0);
    for (size_t k = 0; k < sizes.size(); k++) f.off[k + 1] = f.off[k] + sizes[k];
    if (!f.bases.ensure((size_t)f.off.back() + 1)) return false;
    parallel_for((int64_t)np, threads, [&](int64_t k) {
        const Piece &q = pc[(size_t)k];
        int64_t ctg = q.pre_ctg, next = q.first_ctg;
        char *w = ctg >= 0 ? f.bases.p + f.off[(size_t)ctg] + q.pre_at : nullptr;
        walk(q.beg, q.end,
             [&](size_t, size_t) { ctg = next++; w = f.bases.p + f.off[(size_t)ctg]; },
             [&](size_t a, size_t b) {
                 if (!w) return;
                 for (size_t i = a; i < b; i++) { const uint8_t c = d[i]; *w++ = (char)((c >= 'a' && c <= 'z') ? c - 32 : c); }
             });
    });
    return true;
}

}  // namespace npore
