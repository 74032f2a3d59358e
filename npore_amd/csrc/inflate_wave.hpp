// inflate_wave.hpp -- raw DEFLATE (RFC 1951) decoded by ONE WAVE per stream: the rule, stated ONCE and compiled for the
// gfx950 kernel (inflate_kernels.hpp inflate_blocks_kernel) and for the host twin (inflate_wave_host below, plain g++),
// the way confusion_rec.hpp, purity_rec.hpp and md_rec.hpp are.  The host twin runs the same code with the loop over the
// 64 lanes written out (NPORE_IW_LANES), per-lane registers as arrays of 64 (IwLane) and the waits as nothing.
//
// One stream in[0, in_len) must inflate to exactly out_len bytes (at most 65 536: a BGZF member's).  Result 1: inflated;
// 0: malformed, or one of the legal oddities inflate.hpp declines too (a literal / length code of a single symbol) -- the
// caller then hands the block to the host decoder, which decides.
//
// WHAT IS UNIFORM.  A DEFLATE stream is one dependent chain -- where a symbol's bits begin is known when the one before
// has been looked up -- so the chain is the WAVE's, not a lane's: the bit buffer (64 bits), the input and output
// positions, the table entry and every branch on them are the same in all lanes, and every value that comes from LDS or
// from another lane passes iw_uni() (readfirstlane), so that the compiler keeps them in scalar registers and the symbol
// loop is scalar code with scalar branches.  The lanes do what is wide:
//   input     a window of 512 bytes of the stream in two registers per lane (lane l: dwords l and 64 + l), loaded by the
//             whole wave in 256-byte rows; the bit buffer takes 32 bits at a time from it by readlane, no memory access
//   literals  gathered one per lane in a register (lane k keeps the k-th pending one) and stored as a run of up to 64
//             consecutive bytes by one vector store
//   matches   copied by all lanes at once: byte k of a match of distance d and length len is out[o - d + k] where
//             d >= len and out[o - d + (k mod d)] where d < len, so that an overlapping match needs no serial loop
//   tables    counted, ranked and spread into the primary tables with a symbol per lane
// READING ITS OWN OUTPUT.  A match reads bytes this wave stored a moment ago.  Those reads are per-lane (vector) loads
// through a pointer that is neither const nor restrict, behind iw_stores_done(): a wait for every store of the wave.
//
// TABLES (IwTables, 3 676 bytes of LDS per wave: eight waves per SIMD fit the CU's 160 KiB).  A primary table of 16-bit
// entries `symbol << 4 | bits` indexed by the next 10 bits (literal / length) or 8 bits (distance); an entry 0 means the
// code is longer (or invalid), and the symbol is then found the canonical way, a bit at a time, over the counts per
// length and the symbols sorted by (length, symbol).  The code-length code has that second form only.  Length and
// distance bases are computed, not looked up.
//
// VALIDITY, as inflate.hpp has it: an over-subscribed or incomplete code set is refused -- but one 1-bit distance code
// and no distance code at all are legal --, HLIT > 286, HDIST > 30, a missing end-of-block code, a repeat without a
// length before it or past the end, a stored block whose LEN / NLEN disagree, block type 3.
// BOUNDS.  Every read lies in [in, in + in_len) (bytes beyond read as zero, and a stream that USES a bit beyond is
// malformed), every write and every match's source in [out, out + out_len): a distance that reaches in front of out, a
// length or a literal that reaches past out_len, a stream that ends short of out_len are malformed.
// TERMINATION.  Every iteration of every loop consumes at least one bit of the stream or produces at least one byte, and
// stops when more bits than the input has were consumed; over that, the symbol loops share one budget of
// 8 * in_len + out_len + 64 iterations.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NPORE_IW_HD __host__ __device__ __forceinline__
#else
#define NPORE_IW_HD inline
#endif

namespace npore {

constexpr int IW_LIT_BITS = 10, IW_DIST_BITS = 8;
constexpr uint32_t IW_MAX_OUT = 65536u, IW_MAX_IN = 1u << 27;       // (8 * in_len stays a 32-bit number)
constexpr uint32_t IW_WINDOW = 512;                                 // bytes of input held in the lanes' registers

// one wave's tables (LDS on the device)
struct IwTables {
    uint16_t lit[1 << IW_LIT_BITS];        // primary, literal / length
    uint16_t dist[1 << IW_DIST_BITS];      // primary, distance
    uint16_t lit_sym[288], dist_sym[32], cl_sym[20];     // symbols sorted by (code length, symbol)
    uint16_t lit_cnt[16], dist_cnt[16], cl_cnt[16];      // codes per length
    uint8_t lens[288 + 32];                // the code lengths being read
    uint8_t cl_lens[20];
};
static_assert(sizeof(IwTables) <= 5120, "one wave's tables must fit in 160 KiB / 32");

#if defined(__HIP_DEVICE_COMPILE__)
#define NPORE_IW_LANES(l) for (int l = (int)(threadIdx.x & 63u), once_ = 1; once_; once_ = 0)
template <class T> struct IwLane {
    T v;
    __device__ __forceinline__ T &at(int) { return v; }
};
__device__ __forceinline__ uint32_t iw_uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint32_t iw_lane_get(IwLane<uint32_t> &r, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)r.v, (int)lane); }
// every store of this wave has completed: what it wrote may be read back by any of its lanes
__device__ __forceinline__ void iw_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// the wave's LDS accesses complete in order; this keeps the compiler from moving one across
__device__ __forceinline__ void iw_tables_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
#else
#define NPORE_IW_LANES(l) for (int l = 0; l < 64; l++)
template <class T> struct IwLane {
    T v[64];
    NPORE_IW_HD T &at(int l) { return v[l]; }
};
NPORE_IW_HD uint32_t iw_uni(uint32_t x) { return x; }
NPORE_IW_HD uint32_t iw_lane_get(IwLane<uint32_t> &r, uint32_t lane) { return r.v[lane]; }
NPORE_IW_HD void iw_stores_done() {}
NPORE_IW_HD void iw_tables_done() {}
#endif

NPORE_IW_HD uint32_t iw_reverse(uint32_t code, uint32_t bits)        // the low `bits` (1 ... 15) of code, reversed
{
    uint32_t v = code;
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
    v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
    return v >> (16u - bits);
}
// length symbol s (257 ... 285): base and number of extra bits; distance symbol s (0 ... 29) likewise
NPORE_IW_HD void iw_len_of(uint32_t s, uint32_t &base, uint32_t &extra)
{
    if (s < 265u) { base = s - 254u; extra = 0; }
    else if (s == 285u) { base = 258u; extra = 0; }
    else { extra = (s - 261u) >> 2; base = ((4u + ((s - 265u) & 3u)) << extra) + 3u; }
}
NPORE_IW_HD void iw_dist_of(uint32_t s, uint32_t &base, uint32_t &extra)
{
    if (s < 4u) { base = s + 1u; extra = 0; }
    else { extra = (s >> 1) - 1u; base = ((2u + (s & 1u)) << extra) + 1u; }
}

struct InflateWave {
    const uint8_t *in;
    uint8_t *out;                          // (never const, never restrict: matches read what this wave stored)
    uint32_t in_len, out_len;
    IwTables &t;
    uint64_t bb = 0;                       // bit buffer, LSB first
    uint32_t bc = 0;                       // bits in it
    uint32_t ip = 0;                       // bytes of the stream taken into it (zeros beyond in_len count)
    uint32_t wbase = 0;                    // the window holds stream bytes [wbase, wbase + IW_WINDOW)
    bool have_window = false;
    uint32_t o = 0;                        // bytes produced, the pending literals among them
    uint32_t pending = 0;                  // literals not stored yet: lane k has out[o - pending + k]
    uint32_t budget;
    IwLane<uint32_t> w0, w1, lits;

    NPORE_IW_HD InflateWave(const uint8_t *in_, uint32_t in_len_, uint8_t *out_, uint32_t out_len_, IwTables &t_)
        : in(in_), out(out_), in_len(in_len_), out_len(out_len_), t(t_), budget(8u * in_len_ + out_len_ + 64u)
    {
    }

    // ---- input
    NPORE_IW_HD uint32_t in_byte(uint32_t at) const { return at < in_len ? in[at] : 0u; }
    NPORE_IW_HD void load_window(uint32_t base)
    {
        NPORE_IW_LANES(l)
        {
            const uint32_t a = base + 4u * (uint32_t)l, b = a + 256u;
            w0.at(l) = in_byte(a) | in_byte(a + 1) << 8 | in_byte(a + 2) << 16 | in_byte(a + 3) << 24;
            w1.at(l) = in_byte(b) | in_byte(b + 1) << 8 | in_byte(b + 2) << 16 | in_byte(b + 3) << 24;
        }
        wbase = base;
        have_window = true;
    }
    NPORE_IW_HD uint32_t window_dword(uint32_t i) { return i < 64u ? iw_lane_get(w0, i) : iw_lane_get(w1, i - 64u); }
    // at least 33 bits in the buffer (a length with its extra bits, or a distance with its own, is at most 28)
    NPORE_IW_HD void refill()
    {
        while (bc <= 32u) {
            if (!have_window || ip < wbase || ip + 8u > wbase + IW_WINDOW) load_window(ip & ~3u);
            const uint32_t off = ip - wbase, i = off >> 2, sh = (off & 3u) * 8u;
            const uint64_t two = (uint64_t)window_dword(i) | (uint64_t)window_dword(i + 1u) << 32;
            bb |= (uint64_t)(uint32_t)(two >> sh) << bc;
            bc += 32u;
            ip += 4u;
        }
    }
    NPORE_IW_HD bool overrun() const { return 8u * ip - bc > 8u * in_len; }      // a bit beyond the input was consumed
    NPORE_IW_HD uint32_t peek(uint32_t n) const { return (uint32_t)bb & ((1u << n) - 1u); }
    NPORE_IW_HD void drop(uint32_t n) { bb >>= n; bc -= n; }
    NPORE_IW_HD uint32_t take(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }

    // ---- codes
    // The symbol of the code the buffer begins with (>= 15 bits are there), or -1: prim: the primary table of pb bits
    // (nullptr: none), cnt / sym: the canonical form
    NPORE_IW_HD int decode(const uint16_t *prim, uint32_t pb, const uint16_t *cnt, const uint16_t *sym)
    {
        if (prim) {
            const uint32_t e = iw_uni(prim[peek(pb)]);
            if (e & 15u) { drop(e & 15u); return (int)(e >> 4); }
        }
        int code = 0, first = 0, index = 0;
        for (uint32_t len = 1; len <= 15u; len++) {
            code |= (int)((bb >> (len - 1u)) & 1u);
            const int count = (int)iw_uni(cnt[len]);
            if (code - count < first) { drop(len); return (int)iw_uni(sym[index + (code - first)]); }
            index += count;
            first += count;
            first <<= 1;
            code <<= 1;
        }
        return -1;
    }
    // Tables of the n code lengths at len[]: false if the set is over-subscribed or incomplete (one_code_ok: a single
    // code of one bit is taken, as zlib takes it for distances); no code at all gives tables in which nothing decodes
    NPORE_IW_HD bool build(const uint8_t *len, uint32_t n, uint16_t *cnt, uint16_t *sym, uint16_t *prim, uint32_t pb, bool one_code_ok)
    {
        iw_tables_done();
        NPORE_IW_LANES(l)
        {
            if (l < 16) {
                uint32_t c = 0;
                for (uint32_t i = 0; i < n; i++) c += len[i] == (uint8_t)l ? 1u : 0u;
                cnt[l] = (uint16_t)c;
            }
            if (prim)
                for (uint32_t k = (uint32_t)l; k < (1u << pb); k += 64u) prim[k] = 0;
        }
        iw_tables_done();
        int left = 1;
        uint32_t c1 = 0;
        for (uint32_t b = 1; b < 16u; b++) {
            const uint32_t c = iw_uni(cnt[b]);
            if (b == 1u) c1 = c;
            left = (left << 1) - (int)c;
            if (left < 0) return false;
        }
        const uint32_t c0 = iw_uni(cnt[0]);
        if (c0 == n) return true;
        if (left > 0 && !(one_code_ok && c0 == n - 1u && c1 == 1u)) return false;
        NPORE_IW_LANES(l)
        {
            for (uint32_t i = (uint32_t)l; i < n; i += 64u) {
                const uint32_t L = len[i];
                if (!L) continue;
                uint32_t rank = 0, at = 0, code = 0;            // among the symbols of this length; where the length begins
                for (uint32_t j = 0; j < i; j++) rank += len[j] == (uint8_t)L ? 1u : 0u;
                for (uint32_t b = 1; b < L; b++) { at += cnt[b]; code = (code + cnt[b]) << 1; }
                sym[at + rank] = (uint16_t)i;
                if (prim && L <= pb) {
                    const uint16_t e = (uint16_t)(i << 4 | L);
                    for (uint32_t k = iw_reverse(code + rank, L); k < (1u << pb); k += 1u << L) prim[k] = e;
                }
            }
        }
        iw_tables_done();
        return true;
    }
    NPORE_IW_HD bool fixed_tables()
    {
        NPORE_IW_LANES(l)
        {
            for (uint32_t i = (uint32_t)l; i < 320u; i += 64u)
                t.lens[i] = (uint8_t)(i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : i < 288u ? 8 : 5);
        }
        return build(t.lens, 288, t.lit_cnt, t.lit_sym, t.lit, IW_LIT_BITS, false) &&
               build(t.lens + 288, 32, t.dist_cnt, t.dist_sym, t.dist, IW_DIST_BITS, false);
    }
    // (a value every lane stores to the same place)
    NPORE_IW_HD static void put8(uint8_t *p, uint32_t v) { *p = (uint8_t)v; }
    NPORE_IW_HD bool dynamic_tables()
    {
        refill();
        const uint32_t hlit = take(5) + 257u, hdist = take(5) + 1u, hclen = take(4) + 4u;
        if (hlit > 286u || hdist > 30u) return false;
        NPORE_IW_LANES(l) { if (l < 20) t.cl_lens[l] = 0; }
        iw_tables_done();
        for (uint32_t i = 0; i < hclen; i++) {
            refill();
            const uint32_t at = i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 8u - (i - 3u) / 2u : 8u + (i - 4u) / 2u;      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
            put8(t.cl_lens + at, take(3));
        }
        if (overrun()) return false;
        if (!build(t.cl_lens, 19, t.cl_cnt, t.cl_sym, nullptr, 0, false)) return false;
        const uint32_t total = hlit + hdist;
        uint32_t prev = 0;
        for (uint32_t i = 0; i < total;) {
            refill();
            if (overrun()) return false;
            const int s = decode(nullptr, 0, t.cl_cnt, t.cl_sym);
            if (s < 0) return false;
            if (s < 16) { put8(t.lens + i, (uint32_t)s); prev = (uint32_t)s; i++; continue; }
            uint32_t rep, v = 0;
            if (s == 16) { if (i == 0) return false; v = prev; rep = 3u + take(2); }
            else if (s == 17) rep = 3u + take(3);
            else rep = 11u + take(7);
            if (i + rep > total) return false;
            NPORE_IW_LANES(l)
            {
                for (uint32_t k = (uint32_t)l; k < rep; k += 64u) t.lens[i + k] = (uint8_t)v;
            }
            prev = v;
            i += rep;
        }
        if (overrun()) return false;
        iw_tables_done();
        if (iw_uni(t.lens[256]) == 0u) return false;              // no end-of-block code
        return build(t.lens, hlit, t.lit_cnt, t.lit_sym, t.lit, IW_LIT_BITS, false) &&
               build(t.lens + hlit, hdist, t.dist_cnt, t.dist_sym, t.dist, IW_DIST_BITS, true);
    }

    // ---- output
    NPORE_IW_HD void flush()
    {
        if (!pending) return;
        const uint32_t at = o - pending;
        NPORE_IW_LANES(l) { if ((uint32_t)l < pending) out[at + (uint32_t)l] = (uint8_t)lits.at(l); }
        pending = 0;
    }
    // the symbols of a compressed block whose tables are ready, to its end-of-block code
    NPORE_IW_HD bool codes()
    {
        for (;;) {
            if (budget-- == 0u) return false;
            refill();
            if (overrun()) return false;
            const int s = decode(t.lit, IW_LIT_BITS, t.lit_cnt, t.lit_sym);
            if (s < 0) return false;
            if (s < 256) {
                if (o >= out_len) return false;
                NPORE_IW_LANES(l) { if ((uint32_t)l == pending) lits.at(l) = (uint32_t)s; }
                o++;
                if (++pending == 64u) flush();
                continue;
            }
            if (s == 256) return !overrun();
            if (s > 285) return false;
            uint32_t base, extra;
            iw_len_of((uint32_t)s, base, extra);
            const uint32_t len = base + take(extra);
            refill();
            const int ds = decode(t.dist, IW_DIST_BITS, t.dist_cnt, t.dist_sym);
            if (ds < 0 || ds > 29) return false;
            iw_dist_of((uint32_t)ds, base, extra);
            const uint32_t d = base + take(extra);
            if (overrun()) return false;
            if (d > o || len > out_len - o) return false;
            flush();
            iw_stores_done();
            uint8_t *const dst = out + o;
            const uint8_t *const src = dst - d;
            if (d >= len) {
                NPORE_IW_LANES(l) { for (uint32_t k = (uint32_t)l; k < len; k += 64u) dst[k] = src[k]; }
            } else {                                               // overlapping: the d bytes in front of o, over and over
                NPORE_IW_LANES(l) { for (uint32_t k = (uint32_t)l; k < len; k += 64u) dst[k] = src[k % d]; }
            }
            o += len;
        }
    }
    NPORE_IW_HD bool stored()
    {
        drop(bc & 7u);
        refill();
        const uint32_t n = take(16), nn = take(16);
        if ((n ^ nn) != 0xFFFFu || overrun()) return false;
        const uint32_t at = ip - (bc >> 3);                        // the bit buffer holds whole bytes: give them back
        if (at > in_len || n > in_len - at || n > out_len - o) return false;
        flush();
        NPORE_IW_LANES(l)
        {
            for (uint32_t k = (uint32_t)l; k < n; k += 64u) out[o + k] = in[at + k];
        }
        o += n;
        ip = at + n;
        bb = 0;
        bc = 0;
        return true;
    }
    NPORE_IW_HD int run()
    {
        if (in_len > IW_MAX_IN || out_len > IW_MAX_OUT) return 0;
        for (;;) {
            if (budget-- == 0u) return 0;
            refill();
            const uint32_t last = take(1), type = take(2);
            if (overrun()) return 0;
            if (type == 0u) { if (!stored()) return 0; }
            else if (type == 3u) return 0;
            else {
                if (!(type == 1u ? fixed_tables() : dynamic_tables())) return 0;
                if (!codes()) return 0;
            }
            if (last) break;
        }
        flush();
        return o == out_len && !overrun() ? 1 : 0;
    }
};

// n independent streams by the host twin: stream k is in[in_off[k] .. + in_len[k]) and must inflate to the out_len[k]
// bytes at out + out_off[k]; status[k] as the kernel gives it
inline void inflate_wave_host(const uint8_t *in, const int64_t *in_off, const int64_t *in_len, uint8_t *out, const int64_t *out_off,
                              const int64_t *out_len, int64_t n, int32_t *status)
{
    static thread_local IwTables t;
    for (int64_t k = 0; k < n; k++) {
        if (in_len[k] < 0 || in_len[k] > (int64_t)IW_MAX_IN || out_len[k] < 0 || out_len[k] > (int64_t)IW_MAX_OUT) { status[k] = 0; continue; }
        InflateWave w(in + in_off[k], (uint32_t)in_len[k], out + out_off[k], (uint32_t)out_len[k], t);
        status[k] = w.run();
    }
}

}  // namespace npore
