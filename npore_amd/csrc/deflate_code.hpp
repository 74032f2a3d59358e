// deflate_code.hpp -- the rule by which a BGZF member's payload becomes ONE dynamic-Huffman DEFLATE block of literals
// (BAM out, --bam_compress huffman), written once and compiled for the host (bam_reader.hpp: the host twin) and for the
// gfx950 kernels (bam_deflate_kernels.hpp).  npore_amd/bam.py deflate_member states the same rule in Python.
//
// THE MEMBER.  The record stream is cut every 65 280 bytes counted from its first byte, whatever the mode.  A member is
// the 18-byte BGZF header (BSIZE = member size - 1), the DEFLATE stream, CRC-32 and ISIZE of the payload.  The stream is
// one final block of type 2 that holds the payload's bytes as literals and the end-of-block symbol: no length symbol,
// no match.  HLIT = 257 symbols; HDIST = 1 distance code of length 0 (no distance code at all: the smallest form that
// both zlib and inflate.hpp take).  A payload of 0 bytes, or one whose block would take >= payload + 5 bytes, is written
// as the stored block (member = payload + 31 bytes), byte for byte as the stored mode writes it.
//
// CODE LENGTHS (deflate_lengths), for an alphabet with frequencies f[0 .. n), at most `limit` bits:
//   1. the symbols with f > 0 in ascending order of (f, symbol);
//   2. Huffman's algorithm on that order in the in-place form of Moffat and Katajainen: two queues, the leaves and the
//      internal nodes in order of creation; of a leaf and an internal node of equal weight the LEAF is taken first.  This
//      gives every leaf its depth; the depths fall from the first (rarest) leaf to the last;
//   3. limit: the number of codes per length is counted, depths beyond `limit` counted as `limit`; while the Kraft sum
//      (in units of 2^-limit) exceeds 1, one code of length `limit` is taken away, the longest shorter length that has a
//      code gives one up and the length above it gains two (the sum falls by one unit each time);
//   4. the lengths go to the symbols in the order of step 1, the longest first.
//   Without step 3 acting the sum of f * length is Huffman's optimum.  Literals: limit 15; code-length alphabet: 7.
// CODES: canonical (RFC 1951 3.2.2).
// THE CODE-LENGTH SEQUENCE: the 257 literal / end-of-block lengths and the one distance length 0, as one sequence of 258,
//   cut into maximal runs of equal values (a run may span the two tables).  A run of r zeros: symbol 18 (11 ... 138) while
//   r >= 11, each taking min(r, 138); then one symbol 17 if r >= 3; then single zeros.  A run of r times v > 0: v once;
//   then symbol 16 (3 ... 6) while r >= 3, each taking min(r, 6); then single v's.  HCLEN: up to the last code-length
//   symbol of RFC order that is used, at least 4.
// From the histogram alone: header bits = 17 + 3 * HCLEN + sum over the sequence's symbols of (code length + extra
// bits); data bits = sum f * length (end-of-block has f = 1); the block takes (header + data + 7) / 8 bytes.
//
// MATCHES (--bam_compress match; DEFLATE_MODE_MATCH).  The member's block holds literals AND length / distance pairs.  For a
// payload p[0 .. n), n <= 65 280:
//   1. HASH.  H(i), for i <= n - 4: the four bytes at i read little-endian as a 32-bit word, times 2654435761 modulo 2^32,
//      the top 15 bits.
//   2. CANDIDATE.  c(i): the greatest j < i with H(j) = H(i), or none -- the nearest earlier position of equal HASH, whatever
//      its bytes: collisions are part of the rule, so a table that keeps the most recent position per bucket is exact.
//   3. MATCH.  L(i): the number of equal bytes p[c(i) + k] = p[i + k], at most min(258, n - i); source and target may
//      overlap.  A match iff L(i) >= 4 and i - c(i) <= 32 768.
//   4. GREEDY PARSE from 0: at a position with a match the token (length L, distance i - c), on at i + L; otherwise a
//      literal, on at i + 1.  No lazy evaluation.  End-of-block comes last.
//   5. ALPHABETS.  Literal / length symbols 0 ... 285 and distance symbols 0 ... 29 with the bases and extra bits of RFC 1951
//      3.2.5.  HLIT = max(257, highest used literal / length symbol + 1); HDIST = max(1, highest used distance symbol + 1).
//      Code lengths of both by deflate_lengths, limit 15 (a single used distance symbol: the one 1-bit code); canonical
//      codes; the code-length sequence and HCLEN by the run rule above on the HLIT + HDIST lengths as ONE sequence.  The
//      literals-only block is the case HLIT = 257, HDIST = 1 with the distance length 0.
//   6. CHOICE.  m: bytes of this block; h: bytes of the literals-only block.  The match block is written iff m < h and
//      m < n + 5; otherwise exactly the member of the literals-only rule (its block, or the stored block if h >= n + 5).
//      So size(match) <= size(huffman) <= n + 31 for every payload, and a payload without a match gives the literals-only
//      member byte for byte.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define NPORE_DFL_HD __host__ __device__ __forceinline__
#else
#define NPORE_DFL_HD inline
#endif

namespace npore {

constexpr int DEFLATE_MEMBER_PAYLOAD = 0xFF00;     // (BGZF_STORED_PAYLOAD)
constexpr int DEFLATE_NSYM = 257, DEFLATE_NSEQ = 258;       // the literals-only block: its alphabet, its code-length sequence
constexpr int DEFLATE_NLL = 286, DEFLATE_NDIST = 30;        // the alphabets of a block with matches
// the block header's bytes at the most: 17 + 3 * 19 bits, then at most 7 bits for each of the 286 + 30 lengths (a symbol with
// extra bits stands for three lengths at the least)
constexpr int DEFLATE_HDR_CAP = 296;
constexpr int DEFLATE_MODE_HUFFMAN = 1, DEFLATE_MODE_MATCH = 2;
constexpr int DEFLATE_HASH_BITS = 15, DEFLATE_MIN_MATCH = 4, DEFLATE_MAX_MATCH = 258, DEFLATE_MAX_DIST = 32768;
constexpr uint32_t DEFLATE_NO_POS = 0xFFFFu;                // (a position is < 65 280)

// ---- CRC-32 as polynomial arithmetic (reflected, as zlib's crc32_combine): what the device needs to join slices
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b)         // a(x) * b(x) mod P
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
constexpr uint32_t crc_xpow_bytes(uint64_t n)                 // x^(8 n) mod P
{
    uint32_t r = 1u << 31, sq = 1u << 23;                     // 1, x^8
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mulmod(r, sq);
        sq = crc_mulmod(sq, sq);
    }
    return r;
}
// the register after one more byte (no conditioning: init and final complement are the caller's)
NPORE_DFL_HD uint32_t crc_byte(uint32_t c, uint32_t byte)
{
    c ^= byte;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
    return c;
}

// ---- the plan of one member: everything but the payload's bits.  4.6 KB: a workgroup's LDS on the device
struct DeflateWork {
    uint32_t freq[DEFLATE_NLL];        // in: the histogram, freq[256] = 1; out: code[s] = length << 16 | code, bit-reversed
    uint32_t dfreq[DEFLATE_NDIST];     // the same of the distance symbols (matches only)
    uint32_t a[DEFLATE_NLL];           // scratch: weights / depths by rank
    uint16_t sym[DEFLATE_NLL + 2];     // scratch: symbol by rank
    uint8_t lens[DEFLATE_NLL + DEFLATE_NDIST + 4];      // lengths of the HLIT symbols, behind them of the HDIST distance codes
    uint8_t dlens[DEFLATE_NDIST + 2];
    uint16_t seq[DEFLATE_NLL + DEFLATE_NDIST + 2];      // the code-length sequence: symbol | extra << 8
    uint32_t clfreq[19], clcode[19];
    uint8_t cllens[20];
    uint32_t count[17], next[17];
    uint32_t n_seq, hclen, hdr_bits, data_bits, hlit, hdist;
};

// ---- the rule's steps 1 to 3 and the symbols of step 5
NPORE_DFL_HD uint32_t deflate_hash(uint32_t word) { return (word * 2654435761u) >> (32 - DEFLATE_HASH_BITS); }
// length 3 ... 258 -> symbol | extra bits << 16 | their value << 24
NPORE_DFL_HD uint32_t deflate_len_symbol(uint32_t len)
{
    const uint32_t l = len - 3;
    if (l < 8) return 257 + l;
    if (len == 258) return 285;
    const uint32_t e = (uint32_t)(31 - __builtin_clz(l)) - 2;
    return (261 + 4 * e + ((l >> e) & 3u)) | e << 16 | (l & ((1u << e) - 1)) << 24;
}
// distance 1 ... 32 768 -> symbol | extra bits << 8 | their value << 16
NPORE_DFL_HD uint32_t deflate_dist_symbol(uint32_t dist)
{
    const uint32_t d = dist - 1;
    if (d < 4) return d;
    const uint32_t lg = (uint32_t)(31 - __builtin_clz(d)), e = lg - 1;
    return (2 * lg + ((d >> e) & 1u)) | e << 8 | (d & ((1u << e) - 1)) << 16;
}

// step 1 for the symbols of freq[0 .. n): a[rank] = weight, sym[rank] = symbol; returns how many are used
NPORE_DFL_HD int deflate_sort(const uint32_t *freq, int n, uint32_t *a, uint16_t *sym)
{
    int m = 0;
    for (int s = 0; s < n; s++) {
        const uint32_t f = freq[s];
        if (!f) continue;
        int k = m++;
        for (; k > 0 && a[k - 1] > f; k--) { a[k] = a[k - 1]; sym[k] = sym[k - 1]; }     // (equal weights: the smaller symbol stays in front)
        a[k] = f;
        sym[k] = (uint16_t)s;
    }
    return m;
}

// steps 2 to 4: the m used symbols sorted in a / sym -> lens[symbol] (the caller has zeroed lens)
NPORE_DFL_HD void deflate_lengths_sorted(uint32_t *a, const uint16_t *sym, int m, int limit, uint32_t *count, uint8_t *lens)
{
    if (m == 0) return;
    if (m == 1) { lens[sym[0]] = 1; return; }
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < m - 1; next++) {
        if (leaf >= m || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; }
        else a[next] = a[leaf++];
        if (leaf >= m || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; }
        else a[next] += a[leaf++];
    }
    a[m - 2] = 0;
    for (int next = m - 3; next >= 0; next--) a[next] = a[a[next]] + 1;
    {
        int avbl = 1, used = 0, dpth = 0, rt = m - 2, nx = m - 1;
        while (avbl > 0) {
            while (rt >= 0 && (int)a[rt] == dpth) { used++; rt--; }
            while (avbl > used) { a[nx--] = (uint32_t)dpth; avbl--; }
            avbl = 2 * used; dpth++; used = 0;
        }
    }
    for (int l = 0; l <= limit; l++) count[l] = 0;
    for (int k = 0; k < m; k++) count[(int)a[k] < limit ? a[k] : (uint32_t)limit]++;
    uint32_t total = 0;
    for (int l = limit; l > 0; l--) total += count[l] << (limit - l);
    while (total != (1u << limit)) {
        count[limit]--;
        for (int l = limit - 1; l > 0; l--)
            if (count[l]) { count[l]--; count[l + 1] += 2; break; }
        total--;
    }
    int k = 0;
    for (int l = limit; l > 0; l--)
        for (uint32_t c = 0; c < count[l]; c++) lens[sym[k++]] = (uint8_t)l;
}

// canonical codes of lens[0 .. n), bit-reversed for an LSB-first stream: code[s] = length << 16 | bits
NPORE_DFL_HD void deflate_codes(const uint8_t *lens, int n, uint32_t *count, uint32_t *next, uint32_t *code)
{
    for (int l = 0; l <= 15; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[lens[s]]++;
    count[0] = 0;
    uint32_t c = 0;
    for (int l = 1; l <= 15; l++) { c = (c + count[l - 1]) << 1; next[l] = c; }
    for (int s = 0; s < n; s++) {
        const uint32_t l = lens[s];
        if (!l) { code[s] = 0; continue; }
        const uint32_t v = next[l]++;
        uint32_t rev = 0;
        for (uint32_t b = 0; b < l; b++) rev |= ((v >> b) & 1u) << (l - 1 - b);
        code[s] = l << 16 | rev;
    }
}

NPORE_DFL_HD int deflate_cl_order(int k)
{
    // RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return k == 0 ? 16 : k == 1 ? 17 : k == 2 ? 18 : k == 3 ? 0 : (k & 1) ? 8 - (k - 4 + 1) / 2 : 8 + (k - 4) / 2;
}
NPORE_DFL_HD uint32_t deflate_cl_extra_bits(uint32_t s) { return s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u; }

// Everything behind step 1 of the literal (matches: literal / length) alphabet: w.a / w.sym hold the m used symbols in
// order, w.freq the histogram (matches: w.dfreq that of the distance symbols).  Leaves the codes in w.freq (and w.dfreq), the
// sequence, its codes, HLIT, HDIST, HCLEN and the two bit counts.
NPORE_DFL_HD void deflate_plan_sorted(DeflateWork &w, int m, bool matches = false)
{
    const int nll = matches ? DEFLATE_NLL : DEFLATE_NSYM;
    for (int s = 0; s < DEFLATE_NLL + DEFLATE_NDIST + 4; s++) w.lens[s] = 0;
    deflate_lengths_sorted(w.a, w.sym, m, 15, w.count, w.lens);
    uint32_t bits = 0;
    int hlit = DEFLATE_NSYM, hdist = 1;
    for (int s = 0; s < nll; s++) {
        bits += w.freq[s] * w.lens[s];
        if (s >= DEFLATE_NSYM && w.freq[s]) {           // (a length symbol: its extra bits)
            if (s >= 265 && s < 285) bits += w.freq[s] * (uint32_t)((s - 261) / 4);
            hlit = s + 1;
        }
    }
    deflate_codes(w.lens, nll, w.count, w.next, w.freq);
    if (matches) {
        for (int s = 0; s < DEFLATE_NDIST + 2; s++) w.dlens[s] = 0;
        const int md = deflate_sort(w.dfreq, DEFLATE_NDIST, w.a, w.sym);
        deflate_lengths_sorted(w.a, w.sym, md, 15, w.count, w.dlens);
        for (int s = 0; s < DEFLATE_NDIST; s++) {
            if (!w.dfreq[s]) continue;
            bits += w.dfreq[s] * (w.dlens[s] + (s < 4 ? 0u : (uint32_t)(s / 2 - 1)));
            hdist = s + 1;
        }
        deflate_codes(w.dlens, DEFLATE_NDIST, w.count, w.next, w.dfreq);
        for (int s = 0; s < hdist; s++) w.lens[hlit + s] = w.dlens[s];
    }
    w.data_bits = bits;
    w.hlit = (uint32_t)hlit;
    w.hdist = (uint32_t)hdist;
    const int n_lens = hlit + hdist;
    // the code-length sequence
    for (int s = 0; s < 19; s++) w.clfreq[s] = 0;
    uint32_t n_seq = 0;
    auto put = [&](uint32_t s, uint32_t extra) { w.seq[n_seq++] = (uint16_t)(s | extra << 8); w.clfreq[s]++; };
    for (int i = 0; i < n_lens;) {
        const uint32_t v = w.lens[i];
        int r = 1;
        while (i + r < n_lens && w.lens[i + r] == v) r++;
        i += r;
        if (v == 0) {
            while (r >= 11) { const int t = r < 138 ? r : 138; put(18, (uint32_t)(t - 11)); r -= t; }
            if (r >= 3) { put(17, (uint32_t)(r - 3)); r = 0; }
        } else {
            put(v, 0); r--;
            while (r >= 3) { const int t = r < 6 ? r : 6; put(16, (uint32_t)(t - 3)); r -= t; }
        }
        for (; r > 0; r--) put(v, 0);
    }
    w.n_seq = n_seq;
    for (int s = 0; s < 20; s++) w.cllens[s] = 0;
    const int mc = deflate_sort(w.clfreq, 19, w.a, w.sym);
    deflate_lengths_sorted(w.a, w.sym, mc, 7, w.count, w.cllens);
    deflate_codes(w.cllens, 19, w.count, w.next, w.clcode);
    uint32_t hclen = 4;
    for (int k = 4; k < 19; k++)
        if (w.cllens[deflate_cl_order(k)]) hclen = (uint32_t)k + 1;
    w.hclen = hclen;
    uint32_t hb = 17 + 3 * hclen;
    for (int s = 0; s < 19; s++) hb += w.clfreq[s] * (w.cllens[s] + deflate_cl_extra_bits((uint32_t)s));
    w.hdr_bits = hb;
}

// bytes of the block; a member is written stored when this is >= payload + 5
NPORE_DFL_HD uint32_t deflate_block_bytes(const DeflateWork &w) { return (w.hdr_bits + w.data_bits + 7) >> 3; }

// an LSB-first bit stream into bytes
struct DeflateBits {
    uint8_t *o;
    uint64_t acc = 0;
    uint32_t n = 0;
    NPORE_DFL_HD explicit DeflateBits(uint8_t *out) : o(out) {}
    NPORE_DFL_HD void put(uint32_t v, uint32_t bits)          // bits <= 16
    {
        acc |= (uint64_t)v << n;
        n += bits;
        while (n >= 8) { *o++ = (uint8_t)acc; acc >>= 8; n -= 8; }
    }
    NPORE_DFL_HD void code(uint32_t c) { put(c & 0xFFFFu, c >> 16); }
};

// the block header's bits (w.hdr_bits of them) from the stream's first bit on; the last byte's upper bits are 0.
// hdr: DEFLATE_HDR_CAP bytes.
NPORE_DFL_HD void deflate_header(const DeflateWork &w, uint8_t *hdr)
{
    DeflateBits b(hdr);
    b.put(1, 1);                       // BFINAL
    b.put(2, 2);                       // BTYPE: dynamic
    b.put(w.hlit - 257, 5);            // HLIT (literals only: 257)
    b.put(w.hdist - 1, 5);             // HDIST (literals only: 1)
    b.put(w.hclen - 4, 4);
    for (uint32_t k = 0; k < w.hclen; k++) b.put(w.cllens[deflate_cl_order((int)k)], 3);
    for (uint32_t k = 0; k < w.n_seq; k++) {
        const uint32_t s = w.seq[k] & 0xFFu, extra = w.seq[k] >> 8;
        b.code(w.clcode[s]);
        if (s >= 16) b.put(extra, deflate_cl_extra_bits(s));
    }
    if (b.n) *b.o = (uint8_t)b.acc;
}

// byte k < 16 of a BGZF member: 1f 8b 08 04 | mtime 0 | xfl 0, os ff | xlen 6 | 'B' 'C' 2 0 (BSIZE follows)
NPORE_DFL_HD uint8_t bgzf_header_byte(int k)
{
    return (uint8_t)((k < 8 ? 0x0000000004088b1full : 0x000243420006ff00ull) >> (8 * (k & 7)));
}
NPORE_DFL_HD void bgzf_member_header(uint8_t *h, uint32_t member_bytes)
{
    for (int k = 0; k < 16; k++) h[k] = bgzf_header_byte(k);
    h[16] = (uint8_t)((member_bytes - 1) & 0xFF);
    h[17] = (uint8_t)((member_bytes - 1) >> 8);
}

// Steps 1 to 4 of the match rule on the host: the tokens of in[0 .. n) -- length << 16 | distance, or the literal -- into
// tok (room for n); head: 2^15 entries of scratch.  Returns how many there are.
inline size_t deflate_tokens_host(const uint8_t *in, size_t n, uint32_t *tok, uint16_t *head)
{
    for (size_t h = 0; h < ((size_t)1 << DEFLATE_HASH_BITS); h++) head[h] = (uint16_t)DEFLATE_NO_POS;
    size_t n_tok = 0, at = 0;                                   // at: where the parse stands
    for (size_t i = 0; i < n; i++) {
        uint32_t len = 0, dist = 0;
        if (i + 4 <= n) {                                       // every position enters the table, parsed or skipped
            const uint32_t word = (uint32_t)in[i] | (uint32_t)in[i + 1] << 8 | (uint32_t)in[i + 2] << 16 | (uint32_t)in[i + 3] << 24;
            const uint32_t h = deflate_hash(word), c = head[h];
            head[h] = (uint16_t)i;
            if (i == at && c != DEFLATE_NO_POS && i - c <= (size_t)DEFLATE_MAX_DIST) {
                const size_t cap = n - i < (size_t)DEFLATE_MAX_MATCH ? n - i : (size_t)DEFLATE_MAX_MATCH;
                while (len < cap && in[c + len] == in[i + len]) len++;
                dist = (uint32_t)(i - c);
            }
        }
        if (i != at) continue;
        if (len >= (uint32_t)DEFLATE_MIN_MATCH) { tok[n_tok++] = len << 16 | dist; at = i + len; }
        else { tok[n_tok++] = in[i]; at = i + 1; }
    }
    return n_tok;
}

// The host twin: the member of in[0 .. n), n <= 65 280, into out (room for n + 31 bytes); returns its size.  crc: the
// payload's CRC-32.  mode: DEFLATE_MODE_HUFFMAN, literals only, or DEFLATE_MODE_MATCH.
inline size_t deflate_member_host(const uint8_t *in, size_t n, uint32_t crc, uint8_t *out, int mode = DEFLATE_MODE_HUFFMAN)
{
    auto trailer = [&](uint8_t *t) {
        for (int k = 0; k < 4; k++) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
    };
    DeflateWork w;
    uint32_t block = 0;
    if (n > 0) {
        for (int s = 0; s < DEFLATE_NSYM; s++) w.freq[s] = 0;
        for (size_t k = 0; k < n; k++) w.freq[in[k]]++;
        w.freq[256] = 1;
        deflate_plan_sorted(w, deflate_sort(w.freq, DEFLATE_NSYM, w.a, w.sym));
        block = deflate_block_bytes(w);
    }
    if (n > 0 && mode == DEFLATE_MODE_MATCH) {                  // step 6: the match block only where it is the smallest
        std::vector<uint32_t> tok(n);
        std::vector<uint16_t> head((size_t)1 << DEFLATE_HASH_BITS);
        const size_t n_tok = deflate_tokens_host(in, n, tok.data(), head.data());
        DeflateWork wm;
        for (int s = 0; s < DEFLATE_NLL; s++) wm.freq[s] = 0;
        for (int s = 0; s < DEFLATE_NDIST; s++) wm.dfreq[s] = 0;
        for (size_t k = 0; k < n_tok; k++) {
            if (tok[k] >> 16) { wm.freq[deflate_len_symbol(tok[k] >> 16) & 0xFFFFu]++; wm.dfreq[deflate_dist_symbol(tok[k] & 0xFFFFu) & 0xFFu]++; }
            else wm.freq[tok[k]]++;
        }
        wm.freq[256] = 1;
        deflate_plan_sorted(wm, deflate_sort(wm.freq, DEFLATE_NLL, wm.a, wm.sym), true);
        const uint32_t mblock = deflate_block_bytes(wm);
        if (mblock < block && mblock < n + 5) {
            bgzf_member_header(out, mblock + 26);
            uint8_t hdr[DEFLATE_HDR_CAP];
            deflate_header(wm, hdr);
            const uint32_t hb = wm.hdr_bits >> 3;
            for (uint32_t k = 0; k < hb; k++) out[18 + k] = hdr[k];
            DeflateBits b(out + 18 + hb);
            if (wm.hdr_bits & 7) b.put(hdr[hb], wm.hdr_bits & 7);
            for (size_t k = 0; k < n_tok; k++) {
                if (!(tok[k] >> 16)) { b.code(wm.freq[tok[k]]); continue; }
                const uint32_t ls = deflate_len_symbol(tok[k] >> 16), ds = deflate_dist_symbol(tok[k] & 0xFFFFu);
                b.code(wm.freq[ls & 0xFFFFu]);
                b.put(ls >> 24, (ls >> 16) & 0xFFu);
                b.code(wm.dfreq[ds & 0xFFu]);
                b.put(ds >> 16, (ds >> 8) & 0xFFu);
            }
            b.code(wm.freq[256]);
            if (b.n) *b.o = (uint8_t)b.acc;
            trailer(out + 18 + mblock);
            return (size_t)mblock + 26;
        }
    }
    if (n == 0 || block >= n + 5) {
        bgzf_member_header(out, (uint32_t)n + 31);
        out[18] = 1;
        out[19] = (uint8_t)(n & 0xFF); out[20] = (uint8_t)(n >> 8);
        out[21] = (uint8_t)(~n & 0xFF); out[22] = (uint8_t)((~n >> 8) & 0xFF);
        for (size_t k = 0; k < n; k++) out[23 + k] = in[k];
        trailer(out + 23 + n);
        return n + 31;
    }
    bgzf_member_header(out, block + 26);
    uint8_t hdr[DEFLATE_HDR_CAP];
    deflate_header(w, hdr);
    const uint32_t hb = w.hdr_bits >> 3;
    for (uint32_t k = 0; k < hb; k++) out[18 + k] = hdr[k];
    DeflateBits b(out + 18 + hb);
    if (w.hdr_bits & 7) b.put(hdr[hb], w.hdr_bits & 7);
    for (size_t k = 0; k < n; k++) b.code(w.freq[in[k]]);
    b.code(w.freq[256]);
    if (b.n) *b.o = (uint8_t)b.acc;
    trailer(out + 18 + block);
    return (size_t)block + 26;
}

}  // namespace npore
