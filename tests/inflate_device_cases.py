"""Shared cases of the wave-per-stream DEFLATE decoder (csrc/inflate_wave.hpp): test_inflate_wave.py runs them through the
host twin, test_gpu_inflate_device.py through the gfx950 kernel.  No tests here.  The yardstick is zlib.decompressobj(-15).

A case is (name, raw, out_len, want): the raw DEFLATE stream, the size its output must have, and the bytes (None: the
stream is malformed for that size and must get status 0; FUZZ: whatever zlib says).  A launch places cases in one input and
one output buffer: inputs at odd offsets, outputs back to back (guard = 0) or with 32 bytes of 0xA5 around each (guard = 32).

Where zlib's compressor does not go: BitWriter writes any block type from explicit code lengths, hand_built_cases() states
the edges of the format with it (codes of 15 bits, one or no distance code, the header's limits, repeats, the code-length
code, the last bit of a stream, hundreds of blocks), mutant_cases() flips every bit of the head of six small streams and
gives each mutant the size zlib inflates it to, and mixed_members() / damaged_files() cut a BAM's stream into BGZF members
of every kind for the readers.
"""
import functools
import os
import struct
import zlib

import numpy as np

from npore_amd import _lib
from test_bam_deflate import KINDS, content

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUZZ = "fuzz"
GUARD = 32
FILL = 0xA5
LEVELS = (0, 1, 6, 9)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY)
DISTANCES = (1, 2, 3, 7, 8, 63, 64, 65, 255, 256, 4097, 32768)
LENGTHS = (3, 4, 10, 11, 63, 64, 65, 257, 258)


def deflate(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def zlib_inflate(raw, out_len):
    """The out_len bytes of the stream, or None where zlib refuses it or it has another size."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw, out_len + 1)
    except zlib.error:
        return None
    return out if d.eof and len(out) == out_len else None


# ---- hand-written fixed-Huffman streams: the sequence of literals and matches is exact
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class FixedWriter:
    """Bits LSB first; Huffman codes MSB first (RFC 1951 3.1.1); one fixed-Huffman block unless told otherwise."""

    def __init__(self, final=1, btype=1):
        self.acc, self.n, self.out, self.made = 0, 0, bytearray(), bytearray()
        self.bits(final, 1)
        self.bits(btype, 2)

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.bits(int(format(v, "0%db" % n)[::-1], 2), n)

    def symbol(self, s):
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xC0 + s - 280, 8)

    def literals(self, data):
        for b in data:
            self.symbol(b)
        self.made += data

    def match(self, length, dist, track=True):
        k = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < 258))
        self.symbol(257 + k)
        self.bits(length - LEN_BASE[k], LEN_EXTRA[k])
        j = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.code(j, 5)
        self.bits(dist - DIST_BASE[j], DIST_EXTRA[j])
        if track:
            for _ in range(length):
                self.made.append(self.made[-dist])

    def end(self):
        self.symbol(256)
        return bytes(self.out + (bytes([self.acc]) if self.n else b""))


def _literals(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


# ---- a writer for any block type: stored, fixed, dynamic from explicit code lengths; several blocks in one stream
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_EXTRA = {16: 2, 17: 3, 18: 7}
CL_ALL = [4] * 13 + [5] * 6                                          # a complete code over all 19 symbols: 13 / 16 + 6 / 32


def canonical_codes(lengths):
    """{symbol: (code, bits)} of the code lengths, RFC 1951 3.2.2 (the codes of an over-subscribed set are cut to their bits)"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, first = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        first[b] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (first[n] & ((1 << n) - 1), n)
            first[n] += 1
    return out


def flat_lens(symbols, n):
    """n code lengths: a complete code over the (two or more) symbols, each of k - 1 or k bits"""
    symbols = sorted(set(symbols))
    k = (len(symbols) - 1).bit_length()
    short = (1 << k) - len(symbols)
    lens = [0] * n
    for j, s in enumerate(symbols):
        lens[s] = k - 1 if j < short else k
    return lens


def plain_items(lens):
    return [(n, 0) for n in lens]


def run_items(lens):
    """the lengths with their runs of zeros as repeats 17 and 18, as a compressor would send them"""
    items, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == 0:
            j += 1
        run = j - i
        while run >= 3:
            take = min(run, 138)
            items.append((18, take - 11) if take >= 11 else (17, take - 3))
            run -= take
            i += take
        if i < len(lens):
            items.append((lens[i], 0))
            i += 1
    return items


def expand_items(items):
    """the code lengths a valid item list [(code-length symbol, value of its extra bits)] stands for"""
    lens = []
    for s, x in items:
        assert 0 <= x < (1 << CL_EXTRA.get(s, 0))
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + x)
        else:
            lens += [0] * ((3 if s == 17 else 11) + x)
    return lens


class BitWriter(FixedWriter):
    """A stream block by block: stored(), fixed() or dynamic(), then literals() / match() / symbol() / raw codes, eob();
    done() gives the stream.  `made` follows what the stream must inflate to (tracked calls only)."""

    def __init__(self):
        self.acc, self.n, self.out, self.made = 0, 0, bytearray(), bytearray()
        self.lit, self.dist, self.headers_at = {}, {}, []

    def position(self):
        return 8 * len(self.out) + self.n

    def stored(self, data, final=0, nlen=None):
        self.headers_at.append(self.position())
        self.bits(final, 1)
        self.bits(0, 2)
        self.bits(0, -self.n % 8)
        self.out += struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data
        self.made += data

    def fixed(self, final=1):
        self.headers_at.append(self.position())
        self.bits(final, 1)
        self.bits(1, 2)
        self.lit, self.dist = canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST)

    def dynamic(self, lit_lens=None, dist_lens=None, final=1, cl_lens=None, hclen=None, items=None, hlit=None, hdist=None):
        """lit_lens / dist_lens: the codes of the block's symbols (None: what `items` expands to, cut at hlit); items: how
        the lengths are sent (None: one by one); cl_lens / hclen: the code-length code (None: CL_ALL, as many as needed);
        hlit / hdist: the counts the header announces (None: those of the lists)"""
        if items is None:
            items = plain_items(list(lit_lens) + list(dist_lens))
        if lit_lens is None:
            lens = expand_items(items)
            lit_lens, dist_lens = lens[:hlit], lens[hlit:]
        hlit = len(lit_lens) if hlit is None else hlit
        hdist = len(dist_lens) if hdist is None else hdist
        cl_lens = CL_ALL if cl_lens is None else cl_lens
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
        self.headers_at.append(self.position())
        self.bits(final, 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CL_ORDER[i]], 3)
        cl = canonical_codes(cl_lens)
        for s, x in items:
            self.code(*cl[s])
            self.bits(x, CL_EXTRA.get(s, 0))
        self.lit, self.dist = canonical_codes(lit_lens), canonical_codes(dist_lens)

    def symbol(self, s):
        self.code(*self.lit[s])

    def dist_symbol(self, s):
        self.code(*self.dist[s])

    def match(self, length, dist, track=True, len_symbol=None):
        k = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < 258)) if len_symbol is None else len_symbol - 257
        assert 0 <= length - LEN_BASE[k] < (1 << LEN_EXTRA[k])
        self.symbol(257 + k)
        self.bits(length - LEN_BASE[k], LEN_EXTRA[k])
        j = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.dist_symbol(j)
        self.bits(dist - DIST_BASE[j], DIST_EXTRA[j])
        if track:
            for _ in range(length):
                self.made.append(self.made[-dist])

    def eob(self):
        self.symbol(256)

    def done(self):
        return bytes(self.out + (bytes([self.acc]) if self.n else b""))

    def end(self):
        self.eob()
        return self.done()


def _same_as_fixed_writer():
    """the streams of fixed_cases() come out of BitWriter byte for byte"""
    for d, length in ((1, 3), (7, 258), (4097, 65), (32768, 257)):
        a, b = FixedWriter(), BitWriter()
        b.fixed()
        for w in (a, b):
            w.literals(_literals(d, d * 1000 + length))
            w.match(length, d)
            w.literals(b"Z")
            w.match(3, 1)
            w.match(min(length, 258), min(d, 2))
        assert a.end() == b.end() and a.made == b.made, (d, length)


_same_as_fixed_writer()


def zlib_refusal(raw):
    """zlib's words for refusing the stream (None: it does not refuse it, though it may want more input)"""
    try:
        zlib.decompressobj(-15).decompress(raw, IW_MAX_OUT + 2)
    except zlib.error as e:
        return str(e)
    return None


IW_MAX_OUT = 65536
LETTERS15 = tuple(sorted(b"ACGTNacgtn#$%&*"))
LONG_LENS = list(range(1, 15)) + [15, 15]                            # complete: 1/2 + ... + 2^-14 + 2 * 2^-15 = 1


def long_literal_lens(low_long):
    """literal / length code lengths 1, 2, ... 14, 15, 15 over LETTERS15 and 256 (low_long: the long codes on the low symbols)"""
    lens = [0] * 257
    for s, n in zip(LETTERS15 + (256,), LONG_LENS[::-1] if low_long else LONG_LENS):
        lens[s] = n
    return lens


def _letters(n, seed, letters=LETTERS15):
    """every letter three times, then n random ones"""
    rng = np.random.default_rng(seed)
    return bytes(letters) * 3 + bytes(rng.choice(np.array(letters, np.uint8), n))


def long_literal_stream(low_long, items=plain_items, n=400):
    w = BitWriter()
    lens = long_literal_lens(low_long)
    w.dynamic(lens, [0], items=items(lens + [0]))
    w.literals(_letters(n, 31 + low_long))
    return w


def one_distance_stream(sym, items=plain_items):
    """a block whose only distance code is one bit for distance symbol `sym`, with matches through it"""
    w = BitWriter()
    if DIST_BASE[sym] > 300:                                         # the bytes such a distance reaches back over
        w.fixed(final=0)
        w.literals(_literals(97, sym))
        while len(w.made) < DIST_BASE[sym] + 100:
            w.match(258, 97)
        w.eob()
    lit, dist = flat_lens(list(b"pqrstuvw") + [256, 257, 260, 285], 286), [0] * sym + [1]
    w.dynamic(lit, dist, items=items(lit + dist))
    w.literals(_letters(80, sym, tuple(b"pqrstuvw")))
    lo, hi = DIST_BASE[sym], min(DIST_BASE[sym] + (1 << DIST_EXTRA[sym]) - 1, len(w.made))
    for length, d in ((3, lo), (258, hi), (6, lo), (3, hi)):
        w.match(length, d)
        w.literals(b"q")
    w.eob()
    return w


def lone_eob_payload(data):
    """An empty non-final dynamic block whose literal / length code is the end-of-block code alone (one bit), then the
    data in a stored block: legal (zlib takes it), one of the oddities the decoders here may decline"""
    w = BitWriter()
    w.dynamic([0] * 256 + [1], [0], final=0, items=run_items([0] * 256 + [1, 0]))
    w.eob()
    w.stored(data, final=1)
    return w.done()


@functools.lru_cache(None)
def hand_built_cases():
    """Streams zlib's compressor never writes, each stated symbol by symbol; a malformed one is named "bad: ..." and is
    checked to be refused by zlib for the reason it was built for."""
    cases = []

    def add(name, w, why=False, raw=None, n=None):
        """why: False = valid; else the stream is malformed, and zlib's words contain `why` (None: it only runs short)"""
        raw = w.done() if raw is None else raw
        n = len(w.made) if n is None else n
        if why is False:
            want = bytes(w.made)
            assert zlib_inflate(raw, n) == want, name
            cases.append((name, raw, n, want))
        else:
            said = zlib_refusal(raw)
            assert zlib_inflate(raw, n) is None and (said is None if why is None else said is not None and why in said), (name, said)
            cases.append(("bad: " + name, raw, n, None))

    def body(w, text=b"lit-only body"):
        w.literals(text)
        w.eob()
        return w

    # -- long codes: beyond the primary tables (10 bits literal / length, 8 bits distance)
    for low_long in (0, 1):
        w = long_literal_stream(low_long)
        w.eob()
        add("literal codes of 1 to 15 bits" + (", long ones low" if low_long else ""), w)
    far_lit = flat_lens(list(b"abcdefghijklmnop") + [256, 257, 285], 286)
    for which in ("smallest", "largest"):
        w = BitWriter()
        w.dynamic(far_lit, LONG_LENS)
        w.literals(_letters(260, 41, tuple(b"abcdefghijklmnop")))
        for j in range(16):
            d = DIST_BASE[j] if which == "smallest" else DIST_BASE[j] + (1 << DIST_EXTRA[j]) - 1
            for length in (3, 258):
                w.match(length, d)
                w.literals(bytes([97 + (j + length) % 16]))
        w.eob()
        add("distance codes of 1 to 15 bits, %s distances" % which, w)
    # -- one distance code of one bit; no distance code
    for sym in (0, 11, 29):
        add("one distance code, symbol %d" % sym, one_distance_stream(sym))
    few = flat_lens(list(b"xyz") + [256, 257], 258)
    w = BitWriter()
    w.dynamic(few, [1])
    w.literals(b"xyzzy")
    w.symbol(257)
    w.code(1, 1)                                                    # the 1-bit code that has no symbol
    w.eob()
    add("the unassigned 1-bit distance code", w, "invalid distance code", n=8)
    for name, dist in (("one distance code of 2 bits", [2]), ("two distance codes of 2 bits", [2, 2]), ("three 1-bit distance codes", [1, 1, 1])):
        w = BitWriter()
        w.dynamic(few, dist)
        add(name, body(w, b"xyzzy"), "invalid distances set")
    w = BitWriter()
    w.dynamic(few, [0])
    add("no distance code, literals only", body(w, b"xyzzy" * 40))
    w = BitWriter()
    w.dynamic(few, [0])
    w.literals(b"xyzzy")
    w.symbol(257)
    w.bits(0, 5)
    w.eob()
    add("a length symbol without any distance code", w, "invalid distance code", n=8)
    # -- a literal / length code of a single symbol
    data = _letters(200, 43)
    raw = lone_eob_payload(data)
    assert zlib_inflate(raw, len(data)) == data
    cases.append(("lone end-of-block code, then stored", raw, len(data), data))
    w = BitWriter()
    w.dynamic(flat_lens(b"wxyz", 257), [0])
    w.literals(b"xyzzy")
    add("a literal set without 256", w, "missing end-of-block")
    # -- header limits
    w = BitWriter()
    w.fixed(final=0)
    w.literals(_literals(128, 47))
    for _ in range(127):
        w.match(258, 128)
    w.eob()
    assert len(w.made) >= 32768
    w.dynamic(flat_lens(list(b"hijklmno") + [256, 284, 285], 286), flat_lens([28, 29], 30))
    w.literals(b"limno")
    for length, d, s in ((258, 16385, None), (258, 24577, 284), (227, 32768, None), (258, 24576, 284), (257, 32768, None), (258, 32768, None)):
        w.match(length, d, len_symbol=s)
        w.literals(b"k")
    w.eob()
    add("HLIT 286 and HDIST 30, 258 as 285 and as 284 + 31", w)
    for hlit, hdist in ((287, 2), (288, 2), (257, 31), (257, 32)):
        w = BitWriter()
        w.dynamic(flat_lens(list(b"xyz") + [256], hlit), flat_lens([0, 1], hdist))
        add("HLIT %d, HDIST %d" % (hlit, hdist), body(w, b"xyzzy"), "too many length or distance symbols")
    for s in (286, 287):
        w = BitWriter()
        w.fixed()
        w.literals(b"abc")
        w.symbol(s)
        w.bits(0, 5)
        w.eob()
        add("fixed block, literal/length symbol %d" % s, w, "invalid literal/length code", n=6)
    for s in (30, 31):
        w = BitWriter()
        w.fixed()
        w.literals(b"abc")
        w.symbol(257)
        w.dist_symbol(s)
        w.eob()
        add("fixed block, distance symbol %d" % s, w, "invalid distance code", n=6)
    # -- repeats in the code lengths
    lens = flat_lens([138, 139, 140, 256], 257) + [0]
    w = BitWriter()
    w.dynamic(items=[(18, 127)] + plain_items(lens[138:]), hlit=257)
    assert w.lit == canonical_codes(lens[:257])
    add("repeat 18 with 138 zeros", body(w, bytes([138, 139, 140, 139] * 30)))
    lens = [0] * 255 + [2]                                          # 255, 256, 257 and the four distance codes: 2 bits, by one repeat
    lens[65] = lens[66] = 3
    w = BitWriter()
    w.dynamic(items=plain_items(lens) + [(16, 3)], hlit=258)
    assert len(w.lit) == 5 and w.dist == canonical_codes([2, 2, 2, 2])
    w.literals(bytes([65, 66, 255, 66, 65]))
    for d in (1, 2, 3, 4, 2):
        w.match(3, d)
        w.literals(bytes([255]))
    w.eob()
    add("repeat 16 across the literal / distance boundary", w)
    w = BitWriter()                                                 # 0: 2 bits | 17: three zeros | 16: three more | 7, 8: 2 bits | zeros | 256: 2 bits | no distance code
    w.dynamic(items=[(2, 0), (17, 0), (16, 0), (2, 0), (2, 0), (18, 127), (18, 98), (2, 0), (0, 0)], hlit=257)
    assert sorted(w.lit) == [0, 7, 8, 256]
    add("repeat 16 directly after a 17", body(w, bytes([0, 7, 8, 8, 7, 0] * 20)))
    lens = flat_lens(list(b"xyz") + [256], 257) + [0]
    w = BitWriter()
    w.dynamic(lens[:257], lens[257:], items=[(16, 0)] + plain_items(lens[3:]))
    add("repeat 16 as the first item", body(w, b"xyzzy"), "invalid bit length repeat")
    w = BitWriter()
    w.dynamic(lens[:257], lens[257:], items=plain_items(lens[:250]) + [(18, 127)])
    add("a repeat past HLIT + HDIST", body(w, b"xyzzy"), "invalid bit length repeat")
    # -- the code-length code
    lens = long_literal_lens(0)
    w = BitWriter()
    w.dynamic(lens, [0], cl_lens=[4] * 16 + [0] * 3)
    add("HCLEN 19, sixteen 4-bit code-length codes", body(w, _letters(300, 53)))
    lens = flat_lens(list(b"xyz") + [256], 257)
    w = BitWriter()
    w.dynamic(lens, [0], cl_lens=[0] * 19, hclen=4, items=[])
    w.bits(0, 8 * 48)
    add("HCLEN 4, every code-length code absent", w, "missing end-of-block", n=5)
    for name, cl in (("a single 1-bit code-length code", [1] + [0] * 18), ("three 1-bit code-length codes", [1, 1, 1] + [0] * 16)):
        w = BitWriter()
        w.dynamic(lens, [0], cl_lens=cl, items=[(0, 0)] * 258)
        w.bits(0, 64)
        add(name, w, "invalid code lengths set", n=5)
    for name, n in (("three 2-bit literal codes (incomplete)", 2), ("three 1-bit literal codes (over-subscribed)", 1)):
        bad = [0] * 257
        bad[120] = bad[121] = bad[256] = n
        w = BitWriter()
        w.dynamic(bad, [0])
        add(name, body(w, b"xyyx"), "invalid literal/lengths set")
    # -- the end of the stream, bit by bit: a 9-bit literal more moves the last bit of the end-of-block code by one
    ends = set()
    for k in range(8):
        w = BitWriter()
        w.fixed()
        w.literals(b"end" + bytes(range(200, 200 + k)))
        w.eob()
        ends.add(w.position() % 8)
        add("the last code ends at bit %d" % (w.position() % 8), w)
        add("the last code ends at bit %d, last byte cut off" % (w.position() % 8), w, None, raw=w.done()[:-1])
        add("the last code ends at bit %d, a zero byte behind" % (w.position() % 8), w, raw=w.done() + b"\0")
    assert len(ends) == 8
    # -- many blocks
    w = BitWriter()
    for _ in range(300):
        w.fixed(final=0)
        w.eob()
    w.fixed()
    add("300 empty fixed blocks, then three literals", body(w, b"abc"))
    w = BitWriter()
    for k in range(201):
        w.stored(b"", final=int(k == 200))
    add("201 empty stored blocks", w)
    w = BitWriter()
    rng = np.random.default_rng(59)
    for k in range(40):
        w.fixed(final=0)
        w.literals(b"round %2d " % k + bytes(range(150, 150 + k % 8)))      # (k % 8 literals of 9 bits: the next header's bit offset)
        w.match(3 + k, 4 + k % 5)
        w.eob()
        w.stored(bytes(rng.integers(0, 256, 61 + 13 * k, dtype=np.uint8)))
    lens = long_literal_lens(1)
    w.dynamic(lens, [0], items=run_items(lens + [0]))
    w.literals(_letters(100, 61))
    w.eob()
    assert len(w.headers_at) == 81 and {p % 8 for p in w.headers_at[1:80:2]} == set(range(8))      # (the stored blocks' headers)
    add("40 rounds of fixed and stored blocks, then a dynamic one", w)
    w = BitWriter()
    w.stored(_literals(65535, 67))
    w.stored(b"!", final=1)
    add("stored blocks of 65535 bytes and 1 byte", w)
    return tuple(cases)


def oversize_case():
    """an out_len beyond a BGZF member's 65 536 bytes: refused for its size alone, nothing written"""
    raw = next(c[1] for c in hand_built_cases() if c[0] == "stored blocks of 65535 bytes and 1 byte")
    assert zlib_inflate(raw, IW_MAX_OUT + 1) is None
    return ("bad: out_len 65537", raw, IW_MAX_OUT + 1, None)


def fixed_cases():
    cases = []
    for d in DISTANCES:
        for length in LENGTHS:
            # d exactly the number of bytes produced so far; then a literal, and a match over what the first one wrote
            w = FixedWriter()
            w.literals(_literals(d, d * 1000 + length))
            w.match(length, d)
            w.literals(b"Z")
            w.match(3, 1)
            w.match(min(length, 258), min(d, 2))
            raw, want = w.end(), bytes(w.made)
            assert zlib_inflate(raw, len(want)) == want
            cases.append(("fixed d=%d len=%d" % (d, length), raw, len(want), want))
        # more in front of the match than it reaches back
        w = FixedWriter()
        w.literals(_literals(d + 7, d))
        w.match(258, d)
        raw, want = w.end(), bytes(w.made)
        assert zlib_inflate(raw, len(want)) == want
        cases.append(("fixed d=%d after %d" % (d, d + 7), raw, len(want), want))
        # the malformed twins
        if d < 32768:
            w = FixedWriter()                                       # one further back than there are bytes
            w.literals(_literals(d, d))
            w.match(10, d + 1, track=False)
            cases.append(("bad: d=%d with %d bytes" % (d + 1, d), w.end(), d + 10, None))
        w = FixedWriter()                                           # a match running past out_len
        w.literals(_literals(d, d))
        w.match(10, d)
        raw = w.end()
        cases.append(("bad: match past out_len, d=%d" % d, raw, d + 9, None))
        cases.append(("bad: ends at out_len - 1, d=%d" % d, raw, d + 11, None))
    w = FixedWriter(btype=0)                                        # a stored block whose LEN / NLEN disagree
    w.bits(0, 5)
    w.out += bytes([4, 0, 0xFA, 0xFF]) + b"ABCD"
    cases.append(("bad: stored LEN/NLEN", bytes(w.out), 4, None))
    good = bytes([1, 4, 0, 0xFB, 0xFF]) + b"ABCD"
    assert zlib_inflate(good, 4) == b"ABCD"
    cases.append(("stored, by hand", good, 4, b"ABCD"))
    w = FixedWriter(btype=3)
    w.literals(b"AB")
    cases.append(("bad: block type 3", w.end(), 2, None))
    for name, raw, n, want in cases:
        assert want is not None or zlib_inflate(raw, n) is None, name
    return cases


def golden_bam_blocks():
    raw = open(os.path.join(GOLDEN, "data", "reads.bam"), "rb").read()
    p, out = 0, []
    while p < len(raw):
        xlen = int.from_bytes(raw[p + 10:p + 12], "little")
        bsize = int.from_bytes(raw[p + 16:p + 18], "little") + 1
        isize = int.from_bytes(raw[p + bsize - 4:p + bsize], "little")
        out.append((raw[p + 12 + xlen:p + bsize - 8], isize))
        p += bsize
    return out


def host_datas():
    """The contents of test_host_logic.test_inflate_decoder_equals_zlib."""
    rng = np.random.default_rng(11)
    return [b"", b"A", b"ACGT" * 5000, bytes(rng.integers(0, 256, 60000, dtype=np.uint8)), bytes(rng.integers(0, 4, 65280, dtype=np.uint8)),
            b"\0" * 65280, bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 40000)) + bytes(rng.integers(33, 75, 25000, dtype=np.uint8)),
            bytes(np.repeat(rng.integers(0, 256, 300, dtype=np.uint8), rng.integers(1, 300, 300)))[:65000]]


@functools.lru_cache(None)
def valid_and_malformed_cases():
    cases = []
    datas = [("host%d" % i, d) for i, d in enumerate(host_datas())] + [(k, content(k, n)) for k in KINDS for n in (1021, 65280)]
    for name, data in datas:
        for level in LEVELS:
            for strat in STRATEGIES:
                cases.append(("%s level=%d strategy=%d" % (name, level, strat), deflate(data, level, strat), len(data), data))
    cases.append(("empty", deflate(b"", 6), 0, b""))
    cases.append(("BGZF EOF payload", bytes([3, 0]), 0, b""))
    rng = np.random.default_rng(5)
    for n in (1, 65535, 65536):
        data = bytes(rng.integers(0, 64, n, dtype=np.uint8))
        cases.append(("%d bytes" % n, deflate(data, 6), n, data))
    parts = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 9000)), bytes(rng.integers(33, 75, 7000, dtype=np.uint8)), b"tail" * 900]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(parts[0]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(parts[1]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(parts[2]) + c.flush()
    cases.append(("sync and full flush", raw, sum(map(len, parts)), b"".join(parts)))
    for i, (pay, isize) in enumerate(golden_bam_blocks()):
        cases.append(("reads.bam block %d" % i, pay, isize, zlib.decompress(pay, -15)))
    for name, raw, n, want in cases:
        assert zlib_inflate(raw, n) == want, name
    return tuple(cases + fixed_cases() + list(hand_built_cases()))


@functools.lru_cache(None)
def corrupt_cases():
    """200 mutations of one dynamic stream, as the host test makes them: 1 - 3 bit flips, every third one truncated."""
    rng = np.random.default_rng(11)
    data = host_datas()[6]
    base = deflate(data, 6)
    out = []
    for k in range(200):
        bad = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        if k % 3 == 0:
            bad = bad[:int(rng.integers(1, len(bad)))]
        out.append(("mutation %d" % k, bytes(bad), len(data), FUZZ))
    return tuple(out)


class Launch:
    """Cases placed in one input and one output buffer."""

    def __init__(self, name, cases, guard):
        self.name, self.cases, self.guard = name, list(cases), guard
        n = len(self.cases)
        self.in_off, self.in_len = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.out_off, self.out_len = np.zeros(n, np.int64), np.zeros(n, np.int64)
        ip, op, chunks = 1, guard, [b"\xee"]
        for k, (_, raw, size, _) in enumerate(self.cases):
            if ip % 2 == 0:                                         # every stream begins at an odd offset
                chunks.append(b"\xee")
                ip += 1
            self.in_off[k], self.in_len[k] = ip, len(raw)
            chunks.append(raw)
            ip += len(raw)
            self.out_off[k], self.out_len[k] = op, size
            op += size + guard
        self.inp = np.frombuffer(b"".join(chunks) + b"\xee", np.uint8).copy()
        self.out_bytes = max(op, 1)

    def fresh_out(self):
        return np.full(self.out_bytes, FILL, np.uint8)

    def piece(self, out, k):
        return out[self.out_off[k]:self.out_off[k] + self.out_len[k]].tobytes()

    def guards_intact(self, out):
        keep = np.ones(self.out_bytes, bool)
        for k in range(len(self.cases)):
            keep[self.out_off[k]:self.out_off[k] + self.out_len[k]] = False
        return bool((out[keep] == FILL).all())


def _pick(cases, n, seed):
    """n cases, the smaller ones, so that a launch of 257 stays a few megabytes"""
    small = [c for c in cases if c[2] <= 5000] or list(cases)
    idx = np.random.default_rng(seed).integers(0, len(small), n)
    return [small[i] for i in idx]


@functools.lru_cache(None)
def launches():
    cases = valid_and_malformed_cases()
    good = next(c for c in cases if c[0].startswith("host2 level=6"))
    out = []
    for guard in (0, GUARD):
        tag = "guard" if guard else "tight"
        out.append(Launch("all " + tag, cases, guard))
        for n in (1, 3, 5, 257):
            out.append(Launch("%d streams %s" % (n, tag), _pick(cases, n, n + guard) if n > 1 else [cases[n + guard]], guard))
    big = [c for c in cases if c[2] >= 60000]
    out.append(Launch("5 large tight", big[3:8], 0))
    return tuple(out)


@functools.lru_cache(None)
def corrupt_launches():
    good = next(c for c in valid_and_malformed_cases() if c[0].startswith("host2 level=6"))
    mixed = []
    for c in corrupt_cases():                                       # back to back with a good neighbour on either side
        mixed += [good, c]
    return (Launch("corrupt guard", corrupt_cases(), GUARD), Launch("corrupt tight", mixed + [good], 0))


def zlib_size(raw):
    """the size zlib inflates the stream to, or None where it refuses it, wants more input or gives more than a member's 65 536 bytes"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw, IW_MAX_OUT + 1)
    except zlib.error:
        return None
    return len(out) if d.eof and len(out) <= IW_MAX_OUT else None


MUTATED_BYTES = 96
OTHER_SIZE = 500


@functools.lru_cache(None)
def mutant_bases():
    rng = np.random.default_rng(23)
    reads = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 300)) + bytes(rng.integers(33, 75, 200, dtype=np.uint8))
    w = long_literal_stream(0, run_items, 600)
    w.eob()
    return (("level 6, bases and qualities", deflate(reads, 6)), ("level 9, repetitive", deflate(b"GATTACA-gattaca+" * 24, 9)),
            ("Z_FIXED, two-bit symbols", deflate(bytes(rng.integers(0, 4, 400, dtype=np.uint8)), 6, zlib.Z_FIXED)),
            ("level 0", deflate(bytes(rng.integers(0, 256, 100, dtype=np.uint8)), 0)),
            ("literal codes of 1 to 15 bits", w.done()), ("one distance code, symbol 11", one_distance_stream(11, run_items).done()))


@functools.lru_cache(None)
def mutant_cases():
    """Every single-bit flip of the first MUTATED_BYTES bytes of each base.  A mutant's out_len is the size zlib inflates it
    to (so that a stream zlib accepts is one the decoder must get right, not one it may refuse for its size), OTHER_SIZE
    where zlib does not; want: zlib's bytes, or None."""
    out = []
    for name, base in mutant_bases():
        assert zlib_size(base) is not None, name
        for bit in range(8 * min(len(base), MUTATED_BYTES)):
            raw = bytearray(base)
            raw[bit >> 3] ^= 1 << (bit & 7)
            raw = bytes(raw)
            n = zlib_size(raw)
            n = OTHER_SIZE if n is None else n
            out.append(("%s, bit %d" % (name, bit), raw, n, zlib_inflate(raw, n)))
    return tuple(out)


@functools.lru_cache(None)
def mutant_launches():
    return (Launch("mutants guard", mutant_cases(), GUARD), Launch("mutants tight", mutant_cases(), 0))


@functools.lru_cache(None)
def oversize_launch():
    """Not for the debug entries (they refuse such a table as a whole: test_inflate_wave.py); for the stand-alone program."""
    good = next(c for c in valid_and_malformed_cases() if c[0] == "stored, by hand")
    return Launch("oversize guard", [good, oversize_case(), good], GUARD)


# ---- BGZF files whose members are chosen by hand
EMPTY_PAYLOAD = bytes([3, 0])
LONE_KIND = "lone end-of-block"


def bgzf_member(payload, data, crc=None):
    """one BGZF member: the gzip header with the BC subfield, the payload, the CRC-32 (crc: another one) and ISIZE of the data"""
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(payload) + 25) + payload +
            struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data)))


def _sync_flushed(data):
    c, a, b = zlib.compressobj(6, zlib.DEFLATED, -15), len(data) // 3, 2 * len(data) // 3
    return c.compress(data[:a]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[a:b]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[b:]) + c.flush()


MEMBER_KINDS = (("level 9", lambda d: deflate(d, 9)), ("Z_FIXED", lambda d: deflate(d, 6, zlib.Z_FIXED)), ("level 0", lambda d: deflate(d, 0)),
                ("sync-flushed", _sync_flushed))


def mixed_members(stream, lo=3000, hi=8000, seed=71):
    """[(kind, payload, data)]: the stream cut into members of lo to hi bytes that rotate through MEMBER_KINDS, every fifth one
    lone_eob_payload; an empty member behind every seventh, two of them once, and the end-of-file member"""
    rng = np.random.default_rng(seed)
    out, p, k, turn = [], 0, 0, 0
    while p < len(stream):
        data = bytes(stream[p:p + int(rng.integers(lo, hi))])
        p += len(data)
        k += 1
        if k % 5 == 0:
            kind, payload = LONE_KIND, lone_eob_payload(data)
        else:
            kind, payload = MEMBER_KINDS[turn % 4][0], MEMBER_KINDS[turn % 4][1](data)
            turn += 1
        assert zlib_inflate(payload, len(data)) == data
        out.append((kind, payload, data))
        if k % 7 == 0:
            out += [("empty", EMPTY_PAYLOAD, b"")] * (2 if k == 14 else 1)
    return out + [("empty", EMPTY_PAYLOAD, b"")]


def member_bytes(members):
    return [bgzf_member(payload, data) for _, payload, data in members]


def damaged_files(members, first=17):
    """{what: (index, the file's members as bytes)}: ONE member changed, none of the `first` members an open call may read"""
    def pick(kind, ok=lambda payload: True):
        return next(i for i in range(first, len(members)) if members[i][0] == kind and ok(members[i][1]))

    def with_member(i, member):
        out = member_bytes(members)
        out[i] = member
        return i, out

    res = {}
    i = pick("Z_FIXED")
    res["crc"] = with_member(i, bgzf_member(members[i][1], members[i][2], zlib.crc32(members[i][2]) ^ 0x10))
    i = pick("level 0")                                             # (one stored block: 01 LEN NLEN, then the bytes)
    _, payload, data = members[i]
    bad = bytearray(payload)
    bad[5 + len(data) // 2] ^= 0x40
    assert zlib_inflate(bytes(bad), len(data)) not in (None, data)
    res["stored byte"] = with_member(i, bgzf_member(bytes(bad), data))
    i = pick("level 9", lambda payload: payload[0] >> 1 & 3 == 2)
    _, payload, data = members[i]
    for bit in range(3, 17 + 3 * 19):                               # HLIT, HDIST, HCLEN, the code-length code's lengths
        bad = bytearray(payload)
        bad[bit >> 3] ^= 1 << (bit & 7)
        if zlib_refusal(bytes(bad)) is not None:
            break
    assert zlib_refusal(bytes(bad)) is not None
    res["header bit"] = with_member(i, bgzf_member(bytes(bad), data))
    return res


def twin_declines(members):
    """how many of the non-empty members the host twin -- hence the device -- leaves to the host decoder"""
    launch = Launch("members", [(kind, payload, len(data), data) for kind, payload, data in members if data], 0)
    status, _ = _call(_lib.load().npore_debug_inflate_wave_host, launch)
    return int((status == 0).sum())


def _call(fn, launch, *head):
    out = launch.fresh_out()
    status = np.full(len(launch.cases), -7, np.int32)
    rc = fn(*head, launch.inp.ctypes.data, launch.inp.size, launch.in_off.ctypes.data, launch.in_len.ctypes.data, out.ctypes.data, out.size,
            launch.out_off.ctypes.data, launch.out_len.ctypes.data, len(launch.cases), status.ctypes.data)
    assert rc == 0, _lib.last_error()
    return status, out


@functools.lru_cache(None)
def twin(launch):
    """(status, out) of the host twin: computed once, shared by the CPU and the GPU tests, never changed."""
    status, out = _call(_lib.load().npore_debug_inflate_wave_host, launch)
    status.setflags(write=False)
    out.setflags(write=False)
    return status, out


def device(ctx, launch):
    return _call(_lib.load().npore_debug_inflate_device, launch, ctx.handle)


def dump_corpus(path):
    """Every launch as scripts/asan_inflate_wave.cpp reads it (the stand-alone sanitizer run of the host twin); expect: 1 zlib
    accepts and csrc/inflate.hpp takes the stream, 0 malformed, -1 either (fuzz, mutants, the oddities inflate.hpp declines)"""
    with open(path, "wb") as fh:
        for launch in launches() + corrupt_launches() + mutant_launches() + (oversize_launch(),):
            n = len(launch.cases)
            either = launch in mutant_launches()
            expect = np.array([-1 if either or c[3] is FUZZ else 0 if c[3] is None else -1 if not _host_takes(c) else 1 for c in launch.cases], np.int32)
            fh.write(b"IWL1" + np.array([n, launch.inp.size, launch.out_bytes], np.int64).tobytes())
            for a in (launch.in_off, launch.in_len, launch.out_off, launch.out_len):
                fh.write(a.tobytes())
            fh.write(expect.tobytes() + launch.inp.tobytes())


def _host_takes(case):
    src, out = np.frombuffer(case[1] + b"\0", np.uint8), np.zeros(case[2] + 1, np.uint8)
    return _lib.load().npore_debug_inflate(src.ctypes.data, len(case[1]), out.ctypes.data, case[2], 1) == 1


if __name__ == "__main__":
    import sys
    dump_corpus(sys.argv[1])
