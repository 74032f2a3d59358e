"""Shared cases of the wave-per-stream DEFLATE decoder (csrc/inflate_wave.hpp): test_inflate_wave.py runs them through the
host twin, test_gpu_inflate_device.py through the gfx950 kernel.  No tests here.  The yardstick is zlib.decompressobj(-15).

A case is (name, raw, out_len, want): the raw DEFLATE stream, the size its output must have, and the bytes (None: the
stream is malformed for that size and must get status 0; FUZZ: whatever zlib says).  A launch places cases in one input and
one output buffer: inputs at odd offsets, outputs back to back (guard = 0) or with 32 bytes of 0xA5 around each (guard = 32).
"""
import functools
import os
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
    return tuple(cases + fixed_cases())


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
    """Every launch as scripts/asan_inflate_wave.cpp reads it (the stand-alone sanitizer run of the host twin)."""
    with open(path, "wb") as fh:
        for launch in launches() + corrupt_launches():
            n = len(launch.cases)
            expect = np.array([-1 if c[3] is FUZZ else 0 if c[3] is None else -1 if not _host_takes(c) else 1 for c in launch.cases], np.int32)
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
