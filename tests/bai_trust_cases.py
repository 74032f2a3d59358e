"""Cases for the trust a one-pass handle puts in the .bai beside a BAM (tests/test_bai_trust.py on the CPU,
tests/test_gpu_bai_trust.py on the device): one small file, a family of indexes for it -- its own, stale ones, a
foreign one, linear-offset mutants of its own, malformed files -- and `expected`, the rule of npore_bam_set_share
stated in Python over the inflated stream.  Nothing here is taken from a run of the code under test.

THE RULE.  The .bai parses (every count bounded by the bytes left), its n_ref is the header's, and it has a non-zero
linear offset.  The cuts are those of csrc/bam_reader.hpp: for k = 1 .. world - 1 the first linear offset at or behind
(c0 + (c1 - c0) * k / world) << 16, c0 / c1 the first payload's begin and the last payload's end in the file; none left:
the end of the stream, for that cut and all behind it.  (1) EVERY non-zero linear offset of the index, a cut at this
world or not, names a BGZF member's first byte, exactly, and an offset inside what the member inflates to, behind the
header.  Every CUT must (2) be where a record starts: block_size >= 32 and the record whole within the stream, its
variable-length parts inside it and its name NUL-terminated, -1 <= refID < n_ref, 0 <= pos < the contig's length; (3) be
followed by another such record, or by the end of the stream.  One offset or cut that is not: refused, for every rank
(and, by (1), at every world: also at one whose own cuts happen to be good).  Otherwise rank r walks [cut r, cut r + 1)."""
import os
import struct
import zlib

import numpy as np

from npore_amd import bam

REFS = [("a", 300_000), ("b", 300_000)]
REFS3 = [("a", 300_000), ("b", 300_000), ("c", 300_000)]
REGIONS = [(0, 0, 300_000), (1, 0, 300_000)]
WORLDS = (2, 3, 5, 16)
REFUSE = "refuse"


def share_records():
    """400 records of 200 ... 900 bases on two contigs (300 + 100), sorted"""
    recs, pos = [], 0
    rng = np.random.default_rng(3)
    for k in range(400):
        n = int(rng.integers(200, 900))
        seq = "".join(rng.choice(list("ACGT"), n))
        recs.append(dict(name=f"r{k}", flag=0, ref_id=k // 300, pos=pos % 200_000, cigar=[(0, n)], seq=seq,
                         qual=bytes(rng.integers(0, 94, n, dtype=np.uint8)), hp=None))
        pos += int(rng.integers(100, 1200))
        if k == 299:
            pos = 0
    return recs


def share_test_bam(tmp_path):
    """The file of the share tests, level 1: about 17 linear offsets and several BGZF members.  Returns (BAM path, records)."""
    recs = share_records()
    path = str(tmp_path / "s.bam")
    bam.write_bam(path, REFS, recs, level=1)
    return path, recs


def three_contig_records(recs):
    """the same records on three contigs (200 + 100 + 100): one that lies between two others"""
    return [dict(r, ref_id=0 if k < 200 else 1 if k < 300 else 2) for k, r in enumerate(recs)]


class Stream:
    """A BGZF BAM's bytes taken apart: members [(offset in the file, payload offset, payload length, offset in the inflated
    stream, inflated length)], the inflated stream, the header's references and where every record starts."""

    def __init__(self, raw):
        self.raw, self.members, parts, p, u = raw, [], [], 0, 0
        while p < len(raw):
            xlen, = struct.unpack_from("<H", raw, p + 10)
            bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
            part = zlib.decompress(raw[p + 12 + xlen:p + bsize - 8], -15)
            self.members.append((p, p + 12 + xlen, bsize - 12 - xlen - 8, u, len(part)))
            parts.append(part)
            u += len(part)
            p += bsize
        self.data = d = b"".join(parts)
        l_text, = struct.unpack_from("<i", d, 4)
        q = 8 + l_text
        n_ref, = struct.unpack_from("<i", d, q)
        q += 4
        self.ref_lens = []
        for _ in range(n_ref):
            l_name, = struct.unpack_from("<i", d, q)
            self.ref_lens.append(struct.unpack_from("<i", d, q + 4 + l_name)[0])
            q += 8 + l_name
        self.first_record = q
        self.starts = []
        while q + 4 <= len(d):
            self.starts.append(q)
            q += 4 + struct.unpack_from("<i", d, q)[0]
        assert q == len(d)

    def member_of(self, at):
        """the member that holds offset `at` of the inflated stream"""
        return max(k for k, m in enumerate(self.members) if m[4] and m[3] <= at)

    def voff(self, at):
        m = self.members[self.member_of(at)]
        return (m[0] << 16) | (at - m[3])

    def at(self, v):
        """offset in the inflated stream of virtual offset `v`, which must be a good one"""
        m, = [m for m in self.members if m[0] == v >> 16]
        assert (v & 0xFFFF) < m[4]
        return m[3] + (v & 0xFFFF)

    def record_at(self, p):
        """the end of the record at `p` if one starts there by the rule's (2), or None"""
        d = self.data
        if p + 4 > len(d):
            return None
        bs, = struct.unpack_from("<i", d, p)
        if bs < 32 or p + 4 + bs > len(d):
            return None
        rid, pos, l_rn, _mq, _bin, n_cig, _flag, l_seq = struct.unpack_from("<iiBBHHHi", d, p + 4)
        if l_rn < 1 or l_seq < 0 or 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or d[p + 4 + 32 + l_rn - 1] != 0:
            return None
        if not -1 <= rid < len(self.ref_lens) or (rid >= 0 and not 0 <= pos < self.ref_lens[rid]):
            return None
        return p + 4 + bs


def parse_bai(raw):
    """[(n_bin, [linear offsets])] per reference, or None where the file is no .bai: a count that is negative or that the
    bytes left cannot hold, a field cut short, a wrong magic"""
    if len(raw) < 8 or raw[:4] != b"BAI\1":
        return None
    q, out = 4, []

    def take(fmt):
        nonlocal q
        n = struct.calcsize(fmt)
        if q + n > len(raw):
            raise EOFError
        v = struct.unpack_from(fmt, raw, q)
        q += n
        return v

    try:
        n_ref, = take("<i")
        if n_ref < 0 or n_ref * 8 > len(raw) - q:
            return None
        for _ in range(n_ref):
            n_bin, = take("<i")
            if n_bin < 0 or n_bin * 8 > len(raw) - q:
                return None
            for _ in range(n_bin):
                _bin, n_chunk = take("<Ii")
                if n_chunk < 0 or n_chunk * 16 > len(raw) - q:
                    return None
                q += 16 * n_chunk
            n_intv, = take("<i")
            if n_intv < 0 or n_intv * 8 > len(raw) - q:
                return None
            out.append((n_bin, list(take(f"<{n_intv}Q"))))
    except EOFError:
        return None
    return out


def declared_with_reads(bai_raw, n_ref):
    """the contigs a one-pass handle may take for the ones with reads: those with a bin or a non-zero linear offset in an
    index whose n_ref is the header's -- every contig otherwise"""
    refs = parse_bai(bai_raw)
    if refs is None or len(refs) != n_ref:
        return set(range(n_ref))
    return {k for k, (n_bin, lin) in enumerate(refs) if n_bin > 0 or any(lin)}


def rewrite_bai(raw, fn):
    """The .bai `raw` with every non-zero linear offset v mapped through fn(v, ref, k) (k: its place in the reference's
    linear index); bins and chunks as they are."""
    out = bytearray(raw)
    n_ref, = struct.unpack_from("<i", raw, 4)
    q = 8
    for ref in range(n_ref):
        n_bin, = struct.unpack_from("<i", raw, q)
        q += 4
        for _ in range(n_bin):
            n_chunk, = struct.unpack_from("<i", raw, q + 4)
            q += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", raw, q)
        q += 4
        for k in range(n_intv):
            v, = struct.unpack_from("<Q", raw, q)
            if v:
                struct.pack_into("<Q", out, q, fn(v, ref, k) & 0xFFFFFFFFFFFFFFFF)
            q += 8
    assert q == len(raw)
    return bytes(out)


def linear_offsets(raw):
    return sorted({v for _, lin in parse_bai(raw) for v in lin if v})


def expected(bam_bytes, bai_bytes, world, stream=None):
    """REFUSE, or the world + 1 cuts as offsets into the inflated stream (the first record's start first, the stream's
    length last): THE RULE of the module's docstring."""
    s = stream or Stream(bam_bytes)
    refs = parse_bai(bai_bytes)
    if refs is None or len(refs) != len(s.ref_lens):
        return REFUSE
    offs = sorted({v for _, lin in refs for v in lin if v})
    if not offs:
        return REFUSE
    by_coff = {m[0]: m for m in s.members}
    for v in offs:                                                          # (1), of EVERY offset
        m = by_coff.get(v >> 16)
        if m is None or (v & 0xFFFF) >= m[4] or m[3] + (v & 0xFFFF) < s.first_record:
            return REFUSE
    c0, c1 = s.members[0][1], s.members[-1][1] + s.members[-1][2]
    cuts = [s.first_record]
    for k in range(1, world):
        target = (c0 + (c1 - c0) * k // world) << 16
        v = next((x for x in offs if x >= target), None)
        if v is None:
            cuts.append(len(s.data))
            continue
        at = by_coff[v >> 16][3] + (v & 0xFFFF)
        nx = s.record_at(at)                                                # (2) and (3), of the cuts
        if nx is None or (nx != len(s.data) and s.record_at(nx) is None):
            return REFUSE
        cuts.append(at)
    return cuts + [len(s.data)]


def _index_of(tmp_path, name, refs, recs):
    p = str(tmp_path / (name + ".bam"))
    bam.write_bam(p, refs, recs, level=1)
    return open(bam.write_bai(p), "rb").read()


# outcomes by name, at every world of WORLDS (tests/test_bai_trust.py asserts them beside expected())
ACCEPTED = ("true", "samtools-like", "stale-first-250", "stale-contig-a", "next-record", "straddle")
MID_RECORD = ("uoff+1", "uoff+4", "uoff+36", "first-cigar-word")
REFUSED = MID_RECORD + ("coff-10", "coff+18", "past-eof", "plus-7000", "uoff=out_len", "uoff=0xffff", "foreign", "stale-every-other")


def index_family(tmp_path, path, recs):
    """{name: bytes of a .bai} for the file at `path` (share_test_bam's), in the order of the issue's list"""
    s = Stream(open(path, "rb").read())
    true = open(bam.write_bai(path, str(tmp_path / "true.bai")), "rb").read()
    fam = {"true": true,
           "samtools-like": open(bam.write_bai(path, str(tmp_path / "bins.bai"), bins=True), "rb").read(),
           # an earlier version of the same file, the same header
           "stale-first-250": _index_of(tmp_path, "first250", REFS, recs[:250]),
           "stale-contig-a": _index_of(tmp_path, "contig_a", REFS, recs[:300]),
           "stale-every-other": _index_of(tmp_path, "every_other", REFS, recs[::2])}
    rng = np.random.default_rng(11)
    other = []
    for k in range(300):
        n = int(rng.integers(300, 700))
        other.append(dict(name=f"f{k}", flag=0, ref_id=k // 150, pos=(k % 150) * 900, cigar=[(0, n)], seq="".join(rng.choice(list("ACGT"), n)),
                          qual=bytes(rng.integers(0, 94, n, dtype=np.uint8)), hp=None))
    fam["foreign"] = _index_of(tmp_path, "foreign", REFS, other)
    offs = linear_offsets(true)
    upper = set(offs[len(offs) - (2 * len(offs)) // 5:])                    # the upper 40 %
    member_len = {m[0]: m[4] for m in s.members}

    def l_read_name(v):
        return s.data[s.at(v) + 12]

    def next_record(v):
        k = s.starts.index(s.at(v))
        return s.voff(s.starts[k + 1]) if k + 1 < len(s.starts) else v

    def last_of_member(v):
        k = s.member_of(s.at(v))
        return s.voff(max(q for q in s.starts if s.member_of(q) == k))

    mutants = {"uoff+1": lambda v, r, k: v + 1, "uoff+4": lambda v, r, k: v + 4, "uoff+36": lambda v, r, k: v + 36,
               "first-cigar-word": lambda v, r, k: s.voff(s.at(v) + 36 + l_read_name(v)),
               "next-record": lambda v, r, k: next_record(v),
               "coff-10": lambda v, r, k: v - (10 << 16) if v >> 16 >= 10 else v,
               "coff+18": lambda v, r, k: v + (18 << 16),                     # (the payload's offset, not the member's)
               "past-eof": lambda v, r, k: v + (len(s.raw) << 16) if v in upper else v,
               "plus-7000": lambda v, r, k: v + (7000 << 16) if v in upper else v,
               "uoff=out_len": lambda v, r, k: (v & ~0xFFFF) | member_len[v >> 16],
               "uoff=0xffff": lambda v, r, k: v | 0xFFFF,
               # every offset moved to the LAST record that starts in its member: where that record ends in the next member
               # (asserted by the test), the cut's record straddles two BGZF members
               "straddle": lambda v, r, k: last_of_member(v)}
    for name, fn in mutants.items():
        fam[name] = rewrite_bai(true, fn)
    assert set(fam) == set(ACCEPTED) | set(REFUSED) and all(fam[n] != true for n in fam if n != "true")
    return fam


def malformed(true, n_ref):
    """{name: bytes}: files that are no .bai for a header of n_ref contigs (every proper prefix of `true` is another)"""
    big, head = struct.pack("<i", 0x7FFFFFFF), b"BAI\1" + struct.pack("<i", n_ref)
    return {"n_ref=0x7fffffff": b"BAI\1" + big + struct.pack("<i", 0),
            "n_bin=0x7fffffff": head + big,
            "n_chunk=0x7fffffff": head + struct.pack("<iI", 1, 4681) + big,
            "n_intv=0x7fffffff": head + struct.pack("<i", 0) + big,
            "wrong-magic": b"BAJ\1" + true[4:],
            "n_ref-off-by-one": b"BAI\1" + struct.pack("<i", n_ref + 1) + true[8:] + struct.pack("<ii", 0, 0)}


def straddles(s, at):
    """the record at `at` begins in one BGZF member and ends in a later one"""
    end = s.record_at(at)
    return s.member_of(at) != s.member_of(end - 1)
