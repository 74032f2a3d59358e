"""Inputs shared by tests/test_bam_full.py and tests/test_gpu_bam_full.py (--records full): aux blocks with what a FULL
record keeps of each, a BAM like test_gpu_bam_out.clipped_bam with tags, mate fields and hard clips of every kind, reads
for the long-CIGAR threshold and for NM -- every expectation written down from the rule (csrc/bam_reader.hpp FULL RECORD,
csrc/nm_rec.hpp), not from a run."""
import struct

import numpy as np

from npore_amd import bam, synth
import long_cigar_cases as lc

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
p32 = lambda v: struct.pack("<I", v)


def aux_cases():
    """[(name, aux bytes of the input record, the bytes a FULL record keeps of them)]"""
    rg, ps, nm, md, cs, de, dv = b"RGZgrp\0", b"PSi" + struct.pack("<i", -7), b"NMC\x03", b"MDZ10A5\0", b"csZ:10*ag\0", \
        b"def" + struct.pack("<f", 0.25), b"dvf" + struct.pack("<f", 0.5)
    cg = b"CGBI" + p32(2) + p32(5 << 4) + p32(6 << 4 | 1)
    every = [b"XAAq", b"Xcc\xff", b"XCC\x07", b"Xss" + struct.pack("<h", -300), b"XSS" + struct.pack("<H", 60000),
             b"Xii" + struct.pack("<i", -70000), b"XII" + p32(4000000000), b"Xff" + struct.pack("<f", 1.5), b"XZZtext\0", b"XHH1AE3\0"]
    arrays = [b"Y" + sub + b"B" + sub + p32(3) + bytes(3 * w) for sub, w in
              ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4))]
    look = [b"nmC\x01", b"MdZx\0", b"cSZy\0", b"CgC\x02"]
    cases = [
        ("none", b"", b""),
        ("only dropped", nm + md + cs + de + dv + cg, b""),
        ("dropped first", nm + rg + ps, rg + ps),
        ("dropped middle", rg + md + cs + ps, rg + ps),
        ("dropped last", rg + ps + cg, rg + ps),
        ("every scalar type", b"".join(every), b"".join(every)),
        ("every array subtype", b"".join(arrays) + dv, b"".join(arrays)),
        ("empty array", b"MLBC" + p32(0) + rg, b"MLBC" + p32(0) + rg),
        ("empty Z", b"XZZ\0" + nm + b"YZZ\0", b"XZZ\0YZZ\0"),
        ("look-alikes", b"".join(look) + nm, b"".join(look)),
        ("HP between", rg + b"HPC\x02" + de + ps, rg + b"HPC\x02" + ps),
        # malformed tails: everything from the tag that cannot be stepped over is dropped
        ("unknown type", rg + nm + b"XQQ\x01\x02" + ps, rg),
        ("value cut", rg + b"XII\x01\x02", rg),
        ("value cut 16", ps + md + b"Xss\x01", ps),
        ("Z without NUL", rg + b"XZZabc", rg),
        ("B count past end", rg + ps + b"XBBC" + p32(9) + bytes(8), rg + ps),
        ("B head cut", rg + b"XBBC\x01\x00", rg),
        ("B unknown subtype", b"XBBZ" + p32(1) + b"\0" + rg, b""),
        ("two stray bytes", rg + b"XY", rg),
        ("malformed dropped tag", rg + b"NMZabc", rg),
    ]
    return cases


def aux_bam(path):
    """A BAM with one read per aux case on a contig of A's: (path, fasta text, [aux], [kept])."""
    cases = aux_cases()
    contig = "ACGT" * 200
    records = [dict(name=f"a{k}", flag=0, ref_id=0, pos=10 + k, mapq=30, cigar=[(S, 1), (M, 20), (I, 1), (M, 9), (H, 2)],
                    seq=contig[9 + k:30 + k] + "A" + contig[30 + k:39 + k], qual=bytes(range(31)), tags=aux) for k, (_, aux, _) in enumerate(cases)]
    bam.write_bam(path, [("ctg", len(contig))], records)
    return contig, records, [c[1] for c in cases], [c[2] for c in cases]


HP_TAGS = [None, b"HPC\x02", b"HPS" + struct.pack("<H", 300), b"HPI" + p32(70000), b"HPc\xff", b"HPs" + struct.pack("<h", -129),
           b"HPi" + struct.pack("<i", -40000)]
HP_VALUES = [0, 2, 300, 70000, -1, -129, -40000]


# the clips of a read (leading, trailing) and the tags in front of and behind its HP: read k takes CLIPS[k % 8], FRONT_TAGS[k % 4],
# HP_TAGS[k % 7] and BACK_TAGS[(k // 2) % 4] (genome_scale_cases.py deals the same tables)
CLIPS = [([], []), ([(S, 3)], []), ([(H, 4), (S, 4)], [(S, 2), (H, 7)]), ([(H, 5)], []), ([(S, 1)], [(S, 2)]), ([], [(H, 6)]),
         ([(S, 4)], [(S, 5)]), ([(H, 1)], [(H, 1)])]
FRONT_TAGS = [b"RGZgrp1\0", b"NMC\x05" + b"RGZg2\0", b"MLBC" + p32(6) + bytes([0, 255, 3, 4, 5, 6]), b""]
BACK_TAGS = [b"PSi" + struct.pack("<i", 12345), b"MDZ10A5\0" + b"mvBc" + p32(3) + bytes([1, 0, 1]), b"", b"SAZctg,1,+,5S,60,0;\0" + b"def" + struct.pack("<f", .1)]


def full_records(seed=5, n_reads=24, ref_len=1500):
    """(references, {contig name: bases}, records for bam.write_bam, [the real CIGAR of each]): reads with soft clips of even
    and odd length, H + S at both ends, an H without S at either end, no clips, N / ambiguity codes, both strands, reads
    without qualities, mate fields, tags around an HP of every integer width and none -- stale ones among them --, and one
    read (7) whose CIGAR disagrees with its sequence."""
    rng = np.random.default_rng(seed)
    refs, seqs, cigs = synth.make_batch(77, n_reads, ref_len=ref_len, p_np=0.1)
    dec = lambda a: "".join("NACGT"[x] for x in a)
    contig, recs = [], []
    clips, front, back = CLIPS, FRONT_TAGS, BACK_TAGS
    for k, (rf, sq, cg) in enumerate(zip(refs, seqs, cigs)):
        pos = len(contig) + 20
        contig += list("ACGT"[x] for x in rng.integers(0, 4, 20)) + list(dec(rf))
        cg = cg.decode() if isinstance(cg, (bytes, bytearray)) else cg if isinstance(cg, str) else "".join(chr(x) for x in cg)
        runs, last, cnt = [], None, 0
        for ch in cg:
            if ch == last:
                cnt += 1
            else:
                if last is not None:
                    runs.append(("MIDNSHP=XB".index(last), cnt))
                last, cnt = ch, 1
        runs.append(("MIDNSHP=XB".index(last), cnt))
        lead, trail = clips[k % len(clips)]
        cig = lead + runs + trail
        nl, nt = sum(n for op, n in lead if op == S), sum(n for op, n in trail if op == S)
        body = dec(sq)
        if k % 7 == 3:
            body = body[:11] + "N" + body[12:40] + "R" + body[41:]
        n = nl + len(sq) + nt
        hp = HP_TAGS[k % len(HP_TAGS)]
        rec = dict(name=f"r{k}", flag=16 if k % 4 == 1 else 0, ref_id=0, pos=pos, mapq=k, cigar=cig, seq="A" * nl + body + "C" * nt,
                   qual=None if k % 5 == 0 else bytes(rng.integers(0, 60, n).tolist()),
                   tags=front[k % 4] + (hp or b"") + back[(k // 2) % 4], _hp=HP_VALUES[k % len(HP_TAGS)])
        if k % 2:
            rec.update(next_ref_id=0, next_pos=pos + 100 + k, tlen=500 + k)
        recs.append(rec)
    recs[7]["cigar"] = recs[7]["cigar"] + [(M, 5)]              # lengths now disagree: refused, not written
    contig = "".join(contig) + "ACGT" * 10
    return [("ctg", len(contig))], {"ctg": contig}, recs, [r["cigar"] for r in recs]


def write_inputs(tmp_path, references, refs, records, name="s"):
    bp, fa = str(tmp_path / f"{name}.bam"), str(tmp_path / f"{name}.fa")
    bam.write_bam(bp, references, [{k: v for k, v in r.items() if not k.startswith("_")} for r in records])
    lc.write_fasta(fa, refs)
    return bp, fa


def input_records(path):
    """The records of a BAM file as they lie in its inflated stream, block_size word first."""
    data = bam._bgzf_decompress(path)
    l_text, = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", data, p)[0]
    out = []
    while p + 4 <= len(data):
        bs, = struct.unpack_from("<i", data, p)
        out.append(bytes(data[p:p + 4 + bs]))
        p += 4 + bs
    return out


def simple_final(rl, sl, k):
    """A final CIGAR of M / I / D that consumes rl reference and sl query bases (no DP here: the finals are given)."""
    m = min(rl, sl) - 1 - k % 3
    a = m // 2
    return f"{a}M" + (f"{sl - m}I" if sl > m else "") + f"{m - a}M" + (f"{rl - m}D" if rl > m else "")


def want_stream(raws, records, cigars, contig, finals, status):
    """bam.full_record of every kept read, one after the other."""
    out = []
    for raw, rec, cig, fin, st in zip(raws, records, cigars, finals, status):
        if st & 32:
            continue
        rc, sc, _ = lc.expected_pack(rec, cig, contig)
        out.append(bam.full_record(raw, rc, sc, fin))
    return b"".join(out)


def parse_full(rec):
    """(fixed fields, name, CIGAR words, bases + qualities, aux) of a record, block_size word first."""
    f = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    l_rn, n_cig, l_seq = f[2], f[5], f[7]
    q = 36
    name = rec[q:q + l_rn]
    q += l_rn
    words = list(struct.unpack_from(f"<{n_cig}I", rec, q))
    q += 4 * n_cig
    body = rec[q:q + (l_seq + 1) // 2 + l_seq]
    return f, name, words, body, rec[q + len(body):]


def without_clips(lines):
    """SAM lines with the S and H operations taken out of the CIGAR column: a FULL record's CIGAR carries the input's clip
    words, the SAM route's text does not (sequence and qualities lose the clips in get_read_data either way)."""
    import re
    out = []
    for l in lines:
        f = l.split("\t")
        f[5] = re.sub(r"\d+[SH]", "", f[5])
        out.append("\t".join(f))
    return out


def nm_tag(nm):
    return b"NM" + (b"C" + struct.pack("<B", nm) if nm < 256 else b"S" + struct.pack("<H", nm) if nm < 65536 else b"I" + p32(nm))


def brute_nm(ref, seq, final):
    """NM by brute force on the expanded CIGAR over the LETTERS: I and D count, an M position counts unless both letters are
    the same one of ACGT."""
    import re
    ops = "".join(op * int(n) for n, op in re.findall(r"(\d+)([MID])", final))
    a = b = nm = 0
    for op in ops:
        if op == "M":
            nm += not (ref[a] == seq[b] and ref[a] in "ACGT")
            a, b = a + 1, b + 1
        elif op == "I":
            nm, b = nm + 1, b + 1
        else:
            nm, a = nm + 1, a + 1
    assert a == len(ref) and b == len(seq)
    return nm


def crafted_reads(seed=9):
    """Reads whose final CIGARs the tests supply -- (references, refs, records, finals): op counts 1, 63, 64, 65, 129 and a
    refused read; M runs of 1, 63, 64, 65 and 200 bases with mismatches at run offsets 0, 63, 64 and last; N in the reference
    only, in the read only, in both; all-I and all-D finals; NM of 255, 256 and 65 536; aux blocks of 0 ... 9, 255, 256, 257,
    4 099 and 40 000 bytes (1 - 3: no tag is that short; the reads' names, CIGARs and lengths vary every copy's alignment)."""
    rng = np.random.default_rng(seed)
    contig = list(lc.random_contig(rng, 72000))
    for p in (5003, 5007, 5008):
        contig[p] = "N"
    contig = "".join(contig)
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4] if c in "ACGT" else "A"
    records, finals = [], []
    aux_len = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 4099, 40000]

    def aux_of(n):
        """`n` bytes of tags: one B,C array from 8 bytes on, one Z tag from 4 (no tag is shorter than 4 bytes: 1 - 3 give none)"""
        if n >= 8:
            return b"MLBC" + p32(n - 8) + bytes(rng.integers(0, 256, n - 8).astype(np.uint8))
        return b"XZZ" + b"a" * (n - 4) + b"\0" if n >= 4 else b""

    def add(name, pos, runs, edits=(), clips=([], []), seq_n=(), status=0):
        """runs: the FINAL CIGAR as [(op, len)]; the read is the contig under it with `edits` (query offsets) substituted"""
        seq, at = [], pos
        for op, ln in runs:
            if op == M:
                seq += list(contig[at:at + ln])
            elif op == I:
                seq += list(lc.random_contig(rng, ln))
            if op in (M, D):
                at += ln
        for e in edits:
            seq[e] = other(seq[e])
        for e in seq_n:
            seq[e] = "N"
        nl, nt = sum(n for op, n in clips[0] if op == S), sum(n for op, n in clips[1] if op == S)
        k = len(records)
        n_aux = aux_len[k % len(aux_len)]
        rec = dict(name=name, flag=0, ref_id=0, pos=pos, mapq=50, cigar=clips[0] + list(runs) + clips[1], seq="G" * nl + "".join(seq) + "T" * nt,
                   qual=bytes(rng.integers(0, 50, nl + len(seq) + nt).tolist()) if seq or nl or nt else None, tags=aux_of(n_aux),
                   next_ref_id=0, next_pos=pos + 7, tlen=-k, _status=status)
        records.append(rec)
        finals.append("".join(f"{ln}{'MID'[op]}" for op, ln in runs))

    pos = 100
    for n_ops in (1, 63, 64, 65, 129):                           # M I M D M ... of n_ops operations
        runs = [((M, I, M, D)[j % 4], (7, 1, 5, 2)[j % 4]) for j in range(n_ops)]
        if runs[-1][0] != M:
            runs[-1] = (M, 3)
        add(f"ops{n_ops}", pos, runs, edits=(0,), clips=([(S, 3)], [(S, 2), (H, 4)]) if n_ops != 64 else ([], []))
        pos += 700
    add("refused", pos, [(M, 30)], status=32)
    pos += 100
    for ln in (1, 63, 64, 65, 200):                              # one long M run between two short ones
        offs = sorted({o for o in (0, 63, 64, ln - 1) if o < ln})
        add(f"run{ln}", pos, [(M, 4), (I, 2), (M, ln), (D, 3), (M, 6)], edits=tuple(6 + o for o in offs), clips=([(H, 2), (S, 1)], []))
        pos += 400
    add("n_in_ref", 5000, [(M, 20)])                             # contig N at 5003, 5007, 5008
    add("n_in_read", 6000, [(M, 20)], seq_n=(4,))
    add("n_in_both", 5000, [(M, 20)], seq_n=(3, 8))              # 5003 both, 5007 reference only, 5008 both
    add("all_i", 7000, [(I, 40)])
    add("all_d", 7100, [(D, 40)])
    add("nm255", 7200, [(I, 255)])
    add("nm256", 7500, [(I, 200), (D, 56)])
    add("nm65536", 3000, [(D, 65536)], clips=([], []))
    both = sorted(zip(records, finals), key=lambda rf: rf[0]["pos"])       # (coordinate order: the file gets an index)
    return [("ctg", len(contig))], {"ctg": contig}, [r for r, _ in both], [f for _, f in both]
