"""Inputs shared by tests/test_bam_cs.py and tests/test_gpu_bam_cs.py (--records full --cs / --de, NPORE_TAG_*): the table of the
rule's examples on raw code arrays (codes 0 and 5 on either side included), the crafted reads at which the device walk can go
wrong -- besides those of bam_md_cases, which both tests run as well --, the reads at the seams of the device walks' frame
(seam_reads), a cs reader for the identities, and the splice that
turns today's record into the record with the new tags.  Every expectation is written down from the rule
(csrc/cs_rec.hpp), not from a run."""
import re
import struct

import numpy as np

from npore_amd import bam
import bam_full_cases as fc
import bam_md_cases as mc
import long_cigar_cases as lc

M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
OPS = "MIDNSHP=X"
FORMS = (None, "short", "long")

# (reference codes, read codes, final CIGAR, cs short, cs long, (E, X, G)) -- 'NACGT-' are the codes 0 ... 5; pinned by hand
TABLE = [
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 1, 2, 3, 4], "8M", ":8", "=ACGTACGT", (8, 0, 0)),
    ([1, 2, 3, 4, 1, 2, 3, 4], [2, 2, 3, 4, 1, 2, 3, 4], "8M", "*ac:7", "*ac=CGTACGT", (7, 1, 0)),
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 1, 2, 3, 1], "8M", ":7*ta", "=ACGTACG*ta", (7, 1, 0)),
    ([1], [3], "1M", "*ag", "*ag", (0, 1, 0)),
    ([1, 2, 3, 4, 1, 2, 3, 4, 1, 2], [1, 2, 3, 4, 3, 4, 1, 2], "4M2D4M", ":4-ac:4", "=ACGT-ac=GTAC", (8, 0, 1)),
    ([1, 2, 3, 4, 1, 2, 3, 4, 1, 2], [1, 2, 3, 4, 2, 4, 1, 2], "4M2D4M", ":4-ac*gc:3", "=ACGT-ac*gc=TAC", (7, 1, 1)),
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 4, 4, 1, 2, 3, 4], "4M2I4M", ":4+tt:4", "=ACGT+tt=ACGT", (8, 0, 1)),
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 1, 2, 3, 4], "3=2X3M", ":8", "=ACGTACGT", (8, 0, 0)),            # one stretch through three words
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 3, 4], "4M2N2M", ":4:2", "=ACGT=GT", (6, 0, 0)),                  # N ends the stretch, skips AC
    ([], [1, 2, 3], "3I", "+acg", "+acg", (0, 0, 1)),
    ([1, 2, 3], [], "3D", "-acg", "-acg", (0, 0, 1)),
    ([1, 2, 3], [4], "2D1I1D", "-ac+t-g", "-ac+t-g", (0, 0, 3)),                                              # neighbouring gaps: one open each
    ([1, 0, 3, 5], [1, 0, 3, 5], "4M", ":1*nn:2", "=A*nn=GN", (3, 1, 0)),                                     # 0 on 0 differs, 5 on 5 does not
    ([0, 2, 5], [1, 2, 3], "3M", "*na:1*ng", "*na=C*ng", (1, 2, 0)),                                          # ... in the reference
    ([1, 2, 3], [0, 2, 5], "3M", "*an:1*gn", "*an=C*gn", (1, 2, 0)),                                          # ... in the read
    ([0, 5, 1], [5, 0, 2], "1M1D1I1M1I", "*nn-n+n*ac+n", "*nn-n+n*ac+n", (0, 2, 3)),                          # ... under I and D
    ([1, 2], [1, 2], "2M1D2M1I", ":2-n*nn*nn+n", "=AC-n*nn*nn+n", (2, 2, 2)),                                 # beyond both arrays: code 0
    ([1, 2], [1, 2], "0M2M0I0D", ":2", "=AC", (2, 0, 0)),                                                     # a word of length 0 does nothing
    ([], [], "", "", "", (0, 0, 0)),
]


def table_de(e, x, g):
    return np.float32((x + g) / (e + x + g)) if e + x + g else np.float32(0.0)


def words_of(final):
    return [int(n) << 4 | OPS.index(op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", final)]


def parse_cs(text):
    """[(sign, payload)] of a cs text in either form; asserts the grammar"""
    toks = re.findall(r":\d+|=[ACGTN]+|\*[acgtn]{2}|\+[acgtn]+|-[acgtn]+", text)
    assert "".join(toks) == text, text
    return [(t[0], t[1:]) for t in toks]


def cs_identities(short, long, nm, final, md=None):
    """The identities of the issue on one read's two texts"""
    ts, tl = parse_cs(short), parse_cs(long)
    stars = sum(1 for s, _ in ts if s == "*")
    assert stars + sum(len(p) for s, p in ts if s in "+-") == nm, (short, nm)
    m_len = sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", final) if op in "M=X")
    assert sum(int(p) for s, p in ts if s == ":") + stars == m_len, (short, final)
    assert re.sub(r"=([ACGTN]+)", lambda m: f":{len(m.group(1))}", long) == short
    assert all(int(p) > 0 for s, p in ts if s == ":")
    for (s1, _), (s2, _) in zip(ts, ts[1:]):
        assert not (s1 == ":" and s2 == ":") or "N" in final, short          # a stretch is maximal (only N splits one silently)
    if md is not None:
        assert sum(c.isalpha() for c in re.sub(r"\^[A-Z]+", "", md)) == stars, (md, short)


def new_tags_of(rec_with):
    """(cs text or None, de float or None, names of the tags in order) of a FULL record"""
    f, name, words, body, aux = fc.parse_full(rec_with)
    tags = mc.parse_tags(aux)
    cs = [v[:-1].decode() for t, ty, v in tags if t == b"cs" and ty == b"Z"]
    de = [struct.unpack("<f", v)[0] for t, ty, v in tags if t == b"de" and ty == b"f"]
    assert len(cs) <= 1 and len(de) <= 1
    return (cs[0] if cs else None), (de[0] if de else None), [t for t, _, _ in tags]


def tag_offset(rec, tag):
    """where the tag begins in the record (block_size word first)"""
    aux = fc.parse_full(rec)[4]
    tags = mc.parse_tags(aux)
    k = [t for t, _, _ in tags].index(tag)
    return len(rec) - len(aux) + sum(3 + len(v) for _, _, v in tags[:k])


def splice(plain, extra):
    """Today's FULL record `plain` (block_size word first) with the tag bytes `extra` in front of its CG tag (at its end where
    it has none) -- what the record with the new tags must be"""
    f, name, words, body, aux = fc.parse_full(plain)
    tags = mc.parse_tags(aux)
    cut = len(plain)
    if tags and tags[-1][0] == b"CG":
        cut -= 3 + len(tags[-1][2])
    out = plain[4:cut] + extra + plain[cut:]
    return struct.pack("<i", len(out)) + out


_CRAFTED = {}


def crafted_reads(seed=17):
    """(references, refs, records, finals, {name: (cs short pinned by hand, de as (E, X, G) or None)}).  Computed once, shared,
    never changed.  See the module's list in the issue's words: digit-width changes of the counts; a stretch through two and
    three M-type words and over a tile border with the 256th / 257th word inside it; insertions and deletions of 1, 63, 64, 65
    and 130 bases; a differing position first, last, alone, everywhere; 1M1I and 1M1D for 300 words; code 0 on either side;
    a reference array shorter than the final claims; the tag at every byte alignment with short texts and texts of 63 / 64 /
    65 bytes; a refused read between two good ones; more than 65 535 words with the clips; stale cs / de beside RG and a B
    array in the input."""
    if seed in _CRAFTED:
        return _CRAFTED[seed]
    rng = np.random.default_rng(seed)
    contig = list(lc.random_contig(rng, 90000))
    for p in (40003, 40007):
        contig[p] = "N"
    contig = "".join(contig)
    low = lambda s: s.lower()
    records, finals, pinned = [], [], {}

    def add(name, pos, runs, edits=(), clips=([], []), seq_sub=None, status=0, rec_cigar=None, final=None, tags=None, ins=None):
        """runs: the FINAL CIGAR as [(op, len)]; the read is the contig under it with `edits` (query offsets) substituted; the
        record's own CIGAR is the final one with = and X as M unless rec_cigar says otherwise.  ins: the inserted letters."""
        seq, at, ins_it = [], pos, iter(ins or ())
        for op, ln in runs:
            if op in (M, EQ, X):
                seq += list(contig[at:at + ln])
            elif op == I:
                seq += list(next(ins_it, None) or lc.random_contig(rng, ln))
            if op in (M, EQ, X, D, N):
                at += ln
        for e in edits:
            seq[e] = mc.other(seq[e])
        for e, c in (seq_sub or {}).items():
            seq[e] = c
        nl, nt = sum(n for op, n in clips[0] if op == S), sum(n for op, n in clips[1] if op == S)
        k = len(records)
        if tags is None:
            tags = (b"", b"RGZgrp\0", b"csZ:3*ac:3\0PSi" + struct.pack("<i", k), b"def" + struct.pack("<f", 0.5) + b"XZZ" + b"a" * (k % 5) + b"\0")[k % 4]
        own = rec_cigar if rec_cigar is not None else [(M if op in (EQ, X) else op, ln) for op, ln in runs]
        records.append(dict(name=name, flag=0, ref_id=0, pos=pos, mapq=40, seq="G" * nl + "".join(seq) + "T" * nt,
                            cigar=clips[0] + list(own) + clips[1],
                            qual=bytes(rng.integers(0, 50, nl + len(seq) + nt).tolist()) if seq or nl or nt else None, tags=tags,
                            _status=status, _ctg="ctg"))
        finals.append(final if final is not None else "".join(f"{ln}{OPS[op]}" for op, ln in runs))
        return "".join(seq)

    pos = 100
    # a mismatch, then 9 / 10 / 99 / ... / 10 000 matches, ..., a closing mismatch
    counts = (9, 10, 99, 100, 999, 1000, 9999, 10000)
    at, ed = 0, []
    for c in counts:
        ed.append(at)
        at += 1 + c
    ed.append(at)
    add("counts", pos, [(M, at + 1)], edits=tuple(ed))
    star = lambda p: "*" + low(contig[p]) + low(mc.other(contig[p]))
    pinned["counts"] = ("".join(star(pos + e) + f":{c}" for e, c in zip(ed, counts)) + star(pos + at), (sum(counts), 9, 0))
    pos += at + 100
    # one stretch through two and three M-type words
    add("two_words", pos, [(EQ, 40), (M, 30)])
    pinned["two_words"] = (":70", (70, 0, 0))
    add("three_words", pos + 100, [(I, 2), (EQ, 70), (X, 64), (M, 5), (D, 1), (M, 3)], ins=["AC"])
    pinned["three_words"] = ("+ac:139-" + low(contig[pos + 239]) + ":3", (142, 0, 2))
    pos += 400
    # 127 x (2M 1I) = 254 words, then 3M 4= | 5X 6M: the 256th and the 257th word (a tile border) inside one stretch of 18 + 2
    runs = [(M, 2), (I, 1)] * 127 + [(M, 3), (EQ, 4), (X, 5), (M, 6)]
    seq = add("border", pos, runs, edits=(0,))
    ins_at = [3 * j + 2 for j in range(127)]
    pinned["border"] = (star(pos) + ":1+" + low(seq[2]) + "".join(f":2+{low(seq[q])}" for q in ins_at[1:]) + ":18", (254 + 18 - 1, 1, 127))
    pos += 600
    for n in (1, 63, 64, 65, 130):
        seq = add(f"ins{n}", pos, [(M, 5), (I, n), (M, 5)])
        pinned[f"ins{n}"] = (f":5+{low(seq[5:5 + n])}:5", (10, 0, 1))
        add(f"del{n}", pos + 200, [(M, 5), (D, n), (M, 5)])
        pinned[f"del{n}"] = (f":5-{low(contig[pos + 205:pos + 205 + n])}:5", (10, 0, 1))
        pos += 600
    add("diff_first", pos, [(M, 10)], edits=(0,))
    pinned["diff_first"] = (star(pos) + ":9", (9, 1, 0))
    add("diff_last", pos + 100, [(M, 10)], edits=(9,))
    pinned["diff_last"] = (":9" + star(pos + 109), (9, 1, 0))
    add("diff_alone", pos + 200, [(M, 1)], edits=(0,))
    pinned["diff_alone"] = (star(pos + 200), (0, 1, 0))
    add("diff_all", pos + 300, [(M, 130)], edits=tuple(range(130)))            # three bytes per base: the bound's worst case
    pinned["diff_all"] = ("".join(star(pos + 300 + q) for q in range(130)), (0, 130, 0))
    add("diff_all_long", pos + 500, [(M, 40), (EQ, 60), (M, 30)], edits=tuple(range(130)), clips=([(S, 2)], [(H, 1)]))
    pinned["diff_all_long"] = ("".join(star(pos + 500 + q) for q in range(130)), (0, 130, 0))
    pos += 800
    seq = add("mi300", pos, [(M, 1), (I, 1)] * 150)
    pinned["mi300"] = ("".join(f":1+{low(seq[2 * j + 1])}" for j in range(150)), (150, 0, 150))
    add("md300", pos + 300, [(M, 1), (D, 1)] * 150)
    pinned["md300"] = ("".join(f":1-{low(contig[pos + 300 + 2 * j + 1])}" for j in range(150)), (150, 0, 150))
    pos += 800
    # code 0: contig N at 40003 (under M) and 40007 (under D); N and an IUPAC letter in the read
    add("n_in_ref", 40000, [(M, 5), (D, 4), (M, 6)])
    pinned["n_in_ref"] = (":3*nn:1-" + low(contig[40005:40007]) + "n" + low(contig[40008]) + ":6", (10, 1, 1))
    add("n_in_read", 40100, [(M, 6), (I, 3), (M, 6)], seq_sub={2: "N", 7: "R", 11: "N"}, ins=["ACG"])
    pinned["n_in_read"] = (f":2*{low(contig[40102])}n:3+ang:2*{low(contig[40108])}n:3", (10, 2, 1))
    # the record covers 20 reference bases and has 20 read bases; the final names 27 and 33
    add("past_end", 40200, [(M, 20)], final="18M3I4M2D1M5I")
    pinned["past_end"] = (":18+" + low(contig[40218:40220]) + "n*" + low(contig[40218]) + "n*" + low(contig[40219]) + "n*nn*nn-nn*nn+nnnnn", (18, 5, 3))
    add("refused_before", 40300, [(M, 30)], edits=(3,))
    add("refused", 40310, [(M, 30)], status=32)
    add("refused_after", 40320, [(M, 30)], edits=(4,))
    add("no_words", 40400, [(M, 10)], final="", clips=([(S, 2)], []))
    pinned["no_words"] = ("", (0, 0, 0))
    # the tag at every byte alignment: the same kind of read under names of 1 ... 4 letters; texts of 0, 2, 3, 4 bytes (no cs
    # text has one byte: the shortest item has two) and, all-I reads, of 63, 64, 65 bytes
    for k, name in enumerate(("b", "bl", "bln", "blnx")):
        p = 40500 + 100 * k
        if k == 0:
            add(name, p, [(M, 4)], final="", tags=b"")
            pinned[name] = ("", (0, 0, 0))
        else:
            ln = (0, 7, 12, 120)[k]
            add(name, p, [(M, ln)], tags=b"")
            pinned[name] = (f":{ln}", (ln, 0, 0))
    for k, (name, n) in enumerate((("c", 62), ("cl", 63), ("cln", 64), ("clnx", 62))):
        seq = add(name, 41000 + 100 * k, [(I, n)], tags=b"")
        pinned[name] = ("+" + low(seq), (0, 0, 1))
    # more than 65 535 words with the clips: CG goes behind cs and de
    seq = add("long", 42000, [(M, 1), (I, 1)] * 32767, clips=([(H, 1), (S, 2)], [(S, 1)]), rec_cigar=[(M, 32767), (I, 32767)],
              tags=b"RGZlong\0csZ:1\0def" + struct.pack("<f", 0.25))
    pinned["long"] = ("".join(f":1+{low(seq[2 * j + 1])}" for j in range(32767)), (32767, 0, 32767))
    # stale cs and de beside RG and a B array: the first two are replaced, the others kept in order
    add("stale", 80000, [(M, 12), (D, 1), (M, 12)], edits=(5,),
        tags=b"csZ:24\0RGZgrp\0def" + struct.pack("<f", 0.125) + b"MLBC" + struct.pack("<i", 5) + bytes(range(5)) + b"NMC\x03")
    pinned["stale"] = (":5" + star(80005) + ":6-" + low(contig[80012]) + ":12", (23, 1, 1))
    both = sorted(zip(records, finals), key=lambda rf: rf[0]["pos"])
    out = ([("ctg", len(contig))], {"ctg": contig}, [r for r, _ in both], [f for _, f in both], pinned)
    _CRAFTED[seed] = out
    return out


_SEAMS = {}


def seam_reads(seed=23):
    """(references, refs, records, finals): reads at the seams of the device walks' frame (csrc/bam_emit_kernels.hpp: tiles
    of 64 words, rounds of 64 positions), where the carry between the rounds of one word meets the carry between two tiles
    of words.  The last word of a tile -- word 64, in the last
    read word 128 -- is an M of 1, 64, 65 or 129 positions that continues a stretch begun in the = word before it; positions
    differ at the in-round offsets 0 and 63 and at the first position of the next round (64, 128), at the word's first and last
    position alone, or nowhere, so that the open stretch leaves the tile; the next tile begins with an M-type word, an I and
    a D in turn.  Computed once, shared, never changed."""
    if seed in _SEAMS:
        return _SEAMS[seed]
    rng = np.random.default_rng(seed)
    contig = lc.random_contig(rng, 12000)
    records, finals = [], []

    def add(name, pos, front, seam, diffs, nxt):
        runs = front + [(M, seam), nxt, (M, 4), (D, 1), (EQ, 70)]
        q0 = sum(ln for op, ln in front if op in (M, EQ, X, I))     # the seam word's first query base
        seq, at = [], pos
        for op, ln in runs:
            if op in (M, EQ, X):
                seq += list(contig[at:at + ln])
            elif op == I:
                seq += list(lc.random_contig(rng, ln))
            if op in (M, EQ, X, D):
                at += ln
        for d in diffs:
            seq[q0 + d] = mc.other(seq[q0 + d])
        records.append(dict(name=name, flag=0, ref_id=0, pos=pos, mapq=40, seq="".join(seq), cigar=[(M if op in (EQ, X) else op, ln) for op, ln in runs],
                            qual=bytes(rng.integers(0, 50, len(seq)).tolist()), tags=b"", _status=0, _ctg="ctg"))
        finals.append("".join(f"{ln}{OPS[op]}" for op, ln in runs))
        return at

    pos = 50
    front = [(M, 2), (I, 1)] * 31 + [(EQ, 3)]                      # words 1 ... 63
    for i, seam in enumerate((1, 64, 65, 129)):
        patterns = ([d for d in (0, 63, 64, 127, 128) if d < seam], [], sorted({0, seam - 1}))
        for j, nxt in enumerate(((X, 5), (I, 3), (D, 3))):          # every pattern meets every kind of next word
            pos = add(f"seam{seam}{OPS[nxt[0]]}", pos, front, seam, patterns[(i + j) % 3], nxt) + 30
    add("seam128", pos, [(M, 2), (D, 1)] * 63 + [(EQ, 1)], 65, [0, 63, 64], (I, 2))
    assert all(len(words_of(f)) in (68, 132) and words_of(f)[len(words_of(f)) - 5] & 15 == M for f in finals)      # the seam word ends a tile
    out = ([("ctg", len(contig))], {"ctg": contig}, records, finals)
    _SEAMS[seed] = out
    return out


def want_stream(raws, records, contigs, finals, status, md=False, cs=None, de=False):
    """bam.full_record(md=, cs=, de=) of every kept read, one after the other"""
    out = []
    for raw, rec, fin, st in zip(raws, records, finals, status):
        if st & 32:
            continue
        rc, sc, _ = lc.expected_pack(rec, rec["cigar"], contigs[rec.get("_ctg", "ctg")])
        out.append(bam.full_record(raw, rc, sc, fin, md=md, cs=cs, de=de))
    return b"".join(out)
