"""Inputs shared by tests/test_bam_md.py and tests/test_gpu_bam_md.py (--records full --md, NPORE_OUT_MD): the table of the
rule's examples, an independent brute-force MD over the LETTERS, an MD reader that rebuilds the reference under an alignment
the way pysam's get_reference_sequence() does, the crafted reads at which the device walk can go wrong, and random reads --
every expectation written down from the rule (csrc/md_rec.hpp), not from a run."""
import re
import struct

import numpy as np

from npore_amd import bam
import bam_full_cases as fc
import long_cigar_cases as lc

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
CODE = {c: i for i, c in enumerate("NACGT-")}
codes = lambda s: np.array([CODE.get(c, 0) for c in s], np.uint8)
other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4] if c in "ACGT" else "A"

# (reference under the alignment, read, final CIGAR, MD) -- the table of the rule's examples
TABLE = [
    ("ACGTACGT", "ACGTACGT", "8M", "8"),
    ("ACGTACGT", "CCGTACGT", "8M", "0A7"),
    ("ACGTACGT", "ACGTACGA", "8M", "7T0"),
    ("ACGTACGTAC", "ACGTGTAC", "4M2D4M", "4^AC4"),
    ("ACGTACGTAC", "ACGTCTAC", "4M2D4M", "4^AC0G3"),
    ("ACGTACGT", "ACGTTTACGT", "4M2I4M", "8"),
    ("", "ACGT" * 10, "40I", "0"),
    ("ACG", "", "3D", "0^ACG0"),
    ("ACG", "T", "2D1I1D", "0^AC0^G0"),
]


def brute_md(ref, seq, final):
    """MD by brute force on the expanded CIGAR over the LETTERS (the style of fc.brute_nm): an M position matches when both
    letters are the same one of ACGT; a reference letter prints as itself when it is one of ACGT and as N otherwise; a
    position beyond either string counts as N.  Returns (text, letters not behind '^', letters behind '^', bases under I)."""
    ops = "".join(op * int(n) for n, op in re.findall(r"(\d+)([MIDNS=X])", final))
    show = lambda a: ref[a] if a < len(ref) and ref[a] in "ACGT" else "N"
    out, u, a, b, subs, dels, ins, in_del = [], 0, 0, 0, 0, 0, 0, False
    for op in ops:
        if op in "M=X":
            in_del = False
            if a < len(ref) and b < len(seq) and ref[a] == seq[b] and ref[a] in "ACGT":
                u += 1
            else:
                out.append(f"{u}{show(a)}")
                u, subs = 0, subs + 1
            a, b = a + 1, b + 1
        elif op == "D":
            if not in_del:
                out.append(f"{u}^")
                u, in_del = 0, True
            out.append(show(a))
            a, dels = a + 1, dels + 1
        elif op == "I":
            in_del = False                                       # (D I D: two deletions, `^` twice)
            b, ins = b + 1, ins + 1
        elif op == "N":
            in_del = False
            a += 1
        else:
            in_del = False
            b += 1
    return "".join(out) + str(u), subs, dels, ins


def rebuild_reference(md, seq, final):
    """The reference under the alignment from MD, the read (without its soft clips) and the CIGAR -- what pysam's
    get_reference_sequence() does: a match takes the read's base, a mismatch and a deletion the letters MD names."""
    toks = re.findall(r"\d+|\^[A-Z]+|[A-Z]", md)
    assert "".join(toks) == md, md
    out, b, t, left = [], 0, 0, 0                                # left: matches of the current number not yet used
    for n, op in re.findall(r"(\d+)([MIDNS=X])", final):
        n = int(n)
        if op in "M=X":
            while n > 0:
                if left == 0:
                    while t < len(toks) and toks[t].isdigit() and int(toks[t]) == 0:
                        t += 1
                    if toks[t].isdigit():
                        left = int(toks[t])
                        t += 1
                        continue
                    assert not toks[t].startswith("^"), (md, final)
                    out.append(toks[t])
                    t, b, n = t + 1, b + 1, n - 1
                    continue
                k = min(left, n)
                out.append(seq[b:b + k])
                left, b, n = left - k, b + k, n - k
        elif op == "D":
            assert left == 0
            while toks[t].isdigit() and int(toks[t]) == 0:
                t += 1
            assert toks[t].startswith("^") and len(toks[t]) == n + 1, (md, final, toks[t])
            out.append(toks[t][1:])
            t += 1
        elif op in "IS":
            b += n
    assert left == 0 and all(x == "0" for x in toks[t:]), (md, final)
    return "".join(out)


def parse_tags(aux):
    """[(tag, type, value bytes)] of a record's aux block, in order"""
    out, q = [], 0
    while q < len(aux):
        n = bam._aux_value_len(aux, q + 3, aux[q + 2:q + 3])
        assert n is not None, aux[q:q + 8]
        out.append((aux[q:q + 2], aux[q + 2:q + 3], aux[q + 3:q + 3 + n]))
        q += 3 + n
    return out


def md_and_nm(rec):
    """(MD text, NM, offset of the MD tag in the record, names of the tags in order) of a FULL record with the tag"""
    f, name, words, body, aux = fc.parse_full(rec)
    tags = parse_tags(aux)
    names = [t for t, _, _ in tags]
    k = names.index(b"MD")
    assert names[k - 1] == b"NM" and tags[k][1] == b"Z" and names.count(b"MD") == 1 and names.count(b"NM") == 1
    nm = int.from_bytes(tags[k - 1][2], "little")
    at = len(rec) - len(aux) + sum(3 + len(v) for _, _, v in tags[:k])
    return tags[k][2][:-1].decode(), nm, at, names


def want_stream(raws, records, contigs, finals, status, md=True):
    """bam.full_record(md=) of every kept read, one after the other.  contigs: {name: bases}, a record's `_ctg` names its own"""
    out = []
    for raw, rec, fin, st in zip(raws, records, finals, status):
        if st & 32:
            continue
        rc, sc, _ = lc.expected_pack(rec, rec["cigar"], contigs[rec.get("_ctg", "ctg")])
        out.append(bam.full_record(raw, rc, sc, fin, md=md))
    return b"".join(out)


def table_reads():
    """The TABLE's rows as reads on a contig that holds each row's reference: (references, refs, records, finals, [MD])"""
    contig, records, finals = "", [], []
    for k, (ref, seq, fin, _) in enumerate(TABLE):
        pos = len(contig) + 3
        contig += "TTT" + ref + "GG"
        cig = [("MID".index(op), int(n)) for n, op in re.findall(r"(\d+)([MID])", fin)]
        records.append(dict(name=f"t{k}", flag=0, ref_id=0, pos=pos, mapq=20, cigar=cig, seq=seq, qual=bytes(len(seq)) if seq else None,
                            tags=b"MDZ99\0RGZg\0" if k % 2 else b"", _status=0))
        finals.append(fin)
    contig += "ACGT" * 5
    return [("ctg", len(contig))], {"ctg": contig}, records, finals, [t[3] for t in TABLE]


_CRAFTED = {}


def crafted_reads(seed=11):
    """The smallest shapes at which the walk can go wrong -- (references, refs, records, finals, {name: MD pinned by hand}).
    Word counts 1, 63, 64, 65, 129; M runs of 1, 63, 64, 65, 200 with mismatches at run offsets 0, 63, 64 and last; 130
    mismatches in a row; a match count that crosses a round, an I word and a tile border; counts of 9 ... 10 000; 100001M on
    a contig of its own; deletions of 1, 63, 64, 65, 300; a deletion first and last; a mismatch directly behind and in front
    of a deletion; D I D; N in the reference under M and D; a final that runs past the reference array; all-I, all-D; a
    refused read; a read with no final words; four reads whose names move the tag over every byte alignment.  The result is
    computed once and shared (nobody changes it)."""
    if seed in _CRAFTED:
        return _CRAFTED[seed]
    rng = np.random.default_rng(seed)
    contig = list(lc.random_contig(rng, 72000))
    for p in (5003, 5007, 5008):
        contig[p] = "N"
    contig = "".join(contig)
    big = lc.random_contig(rng, 100101)
    records, finals, pinned = [], [], {}
    ref_at = lambda ctg, pos, n: (contig if ctg == "ctg" else big)[pos:pos + n]

    def add(name, pos, runs, edits=(), clips=([], []), seq_sub=None, status=0, rec_cigar=None, final=None, ctg="ctg", tags=None):
        """runs: the FINAL CIGAR as [(op, len)]; the read is the contig under it with `edits` (query offsets) substituted.
        rec_cigar: the record's own CIGAR where it is not the final one (the code arrays follow the record's)."""
        seq, at = [], pos
        for op, ln in runs:
            if op == M:
                seq += list(ref_at(ctg, at, ln))
            elif op == I:
                seq += list(lc.random_contig(rng, ln))
            if op in (M, D):
                at += ln
        for e in edits:
            seq[e] = other(seq[e])
        for e, c in (seq_sub or {}).items():
            seq[e] = c
        nl, nt = sum(n for op, n in clips[0] if op == S), sum(n for op, n in clips[1] if op == S)
        k = len(records)
        if tags is None:
            tags = (b"", b"RGZgrp\0", b"MDZ3A3\0PSi" + struct.pack("<i", k), b"NMC\x07XZZ" + b"a" * (k % 5) + b"\0")[k % 4]
        rec = dict(name=name, flag=0, ref_id=0 if ctg == "ctg" else 1, pos=pos, mapq=40, seq="G" * nl + "".join(seq) + "T" * nt,
                   cigar=clips[0] + list(rec_cigar if rec_cigar is not None else runs) + clips[1],
                   qual=bytes(rng.integers(0, 50, nl + len(seq) + nt).tolist()) if seq or nl or nt else None, tags=tags,
                   _status=status, _ctg=ctg)
        records.append(rec)
        finals.append(final if final is not None else "".join(f"{ln}{'MID'[op]}" for op, ln in runs))

    pos = 100
    for n_ops in (1, 63, 64, 65, 129):                           # M I M D M ... of n_ops operations
        runs = [((M, I, M, D)[j % 4], (7, 1, 5, 2)[j % 4]) for j in range(n_ops)]
        if runs[-1][0] != M:
            runs[-1] = (M, 3)
        add(f"ops{n_ops}", pos, runs, edits=(0,), clips=([(S, 3)], [(S, 2), (H, 4)]) if n_ops != 64 else ([], []))
        pos += 700
    for ln in (1, 63, 64, 65, 200):                              # one long M run between two short ones
        offs = sorted({o for o in (0, 63, 64, ln - 1) if o < ln})
        add(f"run{ln}", pos, [(M, 4), (I, 2), (M, ln), (D, 3), (M, 6)], edits=tuple(6 + o for o in offs), clips=([(H, 2), (S, 1)], []))
        pos += 400
    add("mis130", pos, [(M, 130)], edits=tuple(range(130)))
    pinned["mis130"] = "".join("0" + c for c in contig[pos:pos + 130]) + "0"
    pos += 300
    # 4 matches behind the first event, 70 x (2M 1I) without one -- a tile border and 70 I words --, 80 more in a 90M: 4 + 140 + 80
    add("carry", pos, [(M, 5)] + [(M, 2), (I, 1)] * 70 + [(M, 90)], edits=(0, 5 + 210 + 80))
    pinned["carry"] = f"0{contig[pos]}224{contig[pos + 225]}9"
    pos += 500
    counts = (9, 10, 99, 100, 999, 1000, 9999, 10000)            # a mismatch, then that many matches, ..., a closing mismatch
    at, ed = 0, []
    for c in counts:
        ed.append(at)
        at += 1 + c
    ed.append(at)
    add("counts", pos, [(M, at + 1)], edits=tuple(ed))
    pinned["counts"] = "0" + "".join(f"{contig[pos + e]}{c}" for e, c in zip(ed, counts)) + f"{contig[pos + at]}0"
    pos += at + 100
    for nd in (1, 63, 64, 65, 300):
        add(f"del{nd}", pos, [(M, 5), (D, nd), (M, 5)])
        pinned[f"del{nd}"] = f"5^{contig[pos + 5:pos + 5 + nd]}5"
        pos += 500
    add("del_first", pos, [(D, 3), (M, 10)])
    pinned["del_first"] = f"0^{contig[pos:pos + 3]}10"
    add("del_last", pos + 100, [(M, 10), (D, 3)])
    pinned["del_last"] = f"10^{contig[pos + 110:pos + 113]}0"
    add("mis_around_del", pos + 200, [(M, 10), (D, 2), (M, 10)], edits=(9, 10))
    p = pos + 200
    pinned["mis_around_del"] = f"9{contig[p + 9]}0^{contig[p + 10:p + 12]}0{contig[p + 12]}9"
    add("did", pos + 300, [(M, 4), (D, 2), (I, 1), (D, 1), (M, 4)])
    p = pos + 300
    pinned["did"] = f"4^{contig[p + 4:p + 6]}0^{contig[p + 6]}4"
    add("did_only", pos + 400, [(D, 2), (I, 1), (D, 1)])
    p = pos + 400
    pinned["did_only"] = f"0^{contig[p:p + 2]}0^{contig[p + 2]}0"
    add("n_in_ref", 5000, [(M, 5), (D, 6), (M, 9)])              # contig N at 5003 (under M), 5007 and 5008 (under D)
    pinned["n_in_ref"] = f"3N1^{contig[5005:5007]}NN{contig[5009:5011]}9"
    add("r_in_read", 6100, [(M, 20)], seq_sub={7: "R"})           # an IUPAC letter in the read: a mismatch, the reference's letter
    pinned["r_in_read"] = f"7{contig[6107]}12"
    # the record covers 20 reference bases and has 20 query bases; the final names 35 and 30: N beyond both arrays
    add("past_end", 6000, [(M, 20)], rec_cigar=[(M, 20)], final="20M5D10M")
    pinned["past_end"] = "20^NNNNN" + "0N" * 10 + "0"
    add("all_i", 7000, [(I, 40)])
    pinned["all_i"] = "0"
    add("all_d", 7100, [(D, 40)])
    pinned["all_d"] = f"0^{contig[7100:7140]}0"
    add("refused", 7200, [(M, 30)], status=32)
    add("no_words", 7300, [(M, 10)], rec_cigar=[(M, 10)], final="", clips=([(S, 2)], []))
    pinned["no_words"] = "0"
    for k, name in enumerate(("a", "al", "aln", "alnx")):        # the same read under names of 1 ... 4 letters; MD of 1 ... 4 bytes
        p = 7400 + 200 * k
        ln = (8, 12, 120, 17)[k]
        add(name, p, [(M, ln)], edits=((), (), (), (5,))[k], tags=b"")
        pinned[name] = (f"{ln}", f"{ln}", f"{ln}", f"5{contig[p + 5]}11")[k]
    add("m100001", 50, [(M, 100001)], ctg="big", tags=b"RGZbig\0")
    pinned["m100001"] = "100001"
    both = sorted(zip(records, finals), key=lambda rf: (rf[0]["ref_id"], rf[0]["pos"]))      # (coordinate order: the file gets an index)
    out = ([("ctg", len(contig)), ("big", len(big))], {"ctg": contig, "big": big}, [r for r, _ in both], [f for _, f in both], pinned)
    _CRAFTED[seed] = out
    return out


def letters_of(rec, contigs, final):
    """(reference letters under the record's own CIGAR, read letters without the soft clips) of a crafted record"""
    rc, sc, _ = lc.expected_pack(rec, rec["cigar"], contigs[rec.get("_ctg", "ctg")])
    lead = sum(n for op, n in rec["cigar"][:2] if op == S)
    return contigs[rec.get("_ctg", "ctg")][rec["pos"]:rec["pos"] + len(rc)], rec["seq"][lead:lead + len(sc)]


def random_reads(seed=21, n_reads=2000, contig_len=34000):
    """(references, refs, records, finals, [(ref codes, seq codes)]): random M / I / D finals of 1 ... 200 words with lengths of
    1 ... 150 (both drawn log-uniformly: every size occurs, most reads stay small), random substitutions under M."""
    rng = np.random.default_rng(seed)
    arr = rng.integers(1, 5, contig_len).astype(np.uint8)
    contig = "".join("NACGT"[x] for x in arr)
    log_uniform = lambda hi, n: np.minimum(hi, np.exp(rng.uniform(0, np.log(hi + 1), n)).astype(np.int64))
    n_words = log_uniform(200, n_reads)
    n_words[:4] = (1, 200, 64, 65)
    records, finals, arrays = [], [], []
    for k in range(n_reads):
        ops = rng.integers(0, 3, n_words[k])
        lens = log_uniform(150, n_words[k])
        if k == 1:
            lens[:] = 150
        runs = []
        for op, ln in zip(ops.tolist(), lens.tolist()):          # (neighbouring words of one operation stay apart: the walk takes words as they come)
            runs.append((op, ln))
        rl = sum(ln for op, ln in runs if op != I)
        pos = int(rng.integers(0, contig_len - rl))
        ref = arr[pos:pos + rl]
        seq, a = [], 0
        for op, ln in runs:
            if op == M:
                piece = ref[a:a + ln].copy()
                hit = rng.random(ln) < (0.5 if k % 7 == 0 else 0.04)
                piece[hit] = (piece[hit] - 1 + rng.integers(1, 4, int(hit.sum()))) % 4 + 1
                seq.append(piece)
            elif op == I:
                seq.append(rng.integers(1, 5, ln).astype(np.uint8))
            if op != I:
                a += ln
        sq = np.concatenate(seq) if seq else np.zeros(0, np.uint8)
        records.append(dict(name=f"q{k}", flag=0, ref_id=0, pos=pos, mapq=7, cigar=runs, seq="".join("NACGT"[x] for x in sq),
                            qual=None, tags=b"", _status=0))
        finals.append("".join(f"{ln}{'MID'[op]}" for op, ln in runs))
        arrays.append((ref, sq))
    order = sorted(range(n_reads), key=lambda k: records[k]["pos"])
    return [("ctg", contig_len)], {"ctg": contig}, [records[k] for k in order], [finals[k] for k in order], [arrays[k] for k in order]
