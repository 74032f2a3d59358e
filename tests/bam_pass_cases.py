"""Inputs shared by tests/test_bam_pass.py and tests/test_gpu_bam_pass.py (--pass_through): ONE file of 40 records on two
contigs -- primary reads with soft clips on both ends among records the realigner does not take (secondary, supplementary,
placed but unmapped) of every shape the pass-through has to copy, and one read align() refuses --, written by a writer of
this module's own; the parse of what it wrote; and the rule of csrc/staged_head.hpp (a record PASSES iff flag & mask != 0)
with the selection rule of npore_bam_select_pass restated in Python.  Every expectation is the input's own bytes or follows
from the rule, none from a run."""
import struct
import zlib

import numpy as np

from npore_amd import synth
import long_cigar_cases as lc

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
SEQ16 = "=ACMGRSVTWYHKDBN"
PASS_FLAGS = 0x100 | 0x800 | 0x4
ST_PASSED = 128
p32 = lambda v: struct.pack("<I", v)
BIG_ML = 70000                                                   # bytes of the ML:B,C array: the record spans two output members


def passes(flag, mask):
    return (flag & mask) != 0


def write_bam(path, references, records):
    """A BAM of records given as dicts: name, flag, ref_id, pos, mapq, cigar [(op, len)], seq, qual (bytes / None), tags (raw
    bytes), bin; placeholder: the CIGAR field holds `<l_seq>S<reflen>N` and a CG:B,I tag with the words follows `tags`."""
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in references)
    out = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(references)))
    for n, l in references:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    code = {c: i for i, c in enumerate(SEQ16)}
    for r in records:
        name = r["name"].encode() + b"\0"
        nib = [code[c] for c in r["seq"]] + ([0] if len(r["seq"]) & 1 else [])
        packed = bytes(nib[k] << 4 | nib[k + 1] for k in range(0, len(nib), 2))
        qual = bytes([0xFF]) * len(r["seq"]) if r.get("qual") is None else bytes(r["qual"])
        words = b"".join(p32(ln << 4 | op) for op, ln in r["cigar"])
        aux = r.get("tags", b"")
        if r.get("placeholder"):
            aux += b"CGBI" + p32(len(r["cigar"])) + words
            words = p32(len(r["seq"]) << 4 | S) + p32(lc.ref_len(r["cigar"]) << 4 | N)
        body = struct.pack("<iiBBHHHiiii", r["ref_id"], r["pos"], len(name), r.get("mapq", 60), r.get("bin", 4681), len(words) // 4, r["flag"],
                           len(r["seq"]), r.get("next_ref_id", -1), r.get("next_pos", -1), r.get("tlen", 0)) + name + words + packed + qual + aux
        out += struct.pack("<i", len(body)) + body
    with open(path, "wb") as fh:
        for p in range(0, len(out), 0xFF00):
            chunk = bytes(out[p:p + 0xFF00])
            comp = zlib.compressobj(1, zlib.DEFLATED, -15)
            data = comp.compress(chunk) + comp.flush()
            fh.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(data) + 25) + data +
                     struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def runs_of(expanded):
    """[(op, len)] over M / I / D of an expanded op string over =XMID (= and X are M)"""
    text = expanded.decode() if isinstance(expanded, (bytes, bytearray)) else expanded
    out = []
    for ch in text:
        op = {"=": M, "X": M, "M": M, "I": I, "D": D}[ch]
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return [(op, n) for op, n in out]


def pass_file(seed=23):
    """(references, {contig: bases}, records).  The order in the file, k = index (every record lies on a contig, so with the whole
    mask k is its index in the selection too):
       0      a secondary with SEQ `*` (l_seq = 0): a passed record FIRST in the file
       1 - 3  primaries
       4      a supplementary with hard clips on both ends and an odd l_seq
       5 - 6  primaries
       7      a flag-0x4 record with refID >= 0 and no CIGAR (UNMAPPED_AT: its position, a region's start in the tests)
       8 - 10 primaries
       11     a supplementary with stale NM, MD, cs tags and an ML:B,C array of 70 000 bytes
       12     a primary whose CIGAR and sequence lengths disagree: refused
       13 - 15 primaries
       16 - 19 four passed records in a row: at batch_reads = 4 a batch with no read to align
       20 - 24 primaries; contig 1 from 25 on:
       25 - 29 primaries
       30     a secondary written as a long-CIGAR placeholder with a CG:B,I tag of three words
       31 - 38 primaries
       39     a supplementary: a passed record LAST in the file
    Primaries carry soft clips on both ends (3 / 2, odd / even by turns), some an H outside, stale tags among kept ones, mate
    fields; name lengths (with the NUL) run 1 ... 8, so records start at every alignment mod 4."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(200, 2001, 40)
    refs, seqs, cigs = [], [], []
    for k in range(40):
        rf, sq, cg = synth.make_batch(seed * 100 + k, 1, ref_len=int(lens[k]), p_np=0.1)
        refs.append(rf[0]); seqs.append(sq[0]); cigs.append(cg[0])
    dec = lambda a: "".join("NACGT"[x] for x in a)
    kinds = {0: "sec_star", 4: "supp_hard", 7: "unmapped", 11: "supp_big", 12: "refused", 16: "sec", 17: "supp", 18: "unmapped2", 19: "sec",
             30: "sec_cg", 39: "supp"}
    contigs, records = [[], []], []
    for k in range(40):
        c = 0 if k < 25 else 1
        contig = contigs[c]
        pos = len(contig) + 30
        contig += list(lc.random_contig(rng, 30)) + list(dec(refs[k]))
        runs = runs_of(cigs[k])
        body = dec(seqs[k])
        kind = kinds.get(k, "primary")
        name = chr(97 + k % 26) * (k % 8)                       # l_read_name = 1 ... 8 (an empty name is `\0`)
        rec = dict(name=name, ref_id=c, pos=pos, mapq=k, next_ref_id=c, next_pos=pos + 11, tlen=300 + k, _kind=kind, bin=k)
        if kind in ("primary", "refused"):
            lead, trail = (3, 2) if k % 2 else (2, 5)
            cig = ([(H, 4)] if k % 5 == 0 else []) + [(S, lead)] + runs + [(S, trail)] + ([(H, 1)] if k % 3 == 0 else [])
            if kind == "refused":
                cig = cig[:-1] + [(M, 7)] + cig[-1:]
            n = lead + len(body) + trail
            rec.update(flag=16 if k % 4 == 1 else 0, cigar=cig, seq="A" * lead + body + "C" * trail,
                       qual=None if k % 6 == 0 else bytes(rng.integers(0, 60, n).tolist()),
                       tags=b"RGZgrp\0" + b"NMC\x05" + b"HPC\x01" + b"MDZ10A5\0" + b"PSi" + struct.pack("<i", k))
        elif kind == "sec_star":
            rec.update(flag=0x100, cigar=runs, seq="", qual=b"", tags=b"NMC\x02" + b"tpAS")
        elif kind == "supp_hard":
            lead = [] if len(body) % 2 else [(S, 1)]            # (an odd l_seq either way)
            odd = body if len(body) % 2 else "G" + body
            rec.update(flag=0x800, cigar=[(H, 5)] + lead + runs + [(H, 7)], seq=odd, qual=bytes(rng.integers(0, 60, len(odd)).tolist()),
                       tags=b"SAZctg0,1,+,5S,60,0;\0")
        elif kind in ("unmapped", "unmapped2"):
            rec.update(flag=0x4 | 0x1 | 0x8 if kind == "unmapped2" else 0x4, cigar=[], seq=body[:101], qual=bytes(rng.integers(0, 40, 101).tolist()),
                       mapq=0, tags=b"RGZgrp\0")
        elif kind == "supp_big":
            rec.update(flag=0x800 | 16, cigar=[(S, 4)] + runs, seq="G" * 4 + body, qual=bytes(rng.integers(0, 60, 4 + len(body)).tolist()),
                       tags=b"NMS\x2c\x01" + b"MDZ3^AC5\0" + b"csZ:3-ac:5\0" + b"MLBC" + p32(BIG_ML) + bytes(rng.integers(0, 256, BIG_ML).astype(np.uint8)) +
                            b"def" + struct.pack("<f", 0.125) + b"dvf" + struct.pack("<f", 0.25))
        elif kind == "sec_cg":
            three = [(M, 40), (D, 2), (M, 60)]
            rec.update(flag=0x100, cigar=three, seq=body[:100], qual=None, placeholder=True, tags=b"XAAq")
        else:                                                   # a plain secondary / supplementary
            rec.update(flag=0x100 if kind == "sec" else 0x800, cigar=[(S, 1)] + runs, seq="T" + body,
                       qual=bytes(rng.integers(0, 60, 1 + len(body)).tolist()), tags=b"NMC\x00" + b"RGZgrp\0")
        records.append(rec)
    refs_out = {f"ctg{c}": "".join(s) + "ACGT" * 10 for c, s in enumerate(contigs)}
    references = [(n, len(s)) for n, s in refs_out.items()]
    return references, refs_out, records


UNMAPPED_AT = 7                                                  # the index of the flag-0x4 record the region tests cut at


def finals_of(records):
    """the input's own collapsed CIGARs without the clips: the finals the host tests supply ("" for the refused read)"""
    return ["" if r["_kind"] == "refused" else lc.collapsed(r["cigar"]) for r in records]


def parse(rec):
    """(ref_id, pos, flag, reference length of the record's own CIGAR words) of a record, block_size word first"""
    rid, pos, l_rn, _mq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    words = struct.unpack_from(f"<{n_cig}I", rec, 36 + l_rn)
    return rid, pos, flag, sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8))


def py_select(raws, regions, max_reads, mask):
    """npore_bam_select_pass's rule over the parsed stream: per region (ref_id, start, stop) the records on that contig that
    overlap it, in file order; a record that passes and has no reference length overlaps as if its length were 1; the cap is
    looked at in front of the flag filter, as get_read_data has it; what is neither a read nor passes is dropped."""
    kept = []
    for rid, start, stop in regions:
        for i, raw in enumerate(raws):
            r_id, pos, flag, rl = parse(raw)
            if r_id != rid:
                continue
            if rl == 0 and passes(flag, mask):
                rl = 1
            if not (pos < stop and pos + rl > start):
                continue
            if max_reads and len(kept) >= max_reads:
                return kept
            if flag & (PASS_FLAGS & ~mask):
                continue
            kept.append(i)
    return kept


def compose(raws, flags, mask, idx, refused, rest_records):
    """The stream a pass-through run owes: for the selected indices `idx` in order, the input's bytes where the record passes,
    nothing for a read in `refused`, and otherwise the next of `rest_records` -- the FULL records of the reads among idx, in
    order, the refused ones left out."""
    it = iter(rest_records)
    out = []
    for i in idx:
        if passes(flags[i], mask):
            out.append(raws[i])
        elif i not in refused:
            out.append(next(it))
    assert next(it, None) is None
    return out
