"""BAM in / SAM out around align(): counterparts of reference src/bam.pyx:18-89,
127-145 (get_read_data, realign_read, create_header) and src/util.py:16-93
(get_bam_regions), with a batch in the middle instead of one align() per call.

pysam is not needed: BAM is BGZF (concatenated gzip members) around a simple
binary record stream; the reference bases come from the FASTA slice
[reference_start, reference_start + reference_length), which is what pysam's
get_reference_sequence() reconstructs from the MD tag.

Two implementations of the same logic live here:
  * NativeBam / NativeFasta / realign_native: thin ctypes wrappers of the library's
    C++ host I/O (csrc/hostio.hpp, csrc/bam_reader.hpp: parallel BGZF inflate, batch packing, SAM
    formatting) -- what realign.py runs;
  * BamFile / read_fasta / get_read_data / realign_reads: the pure-Python
    restatement, record by record as the reference does it -- what the tests
    compare the native path with.
write_bam() makes small BAM files for tests and benchmarks.
"""
import dataclasses
import os
import struct
import sys
import zlib

import numpy as np

from . import cfg
from .cig import bases_to_int, expand_cigar, standardize_batch

_SEQ16 = "=ACMGRSVTWYHKDBN"
_CIGOPS = "MIDNSHP=XB"


def read_fasta(path):
    """{contig: sequence} (upper-cased), contigs in file order."""
    try:
        fh = open(path)
    except (IOError, OSError):
        print(f"\nERROR: could not open --ref FASTA '{path}'.")
        sys.exit(1)
    seqs, name, parts = {}, None, []
    with fh:
        for line in fh:
            if line.startswith(">"):
                if name is not None:
                    seqs[name] = "".join(parts).upper()
                name, parts = line[1:].split()[0], []
            else:
                parts.append(line.strip())
    if name is not None:
        seqs[name] = "".join(parts).upper()
    return seqs


def _bgzf_decompress(path):
    try:
        raw = open(path, "rb").read()
    except FileNotFoundError:
        print(f"\nERROR: BAM file '{path}' not found.")      # reference src/bam.pyx:22-24
        sys.exit(1)
    out, pos = [], 0
    while pos < len(raw):
        d = zlib.decompressobj(31)
        out.append(d.decompress(raw[pos:]))
        used = len(raw) - pos - len(d.unused_data)
        if used <= 0:
            break
        pos += used
    return b"".join(out)


class BamRecord:
    __slots__ = ("query_name", "flag", "ref_id", "reference_start", "mapping_quality", "cigar", "seq", "qual", "hp")


MAX_CIGAR_OPS = 0xFFFF               # what n_cigar_op holds; more operations go into the CG tag


def resolve_long_cigar(cigar, l_seq, ref_id, pos, aux):
    """The real CIGAR of a record (SAM specification 4.2.2, the rule of csrc/hostio.hpp rec_cigar): `cigar` [(op, len)]
    unless it begins with `<l_seq>S`, the record is placed and its tags `aux` hold CG:B,I (or B,i) with at least as many
    words as `cigar` has operations (and fewer than 2^29), all inside the record -- then those words."""
    if not cigar or cigar[0] != (4, l_seq) or l_seq >= 1 << 28 or ref_id < 0 or pos < 0:
        return cigar
    q, end = 0, len(aux)
    while q + 3 <= end:
        tag, typ = aux[q:q + 2], chr(aux[q + 2])
        q += 3
        if typ in "cCA":
            w = 1
        elif typ in "sS":
            w = 2
        elif typ in "iIf":
            w = 4
        elif typ in "ZH":
            z = aux.find(b"\0", q)
            w = (z if z >= 0 else end) - q + 1
        elif typ == "B" and end - q >= 5 and chr(aux[q]) in "cCsSiIf":
            w = 5 + struct.unpack_from("<I", aux, q + 1)[0] * {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(aux[q]), 4)
        else:
            return cigar
        if w > end - q:
            return cigar
        if tag == b"CG":
            if typ != "B" or chr(aux[q]) not in "Ii":
                return cigar
            n, = struct.unpack_from("<I", aux, q + 1)
            if n < len(cigar) or n >= 1 << 29:
                return cigar
            return [(c & 15, c >> 4) for c in struct.unpack_from(f"<{n}I", aux, q + 5)]
        q += w
    return cigar


class BamFile:
    """Minimal reader: header text, reference names/lengths, all records (a long CIGAR resolved from its CG tag)."""

    def refs_with_reads(self):
        return {r.ref_id for r in self.records if r.ref_id >= 0}

    def __init__(self, path):
        data = _bgzf_decompress(path)
        if data[:4] != b"BAM\1":
            print(f"\nERROR: '{path}' is not a BAM file.")
            sys.exit(1)
        l_text, = struct.unpack_from("<i", data, 4)
        self.text = data[8:8 + l_text].decode(errors="replace").rstrip("\0")
        p = 8 + l_text
        n_ref, = struct.unpack_from("<i", data, p)
        p += 4
        self.references, self.lengths = [], []
        for _ in range(n_ref):
            l_name, = struct.unpack_from("<i", data, p)
            name = data[p + 4:p + 4 + l_name - 1].decode()
            l_ref, = struct.unpack_from("<i", data, p + 4 + l_name)
            self.references.append(name)
            self.lengths.append(l_ref)
            p += 8 + l_name
        self.records = []
        while p + 4 <= len(data):
            block_size, = struct.unpack_from("<i", data, p)
            q = p + 4
            ref_id, pos, l_rn, mapq, _bin, n_cig, flag, l_seq, _nref, _npos, _tlen = struct.unpack_from("<iiBBHHHiiii", data, q)
            q += 32
            r = BamRecord()
            r.query_name = data[q:q + l_rn - 1].decode()
            q += l_rn
            cig = struct.unpack_from(f"<{n_cig}I", data, q)
            q += 4 * n_cig
            r.cigar = [(c & 15, c >> 4) for c in cig]
            sb = np.frombuffer(data, np.uint8, (l_seq + 1) // 2, q)
            q += (l_seq + 1) // 2
            nib = np.empty(2 * len(sb), np.uint8)
            nib[0::2] = sb >> 4
            nib[1::2] = sb & 15
            r.seq = "".join(_SEQ16[x] for x in nib[:l_seq])
            r.qual = data[q:q + l_seq]
            q += l_seq
            r.hp = None
            end = p + 4 + block_size
            r.cigar = resolve_long_cigar(r.cigar, l_seq, ref_id, pos, bytes(data[q:end]))
            while q + 3 <= end:      # optional fields: find HP
                tag, typ = data[q:q + 2], chr(data[q + 2])
                q += 3
                if typ in "cCsSiI":
                    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ]
                    val, = struct.unpack_from(fmt, data, q)
                    q += struct.calcsize(fmt)
                    if tag == b"HP":
                        r.hp = int(val)
                elif typ == "A":
                    q += 1
                elif typ == "f":
                    q += 4
                elif typ in "ZH":
                    z = data.index(b"\0", q)
                    q = z + 1
                elif typ == "B":
                    sub = chr(data[q]); cnt, = struct.unpack_from("<i", data, q + 1)
                    q += 5 + cnt * {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[sub]
                else:
                    break
            r.flag, r.ref_id, r.reference_start, r.mapping_quality = flag, ref_id, pos, mapq
            self.records.append(r)
            p = end


def get_bam_regions(bam, ref_seqs):
    """cfg.args.regions = [(contig, start, end)], reference src/util.py:16-93."""
    a = cfg.args
    if getattr(a, "contig", None):
        if a.contig not in ref_seqs:
            print(f"ERROR: contig '{a.contig}' not present in '{a.ref}'. Valid contigs are: {list(ref_seqs)}")
            sys.exit(1)
        if getattr(a, "contigs", None):
            print("\nERROR: can't set 'contig' and 'contigs'.")
            sys.exit(1)
        beg = a.contig_beg or 0
        max_end = len(ref_seqs[a.contig]) - 1
        end = a.contig_end or max_end
        a.regions = [(a.contig, beg, min(max_end, end))]
    elif getattr(a, "contigs", None):
        if a.contig_beg or a.contig_end:
            print("\nERROR: can't set start/endpoints with multiple contigs.")
            sys.exit(1)
        a.regions = []
        for ctg in a.contigs.split(","):
            if ctg not in ref_seqs:
                print(f"ERROR: contig '{ctg}' not present in '{a.ref}'. Valid contigs are: {list(ref_seqs)}")
                sys.exit(1)
            a.regions.append((ctg, 0, len(ref_seqs[ctg]) - 1))
    elif getattr(a, "bed", None):
        try:
            a.regions = [(c, int(s), int(e)) for c, s, e in (x.strip().split()[:3] for x in open(a.bed) if x.strip())]
        except FileNotFoundError:
            print("\nERROR: could not open 'cfg.args.bed' BED.")
            sys.exit(1)
    else:
        if getattr(a, "contig_beg", None) or getattr(a, "contig_end", None):
            print("\nERROR: 'contig' not supplied, but start/endpoints set.")
            sys.exit(1)
        a.regions = []
        with_reads = bam.refs_with_reads()
        for k, (ctg, l) in enumerate(zip(bam.references, bam.lengths)):
            if ctg not in ref_seqs:
                print(f"WARNING: contig '{ctg}' present in '{a.bam}', but not '{a.ref}', skipping...")
            elif k in with_reads:
                a.regions.append((ctg, 0, l - 1))
    return a.regions


def get_read_data(bam, ref_seqs):
    """Generator of the reference's 11-tuples (src/bam.pyx:18-47): primary mapped reads
    overlapping cfg.args.regions, soft clips trimmed off sequence and qualities."""
    kept = 0
    name_to_id = {n: i for i, n in enumerate(bam.references)}
    for ctg, start, stop in cfg.args.regions:
        rid = name_to_id.get(ctg, -2)
        for r in bam.records:
            if r.ref_id != rid:
                continue
            ref_len = sum(n for op, n in r.cigar if op in (0, 2, 3, 7, 8))
            if not (r.reference_start < stop and r.reference_start + ref_len > start):
                continue
            if cfg.args.max_reads and kept >= cfg.args.max_reads:
                return
            if r.flag & (0x100 | 0x800 | 0x4):          # secondary, supplementary, unmapped
                continue
            kept += 1
            lead = r.cigar[0][1] if r.cigar and r.cigar[0][0] == 4 else 0
            if len(r.cigar) > 1 and r.cigar[0][0] == 5 and r.cigar[1][0] == 4:
                lead = r.cigar[1][1]
            trail = r.cigar[-1][1] if len(r.cigar) > 1 and r.cigar[-1][0] == 4 else 0
            if len(r.cigar) > 2 and r.cigar[-1][0] == 5 and r.cigar[-2][0] == 4:
                trail = r.cigar[-2][1]
            qend = len(r.seq) - trail
            quals = "*" if (not r.qual or r.qual[0] == 0xFF) else "".join(chr(33 + x) for x in r.qual[lead:qend])
            yield (r.query_name, r.flag, ctg, r.reference_start, r.mapping_quality,
                   "".join(f"{n}{_CIGOPS[op]}" for op, n in r.cigar), r.reference_start + ref_len,
                   r.seq[lead:qend].upper(), quals,
                   ref_seqs[ctg][r.reference_start:r.reference_start + ref_len].upper(),
                   0 if r.hp is None else int(r.hp))


def header_text(bam):
    """The header the reference writes through pysam (src/bam.pyx:127-145)."""
    return ("@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{name}\tLN:{l}\n" for name, l in zip(bam.references, bam.lengths)) +
            f"@PG\tPN:realigner\tID:realigner\tVN:{cfg.__version__}\tCL:{' '.join(sys.argv)}\n")


def create_header(outfile, bam):
    """SAM header as the reference writes it through pysam (src/bam.pyx:127-145); truncates."""
    if os.path.dirname(outfile):
        os.makedirs(os.path.dirname(outfile), exist_ok=True)
    with open(outfile, "w") as fh:
        fh.write(header_text(bam))


# ---- BAM out (--out_format bam): the pure-Python statement of csrc/bam_reader.hpp's RECORD / FILE / INDEX rules ----
BGZF_STORED_PAYLOAD = 0xFF00         # payload bytes of a member; a stored member is its payload + 31 bytes
PART_BASE = 65536                    # where the index sidecar of a rank's part takes the part to begin (NPORE_PART_BASE)
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def reg2bin(beg, end):
    """SAM specification 5.3: the bin of [beg, end)."""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def hp_tag(hp):
    """The HP tag in the smallest integer type that holds it, htslib's order: C, S, I from 0 up, c, s, i below."""
    hp = int(hp)
    if hp >= 0:
        typ, fmt = ("C", "<B") if hp <= 0xFF else ("S", "<H") if hp <= 0xFFFF else ("I", "<I")
    else:
        typ, fmt = ("c", "<b") if hp >= -128 else ("s", "<h") if hp >= -32768 else ("i", "<i")
    return b"HP" + typ.encode() + struct.pack(fmt, hp)


def bam_record(rd, final, references=None):
    """BAM record (with its block_size word) of one get_read_data tuple with its final CIGAR: what sam_line says, in
    binary -- the statement npore_bam_format_bam and the device path are tested against.  references: the header's
    contig names (refID = the contig's place among them; 0 without)."""
    import re
    read_id, flag, ref_name, start, mapq, _cig, stop, sseq, quals, _ref, hap = rd
    ref_id = list(references).index(ref_name) if references is not None else 0
    reflen = stop - start
    name = read_id.encode() + b"\0"
    cig = [(int(n), "MIDNSHP=X".index(op)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", final)]
    words = b"".join(struct.pack("<I", (n << 4) | op) for n, op in cig)
    tags = hp_tag(hap)
    if len(cig) > MAX_CIGAR_OPS:         # as htslib writes it: the placeholder <l_seq>S<reflen>N, the words in CG:B,I behind HP
        tags += b"CGBI" + struct.pack("<I", len(cig)) + words
        words = struct.pack("<II", (len(sseq) << 4) | 4, (reflen << 4) | 3)
    code = {c: i for i, c in enumerate(_SEQ16)}
    nib = [code[c] for c in sseq] + ([0] if len(sseq) & 1 else [])
    packed = bytes((nib[k] << 4) | nib[k + 1] for k in range(0, len(nib), 2))
    qual = bytes([0xFF]) * len(sseq) if quals == "*" else bytes(ord(c) - 33 for c in quals)
    body = (struct.pack("<iiBBHHHiiii", ref_id, start, len(name), mapq, reg2bin(start, start + max(1, reflen)), len(words) // 4,
                        flag, len(sseq), -1, -1, reflen) + name + words + packed + qual + tags)
    return struct.pack("<i", len(body)) + body


# ---- --records full: the pure-Python statement of csrc/bam_reader.hpp's FULL RECORD and csrc/nm_rec.hpp -------------
STALE_TAGS = (b"NM", b"MD", b"cs", b"de", b"dv", b"CG")      # what a realignment invalidates


def _aux_value_len(aux, q, typ):
    """Bytes of the value of a tag of type `typ` whose value begins at aux[q]; None: it cannot be stepped over."""
    if typ in b"cCA":
        n = 1
    elif typ in b"sS":
        n = 2
    elif typ in b"iIf":
        n = 4
    elif typ in b"ZH":
        z = aux.find(b"\0", q)
        if z < 0:
            return None
        n = z - q + 1
    elif typ == b"B":
        if q + 5 > len(aux):
            return None
        width = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}.get(aux[q:q + 1])
        if width is None:
            return None
        n = 5 + struct.unpack_from("<I", aux, q + 1)[0] * width
    else:
        return None
    return n if q + n <= len(aux) else None


def filter_aux(aux, oc=False):
    """The tags a FULL record keeps of the input's aux bytes: all of them in input order but STALE_TAGS -- and, under the
    option oc (NPORE_TAG_OC: the run writes its own), OC; a tag that cannot be stepped over ends the list -- it and
    everything behind it are dropped."""
    stale = STALE_TAGS + ((b"OC",) if oc else ())
    aux = bytes(aux)
    out, q = [], 0
    while q + 3 <= len(aux):
        n = _aux_value_len(aux, q + 3, aux[q + 2:q + 3])
        if n is None:
            break
        if aux[q:q + 2] not in stale:
            out.append(aux[q:q + 3 + n])
        q += 3 + n
    return b"".join(out)


def nm_of(ref_codes, seq_codes, final):
    """NM of a final CIGAR text over the code arrays align() got ('NACGT-' -> 0 ... 5, anything else 0): the bases under I
    and D, and the positions under M where the codes differ or either is 0 (a position beyond an array has code 0)."""
    import re
    nm = a = b = 0
    for n, op in re.findall(r"(\d+)([MIDNSHP=X])", final):
        n = int(n)
        if op in "M=X":
            for q in range(n):
                rc = int(ref_codes[a + q]) if a + q < len(ref_codes) else 0
                sc = int(seq_codes[b + q]) if b + q < len(seq_codes) else 0
                nm += rc != sc or rc == 0 or sc == 0
            a, b = a + n, b + n
        elif op == "I":
            nm, b = nm + n, b + n
        elif op == "D":
            nm, a = nm + n, a + n
        elif op == "N":
            a += n
        elif op == "S":
            b += n
    return nm


def md_of(ref_codes, seq_codes, final):
    """MD of a final CIGAR text over the code arrays align() got (csrc/md_rec.hpp, beside nm_of): the matches counted up to
    the next position under M where the codes differ or either is 0 -- the count, then the reference's letter --, or up to
    the next D -- the count, '^', the reference's letters --, and the closing count.  LETTER = "NACGTN"; a position beyond
    an array has code 0.  `samtools calmd`'s text but for nm_of's difference: an IUPAC letter other than N has code 0, so it
    counts as a mismatch and prints as N."""
    import re
    letter = "NACGTN"
    out, u, a, b = [], 0, 0, 0
    for n, op in re.findall(r"(\d+)([MIDNSHP=X])", final):
        n = int(n)
        if op in "M=X":
            for q in range(n):
                rc = int(ref_codes[a + q]) if a + q < len(ref_codes) else 0
                sc = int(seq_codes[b + q]) if b + q < len(seq_codes) else 0
                if rc != sc or rc == 0 or sc == 0:
                    out.append(f"{u}{letter[rc]}")
                    u = 0
                else:
                    u += 1
            a, b = a + n, b + n
        elif op == "D" and n > 0:
            out.append(f"{u}^" + "".join(letter[int(ref_codes[a + q]) if a + q < len(ref_codes) else 0] for q in range(n)))
            u, a = 0, a + n
        elif op == "N":
            a += n
        elif op in "IS":
            b += n
    return "".join(out) + str(u)


def _cs_items(ref_codes, seq_codes, final):
    """The final CIGAR as the items cs and de are made of, over the code arrays align() got: ("=", reference codes) for every
    maximal stretch of compared positions that do not differ -- a position differs where the codes are unequal or either is 0,
    as for NM and MD; a stretch runs on through neighbouring M / = / X words and ends at an I, D or N word and at a differing
    position --, ("*", reference code, read code) for a differing position, ("+", read codes) and ("-", reference codes) for
    an I and a D word.  N only advances the reference, S the read; a word of length 0 does nothing; a position beyond an
    array has code 0."""
    import re
    code = lambda arr, at: int(arr[at]) if at < len(arr) else 0
    items, run, a, b = [], [], 0, 0

    def close():
        if run:
            items.append(("=", list(run)))
            run.clear()
    for n, op in re.findall(r"(\d+)([MIDNSHP=X])", final):
        n = int(n)
        if n == 0:
            continue
        if op in "M=X":
            for q in range(n):
                rc, sc = code(ref_codes, a + q), code(seq_codes, b + q)
                if rc != sc or rc == 0 or sc == 0:
                    close()
                    items.append(("*", rc, sc))
                else:
                    run.append(rc)
            a, b = a + n, b + n
        elif op == "I":
            close()
            items.append(("+", [code(seq_codes, b + q) for q in range(n)]))
            b += n
        elif op == "D":
            close()
            items.append(("-", [code(ref_codes, a + q) for q in range(n)]))
            a += n
        elif op == "N":
            close()
            a += n
        elif op == "S":
            b += n
    close()
    return items


def cs_of(ref_codes, seq_codes, final, long=False):
    """minimap2's cs of a final CIGAR text over the code arrays align() got (beside nm_of and md_of): `:<n>` for a stretch of n
    compared positions that do not differ -- long: `=` and the reference's letters in upper case --, `*<ref><read>` for a
    position that differs, `+<read letters>` for an insertion, `-<reference letters>` for a deletion; letters lowercase,
    "nacgtn" by code.  `~` is never written (a final CIGAR has no N).  minimap2's text but for nm_of's difference: an IUPAC
    letter other than N has code 0, counts as a mismatch and prints as n."""
    low, up = "nacgtn", "NACGTN"
    out = []
    for it in _cs_items(ref_codes, seq_codes, final):
        if it[0] == "=":
            out.append("=" + "".join(up[c] for c in it[1]) if long else f":{len(it[1])}")
        elif it[0] == "*":
            out.append("*" + low[it[1]] + low[it[2]])
        else:
            out.append(it[0] + "".join(low[c] for c in it[1]))
    return "".join(out)


def de_of(ref_codes, seq_codes, final):
    """minimap2's de, the gap-compressed per-base divergence, of the same walk as a float32: (X + G) / (E + X + G) with E and X
    the compared positions that do not and that do differ and G the I and D words (each one gap open); 0 over nothing."""
    items = _cs_items(ref_codes, seq_codes, final)
    e = sum(len(it[1]) for it in items if it[0] == "=")
    x = sum(1 for it in items if it[0] == "*")
    g = sum(1 for it in items if it[0] in "+-")
    return np.float32((x + g) / (e + x + g)) if e + x + g else np.float32(0.0)


def eqx_of(ref_codes, seq_codes, final):
    """The =/X form of a final CIGAR text over the code arrays align() got (csrc/eqx_rec.hpp, beside nm_of, md_of and cs_of):
    every position under M, = or X -- whichever it was -- is X where nm_of counts it (the codes differ or either is 0; a
    position beyond an array has code 0) and = otherwise; the positions are run-length coded, a run going on through
    neighbouring M / = / X words; a word of any other op and length > 0 ends the run and follows it as it is; a word of
    length 0 is left out."""
    import re
    code = lambda arr, at: int(arr[at]) if at < len(arr) else 0
    out, cls, run, a, b = [], "", 0, 0, 0
    for n, op in re.findall(r"(\d+)([MIDNSHP=X])", final):
        n = int(n)
        if n == 0:
            continue
        if op in "M=X":
            for q in range(n):
                rc, sc = code(ref_codes, a + q), code(seq_codes, b + q)
                c = "X" if rc != sc or rc == 0 or sc == 0 else "="
                if run and c != cls:
                    out.append(f"{run}{cls}")
                    run = 0
                cls, run = c, run + 1
            a, b = a + n, b + n
            continue
        if run:
            out.append(f"{run}{cls}")
            run = 0
        out.append(f"{n}{op}")
        if op in "DN":
            a += n
        elif op in "IS":
            b += n
    if run:
        out.append(f"{run}{cls}")
    return "".join(out)


def oc_of(words):
    """The text of the OC tag (csrc/oc_rec.hpp) of an input CIGAR's words [(op, length)]: every word as it stands, its length
    in decimal and its letter -- clips and words of length 0 included, nothing merged, nothing mapped."""
    return "".join(f"{n}{'MIDNSHP=X???????'[op]}" for op, n in words)


def cigar_changed(words, final_text):
    """Whether a realignment CHANGED a read (csrc/oc_rec.hpp): words [(op, length)] is its input CIGAR between the clip words,
    final_text its final CIGAR in M form.  The canonical form of the input -- words of length 0 dropped, = and X read as M,
    neighbouring words of equal op merged -- is compared with the final's words as they stand: unchanged iff they are the
    same words, in number too."""
    import re
    canon = []
    for op, n in words:
        if n == 0:
            continue
        op = 0 if op in (7, 8) else op
        if canon and canon[-1][0] == op:
            canon[-1][1] += n
        else:
            canon.append([op, n])
    fin = [["MIDNSHP=X".index(op), int(n)] for n, op in re.findall(r"(\d+)([MIDNSHP=X])", final_text)]
    return canon != fin


def output_tags(cs, de, eqx=False, oc=False):
    """The word npore_bam_set_output_tags takes: NPORE_TAG_* of the options cs (None, "short", "long"), de and oc, and
    NPORE_CIGAR_EQX of eqx (OutputSpec.tags)"""
    return OutputSpec("bam", records="full", cs=cs, de=de, eqx=eqx, oc=oc).tags


def full_record(raw, ref_codes, seq_codes, final, md=False, cs=None, de=False, eqx=False, oc=False):
    """The FULL record (--records full, with its block_size word) of the input record `raw` (block_size word first) with
    its final CIGAR: the statement npore_bam_format_bam_full and the device path are tested against.  md: with the MD tag
    (md_of) behind NM, as NPORE_OUT_MD writes it; cs ("short" / "long") and de: with cs_of / de_of behind that, as
    NPORE_TAG_CS / NPORE_TAG_DE write them; eqx: the final CIGAR in its =/X form (eqx_of) between the clip words, as
    NPORE_CIGAR_EQX writes it -- the tags are those of `final` either way; oc: with the input's CIGAR as OC:Z (oc_of) behind
    those where `final` is not the input's canonical form (cigar_changed), and without the input's own OC either way, as
    NPORE_TAG_OC writes it."""
    import re
    raw = bytes(raw)
    ref_id, pos, l_rn, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", raw, 4)
    q = 36
    name = raw[q:q + l_rn]
    q += l_rn
    cigar = [(c & 15, c >> 4) for c in struct.unpack_from(f"<{n_cig}I", raw, q)]
    q += 4 * n_cig
    body = raw[q:q + (l_seq + 1) // 2 + l_seq]            # bases and qualities as they lie
    aux = raw[q + len(body):4 + struct.unpack_from("<i", raw, 0)[0]]
    cigar = resolve_long_cigar(cigar, l_seq, ref_id, pos, aux)
    reflen = sum(n for op, n in cigar if op in (0, 2, 3, 7, 8))
    lead = []
    if cigar and cigar[0][0] == 5:
        lead.append(cigar[0])
    if len(cigar) > len(lead) and cigar[len(lead)][0] == 4:
        lead.append(cigar[len(lead)])
    rest, trail = cigar[len(lead):], []
    if rest and rest[-1][0] == 5:
        trail.insert(0, rest.pop())
    if rest and rest[-1][0] == 4:
        trail.insert(0, rest.pop())
    fin = [("MIDNSHP=X".index(op), int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", eqx_of(ref_codes, seq_codes, final) if eqx else final)]
    words = b"".join(struct.pack("<I", (n << 4) | op) for op, n in lead + fin + trail)
    nm = nm_of(ref_codes, seq_codes, final)
    tags = filter_aux(aux, oc) + b"NM" + (b"C" + struct.pack("<B", nm) if nm <= 0xFF else b"S" + struct.pack("<H", nm) if nm <= 0xFFFF
                                      else b"I" + struct.pack("<I", nm))
    if md:
        tags += b"MDZ" + md_of(ref_codes, seq_codes, final).encode() + b"\0"
    if cs:
        tags += b"csZ" + cs_of(ref_codes, seq_codes, final, long=cs == "long").encode() + b"\0"
    if de:
        tags += b"def" + struct.pack("<f", de_of(ref_codes, seq_codes, final))
    if oc and cigar_changed(rest, final):
        tags += b"OCZ" + oc_of(cigar).encode() + b"\0"
    if len(words) // 4 > MAX_CIGAR_OPS:
        tags += b"CGBI" + struct.pack("<I", len(words) // 4) + words
        words = struct.pack("<II", (l_seq << 4) | 4, (reflen << 4) | 3)
    out = (struct.pack("<iiBBHHHiiii", ref_id, pos, l_rn, mapq, reg2bin(pos, pos + max(1, reflen)), len(words) // 4, flag, l_seq,
                       nref, npos, tlen) + name + words + body + tags)
    return struct.pack("<i", len(out)) + out


def bgzf_stored(data):
    """`data` as BGZF members with stored deflate blocks, cut every BGZF_STORED_PAYLOAD bytes."""
    out = []
    for p in range(0, len(data), BGZF_STORED_PAYLOAD):
        chunk = bytes(data[p:p + BGZF_STORED_PAYLOAD])
        n = len(chunk)
        out.append(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, n + 30) +
                   struct.pack("<BHH", 1, n, n ^ 0xFFFF) + chunk + struct.pack("<II", zlib.crc32(chunk), n))
    return b"".join(out)


# ---- --bam_compress huffman: the Python statement of csrc/deflate_code.hpp (read the rule there) ---------------------
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_CL_EXTRA = {16: 2, 17: 3, 18: 7}


def huffman_lengths(freq, limit):
    """Code lengths (at most `limit` bits) of the symbols with freq > 0: Huffman's algorithm on the symbols in ascending
    (freq, symbol) order with two queues -- a leaf before an internal node of equal weight --, the Kraft-sum repair for
    trees deeper than `limit`, the longest lengths to the rarest symbols."""
    order = sorted((f, s) for s, f in enumerate(freq) if f)
    lens = [0] * len(freq)
    m = len(order)
    if m == 0:
        return lens
    if m == 1:
        lens[order[0][1]] = 1
        return lens
    weight = [f for f, _ in order]              # leaves 0 .. m-1, then the internal nodes in order of creation
    parent = [0] * (2 * m - 1)
    leaf, node = 0, m
    for new in range(m, 2 * m - 1):
        w = 0
        for _ in range(2):
            if leaf < m and (node >= new or weight[leaf] <= weight[node]):
                pick, leaf = leaf, leaf + 1
            else:
                pick, node = node, node + 1
            parent[pick] = new
            w += weight[pick]
        weight.append(w)
    depth = [0] * (2 * m - 1)
    for k in range(2 * m - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    count = [0] * (limit + 1)
    for k in range(m):
        count[min(depth[k], limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total != 1 << limit:
        count[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    k = 0
    for l in range(limit, 0, -1):
        for _ in range(count[l]):
            lens[order[k][1]] = l
            k += 1
    return lens


def canonical_codes(lens):
    """(length, code bit-reversed for an LSB-first stream) per symbol: RFC 1951 3.2.2."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 16):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    out = []
    for l in lens:
        if not l:
            out.append((0, 0))
            continue
        v, nxt[l] = nxt[l], nxt[l] + 1
        out.append((l, int(format(v, "0%db" % l)[::-1], 2)))
    return out


def _code_length_header(ll_lens, d_lens):
    """The block header (BFINAL ... the code-length sequence) as (bits as an integer, LSB first; how many): ll_lens the HLIT
    literal / length lengths, d_lens the HDIST distance lengths, run-coded as ONE sequence."""
    seq, cl_freq = [], [0] * 19
    allv = list(ll_lens) + list(d_lens)
    i = 0
    while i < len(allv):
        v, r = allv[i], 1
        while i + r < len(allv) and allv[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                t = min(r, 138)
                seq.append((18, t - 11))
                r -= t
            if r >= 3:
                seq.append((17, r - 3))
                r = 0
        else:
            seq.append((v, 0))
            r -= 1
            while r >= 3:
                t = min(r, 6)
                seq.append((16, t - 3))
                r -= t
        seq += [(v, 0)] * r
    for s, _ in seq:
        cl_freq[s] += 1
    cl_lens = huffman_lengths(cl_freq, 7)
    cl_codes = canonical_codes(cl_lens)
    hclen = max([4] + [k + 1 for k in range(19) if cl_lens[_CL_ORDER[k]]])
    acc, nbits = 0, 0

    def put(v, n):
        nonlocal acc, nbits
        acc |= v << nbits
        nbits += n
    put(1, 1), put(2, 2), put(len(ll_lens) - 257, 5), put(len(d_lens) - 1, 5), put(hclen - 4, 4)
    for k in range(hclen):
        put(cl_lens[_CL_ORDER[k]], 3)
    for s, extra in seq:
        put(cl_codes[s][1], cl_codes[s][0])
        if s >= 16:
            put(extra, _CL_EXTRA[s])
    return acc, nbits


def _pack_fields(acc, header_bits, values, widths, n_bytes):
    """The block's bytes: the header's bits, then field k's widths[k] low bits of values[k], LSB first, one after the other."""
    values, widths = np.asarray(values, np.int64), np.asarray(widths, np.int64)
    at = header_bits + np.concatenate([[0], np.cumsum(widths)[:-1]])
    bits = np.zeros(n_bytes * 8, np.uint8)
    bits[:header_bits] = np.array([(acc >> k) & 1 for k in range(header_bits)], np.uint8)
    for b in range(int(widths.max()) if len(widths) else 0):
        use = widths > b
        bits[at[use] + b] = (values[use] >> b) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def deflate_block(payload):
    """(block bytes or None when it would not be smaller than the stored block, header bits, data bits) of the payload as
    one final dynamic-Huffman block of literals."""
    freq = np.bincount(np.frombuffer(payload, np.uint8), minlength=257).tolist()
    freq[256] = 1
    lens = huffman_lengths(freq, 15)
    codes = canonical_codes(lens)
    acc, header_bits = _code_length_header(lens, [0])       # ... and the one distance code, of length 0
    data_bits = sum(f * l for f, l in zip(freq, lens))
    n_bytes = (header_bits + data_bits + 7) // 8
    if n_bytes >= len(payload) + 5:
        return None, header_bits, data_bits
    sym = np.concatenate([np.frombuffer(payload, np.uint8).astype(np.int64), [256]])
    ln = np.array([c[0] for c in codes], np.int64)[sym]
    cd = np.array([c[1] for c in codes], np.int64)[sym]
    return _pack_fields(acc, header_bits, cd, ln, n_bytes), header_bits, data_bits


# ---- --bam_compress match: the rule's steps 1 to 6 (csrc/deflate_code.hpp, MATCHES), with the tables of RFC 1951 3.2.5 ---------
_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0) + tuple(e for e in range(1, 14) for _ in range(2))
MATCH_HASH_BITS, MATCH_MIN, MATCH_MAX, MATCH_MAX_DIST = 15, 4, 258, 32768


def _len_symbol(length):
    k = max(j for j in range(29) if _LEN_BASE[j] <= length)
    return 257 + k, _LEN_EXTRA[k], length - _LEN_BASE[k]


def _dist_symbol(dist):
    k = max(j for j in range(30) if _DIST_BASE[j] <= dist)
    return k, _DIST_EXTRA[k], dist - _DIST_BASE[k]


def match_hashes(payload):
    """H(i) for i <= n - 4: the four bytes at i little-endian, times 2654435761 modulo 2^32, the top 15 bits."""
    p = np.frombuffer(payload, np.uint8).astype(np.uint64)
    if len(p) < 4:
        return np.zeros(0, np.int64)
    word = p[:-3] | p[1:-2] << np.uint64(8) | p[2:-1] << np.uint64(16) | p[3:] << np.uint64(24)
    return (((word * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - MATCH_HASH_BITS)).astype(np.int64)


def match_tokens(payload):
    """The greedy parse: a list of literals (an int) and matches ((length, distance)).  The candidate of a position is the
    nearest earlier position of equal HASH; a match has >= 4 equal bytes, at most 258 and not past the end, at most 32 768 back."""
    payload = bytes(payload)
    n = len(payload)
    hashes = match_hashes(payload).tolist()
    cand, last = [], {}
    for i, h in enumerate(hashes):
        cand.append(last.get(h, -1))
        last[h] = i
    tokens, i = [], 0
    while i < n:
        c = cand[i] if i < len(cand) else -1
        length = 0
        if c >= 0 and i - c <= MATCH_MAX_DIST:
            cap = min(MATCH_MAX, n - i)
            a, b = payload[c:c + cap], payload[i:i + cap]
            length = cap if a == b else next(k for k in range(cap) if a[k] != b[k])
        if length >= MATCH_MIN:
            tokens.append((length, i - c))
            i += length
        else:
            tokens.append(payload[i])
            i += 1
    return tokens


def deflate_match_block(payload, tokens=None):
    """(block bytes, header bits, data bits) of the payload as one final dynamic-Huffman block of its tokens."""
    tokens = match_tokens(payload) if tokens is None else tokens
    ll_freq, d_freq = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            ll_freq[_len_symbol(t[0])[0]] += 1
            d_freq[_dist_symbol(t[1])[0]] += 1
        else:
            ll_freq[t] += 1
    ll_freq[256] = 1
    ll_lens, d_lens = huffman_lengths(ll_freq, 15), huffman_lengths(d_freq, 15)
    hlit = max([257] + [s + 1 for s in range(286) if ll_freq[s]])
    hdist = max([1] + [s + 1 for s in range(30) if d_freq[s]])
    ll_codes, d_codes = canonical_codes(ll_lens), canonical_codes(d_lens)
    acc, header_bits = _code_length_header(ll_lens[:hlit], d_lens[:hdist])
    values, widths = [], []
    for t in tokens + [256]:
        if isinstance(t, tuple):
            ls, le, lv = _len_symbol(t[0])
            ds, de, dv = _dist_symbol(t[1])
            values += [ll_codes[ls][1], lv, d_codes[ds][1], dv]
            widths += [ll_codes[ls][0], le, d_codes[ds][0], de]
        else:
            values.append(ll_codes[t][1])
            widths.append(ll_codes[t][0])
    data_bits = sum(widths)
    n_bytes = (header_bits + data_bits + 7) // 8
    return _pack_fields(acc, header_bits, values, widths, n_bytes), header_bits, data_bits


def deflate_member(payload, matches=False):
    """One BGZF member (at most BGZF_STORED_PAYLOAD bytes of payload) in --bam_compress huffman: one dynamic-Huffman block
    of literals, or the stored member where that is not smaller (and for an empty payload).  matches (--bam_compress match):
    the block of literals and length / distance pairs where it is smaller than both, otherwise that same member."""
    payload = bytes(payload)
    n = len(payload)
    block, hb, db = deflate_block(payload) if n else (None, 0, 0)
    if matches and n:
        h = (hb + db + 7) // 8
        mblock = deflate_match_block(payload)[0]
        if len(mblock) < h and len(mblock) < n + 5:
            block = mblock
    if block is None:
        return _stored_member(payload)
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(block) + 25) + block +
            struct.pack("<II", zlib.crc32(payload), n))


def _stored_member(chunk):
    n = len(chunk)
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, n + 30) +
            struct.pack("<BHH", 1, n, n ^ 0xFFFF) + chunk + struct.pack("<II", zlib.crc32(chunk), n))


def bgzf_members(data, compress="none"):
    """`data` cut every BGZF_STORED_PAYLOAD bytes, each piece a member of the mode."""
    if compress == "none":
        return bgzf_stored(data)
    if compress not in ("huffman", "match"):
        raise ValueError("compress must be 'none', 'huffman' or 'match'")
    return b"".join(deflate_member(data[p:p + BGZF_STORED_PAYLOAD], compress == "match") for p in range(0, len(data), BGZF_STORED_PAYLOAD))


def bam_header_bytes(text, references, lengths):
    out = bytearray(b"BAM\1" + struct.pack("<i", len(text.encode())) + text.encode() + struct.pack("<i", len(references)))
    for n, l in zip(references, lengths):
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return bytes(out)


def create_bam_header(outfile, bam):
    """create_header for a BAM: the same text and the binary reference list, in BGZF members of their own; truncates."""
    if os.path.dirname(outfile):
        os.makedirs(os.path.dirname(outfile), exist_ok=True)
    with open(outfile, "wb") as fh:
        fh.write(bgzf_stored(bam_header_bytes(header_text(bam), bam.references, bam.lengths)))


NOT_SORTED_MSG = "    (the records did not go out in coordinate order: no .bai index is written)"


class BamRecordWriter:
    """Pure-Python twin of the library's BgzfStoredWriter: record bytes appended to `path` behind what lies there (the
    header's members), the stream cut every BGZF_STORED_PAYLOAD bytes whatever the batches were; close() writes the last
    member, the EOF member and -- when the records came in coordinate order -- `bai` (write_bai with its bins).  Whole
    files only: --python_io runs in one process."""

    def __init__(self, path, bai=None, compress="none"):
        self.path, self.bai, self.compress = path, bai, compress
        self.fh = open(path, "ab")
        self.carry = b""
        self.sorted, self.last = True, (-1, -1)
        self.n_records = 0

    def add(self, records):
        for rec in records:
            key = struct.unpack_from("<ii", rec, 4)
            if key < self.last:
                self.sorted = False
            self.last = key
            self.n_records += 1
        data = self.carry + b"".join(records)
        whole = len(data) - len(data) % BGZF_STORED_PAYLOAD
        self.fh.write(bgzf_members(data[:whole], self.compress))
        self.carry = data[whole:]

    def close(self):
        """Returns True when the index was written (or none was asked for)."""
        self.fh.write(bgzf_members(self.carry, self.compress))
        self.fh.write(BGZF_EOF)
        self.fh.close()
        if self.bai and self.sorted:
            write_bai(self.path, self.bai, bins=True)
        elif self.bai:
            if os.path.exists(self.bai):
                os.remove(self.bai)
            print(NOT_SORTED_MSG)
        return self.sorted or not self.bai


def realign_reads(ctx, read_data, out_sam, r=30, max_b_rows=20000, bam_writer=None, references=None):
    """Batched realign_read (src/bam.pyx:51-84): align on the GPU, standardise, append SAM lines -- or, with a
    BamRecordWriter, hand it the reads' BAM records (out_sam is not touched then).
    Returns the number of reads written."""
    read_data = list(read_data)
    if not read_data:
        return 0
    cigs, refs, seqs = [], [], []
    for rd in read_data:
        cigs.append(expand_cigar(rd[5]).replace("S", "").replace("H", ""))     # src/bam.pyx:59
        refs.append(bases_to_int(rd[9]))
        seqs.append(bases_to_int(rd[7]))
    alns, status = ctx.align_batch(refs, seqs, cigs, r=r, max_b_rows=max_b_rows, return_status=True)
    finals = standardize_batch(alns, refs, seqs)          # src/bam.pyx:65-78, C++ glue in the library
    lines = []
    for rd, final, st in zip(read_data, finals, status):
        read_id = rd[0]
        if st & 32:
            print(f"\nERROR: read '{read_id}': CIGAR does not match sequence lengths; skipped.")
            continue
        if st:
            print(f"\nERROR: inconsistent traceback for read '{read_id}' (status {int(st)})")   # src/aln.pyx:689-716
        lines.append(sam_line(rd, final) if bam_writer is None else bam_record(rd, final, references))
    if bam_writer is not None:
        bam_writer.add(lines)
    else:
        with open(out_sam, "a") as fh:
            fh.write("".join(lines))
    return len(read_data)


def realign_haps(ctx, hap_data, r=30, max_b_rows=20000):
    """Batched realign_hap (src/bam.pyx:93-123), the second caller of align() in the reference
    (standardize_vcf.py:32-34: whole haplotype sequences against the reference, thousands of
    independent chunks per sequence): [(contig, hap, seq, ref, cigar)] -> the same tuples with the
    realigned, standardised, expanded 'MID' CIGAR."""
    hap_data = list(hap_data)
    if not hap_data:
        return []
    refs = [bases_to_int(h[3]) for h in hap_data]
    seqs = [bases_to_int(h[2]) for h in hap_data]
    alns, status = ctx.align_batch(refs, seqs, [h[4] for h in hap_data], r=r, max_b_rows=max_b_rows, return_status=True)
    for h, st in zip(hap_data, status):
        if st:
            print(f"\nERROR: inconsistent traceback for {h[0]} hap {h[1]} (status {int(st)})")
    finals = standardize_batch(alns, refs, seqs, expanded=True)
    return [(h[0], h[1], h[2], h[3], f) for h, f in zip(hap_data, finals)]


def sam_line(rd, final):
    """SAM record of one get_read_data tuple with its final CIGAR (src/bam.pyx:83)."""
    read_id, flag, ref_name, start, mapq, _cig, stop, sseq, quals, _ref, hap = rd
    return (f"{read_id}\t{flag}\t{ref_name}\t{start + 1}\t{mapq}\t{final}\t*\t0\t"
            f"{stop - start}\t{sseq}\t{quals}\tHP:i:{hap}\n")


# ---------------------------------------------------------------------------
# native host I/O (libnpore_amd.so, csrc/hostio.hpp + csrc/bam_reader.hpp)
class NativeFasta:
    """Contig names / lengths of a FASTA held by the library; behaves like {name: sized} for get_bam_regions."""

    class _Sized:
        def __init__(self, n):
            self._n = n

        def __len__(self):
            return self._n

    def __init__(self, path):
        from . import _lib
        self._lib = _lib.load()
        self.handle = self._lib.npore_fasta_open(os.fsencode(path))
        if not self.handle:
            print(f"\nERROR: could not open --ref FASTA '{path}'.")
            sys.exit(1)
        self.names = [self._lib.npore_fasta_name(self.handle, i).decode() for i in range(self._lib.npore_fasta_n(self.handle))]
        self._len = {n: int(self._lib.npore_fasta_len(self.handle, i)) for i, n in enumerate(self.names)}

    def __contains__(self, name):
        return name in self._len

    def __getitem__(self, name):
        return NativeFasta._Sized(self._len[name])

    def __iter__(self):
        return iter(self.names)

    def sequence(self, name):
        """The upper-cased bases of a contig as a str (a copy)."""
        import ctypes as C
        i = len(self.names) - 1 - self.names[::-1].index(name)       # a repeated name: the last one, like a dict
        return C.string_at(self._lib.npore_fasta_seq(self.handle, i), self._len[name]).decode()

    def close(self):
        if self.handle:
            self._lib.npore_fasta_close(self.handle)
            self.handle = None


class NativeFastaSeqs:
    """{contig: upper-cased sequence}, like read_fasta(), backed by the library's parallel parser; a contig's
    str is made on first use (callers that only need a few contigs of a genome)."""

    def __init__(self, path):
        self._fa = NativeFasta(path)
        self._cache = {}

    def __contains__(self, name):
        return name in self._fa

    def __iter__(self):
        return iter(dict.fromkeys(self._fa.names))

    def __len__(self):
        return len(dict.fromkeys(self._fa.names))

    def __getitem__(self, name):
        if name not in self._cache:
            if name not in self._fa:
                raise KeyError(name)
            self._cache[name] = self._fa.sequence(name)
        return self._cache[name]

    def items(self):
        return ((n, self[n]) for n in self)

    def keys(self):
        return list(self)


# --pass_through (npore_bam_set_output_pass): the flag bits whose records a FULL-record run can write as they came -- secondary,
# supplementary, placed but unmapped -- and the status bit such a record gets
PASS_FLAGS = 0x100 | 0x800 | 0x4
ST_PASSED = 128
# the words an output setting is said in (include/npore_amd.h, NPORE_* of the same names): the flags of npore_bam_set_output and
# of the npore_bam_format_bam_full entries (which know OUT_MD alone), and the word of npore_bam_set_output_tags
OUT_EOF, OUT_PART, OUT_DEFLATE, OUT_MATCH, OUT_FULL, OUT_MD = 1, 2, 4, 8, 16, 32
TAG_CS, TAG_CS_LONG, TAG_DE, CIGAR_EQX, TAG_OC = 1, 2, 4, 32, 256

_COMPRESS = {"none": 0, "huffman": OUT_DEFLATE, "match": OUT_DEFLATE | OUT_MATCH}
_CS = {None: 0, "short": TAG_CS, "long": TAG_CS | TAG_CS_LONG}


def _needs_full(field):
    return lambda s: bool(getattr(s, field)) and s.records != "full"


# The rules of an output setting, in the order OutputSpec states them: what breaks the rule, the ValueError's text, and the line
# realign prints (None: argparse's choices say it there).  realign names the first broken rule of _CLI_ORDER.
_TAGS_NEED_FULL = "cs, de, eqx and oc need records 'full'"
_RULES = {
    "pass_mask": (_needs_full("pass_mask"), "pass_mask needs records 'full'", "--pass_through needs --out_format bam --records full."),
    "compress values": (lambda s: s.compress not in _COMPRESS, "compress must be 'none', 'huffman' or 'match'", None),
    "records values": (lambda s: s.records not in ("reference", "full"), "records must be 'reference' or 'full'", None),
    "records": (lambda s: s.records == "full" and s.out_format != "bam", "records 'full' needs out_format 'bam'",
                "--records full needs --out_format bam."),
    "md": (_needs_full("md"), "md needs records 'full'", "--md needs --records full."),
    "cs values": (lambda s: s.cs not in _CS, "cs must be None, 'short' or 'long'", None),
    "cs": (_needs_full("cs"), _TAGS_NEED_FULL, "--cs needs --out_format bam --records full."),
    "de": (_needs_full("de"), _TAGS_NEED_FULL, "--de needs --out_format bam --records full."),
    "eqx": (_needs_full("eqx"), _TAGS_NEED_FULL, "--eqx needs --out_format bam --records full."),
    "oc": (_needs_full("oc"), _TAGS_NEED_FULL, "--oc needs --out_format bam --records full."),
    "compress": (lambda s: s.compress != "none" and s.out_format != "bam", "compress needs out_format 'bam'",
                 "--bam_compress needs --out_format bam."),
}
_CLI_ORDER = ("records", "md", "cs", "de", "eqx", "oc", "pass_mask", "compress")


class OutputSpecError(ValueError):
    """An OutputSpec that breaks a rule; .cli is the line realign prints for it."""

    def __init__(self, text, cli):
        super().__init__(text)
        self.cli = cli


@dataclasses.dataclass(frozen=True)
class OutputSpec:
    """What a run (realign_file / realign_sequential / write_file) appends to its output path; NativeBam.set_output hands it to
    the library.  out_format: "sam", or "bam" -- records in BGZF members behind what lies in the file (the header's members:
    create_bam_header) and `bai` written when the records went out in coordinate order.  eof: the run ends the file (the EOF
    member, OUT_EOF); False: it writes one rank's PART (OUT_PART) -- no EOF member, and `bai` is a sidecar whose offsets count
    from PART_BASE (dist.gather_bam_parts shifts and merges them).  compress: "none", stored members, "huffman", every member
    one dynamic-Huffman block of literals (OUT_DEFLATE), or "match", of literals and length / distance pairs where that is
    smaller (OUT_MATCH beside it); "bam" only.  records: "reference", the reference's SAM line in binary, or "full", the input
    record with only what the realignment changes replaced (OUT_FULL; "bam" only).  The rest needs records "full".  md: the MD
    tag behind the recounted NM of every record (OUT_MD).  cs: "short" or "long", minimap2's cs tag behind that (TAG_CS,
    TAG_CS_LONG), de: its de tag behind that (TAG_DE).  pass_mask: a subset of PASS_FLAGS -- the records with one of those flag
    bits are written as they came (npore_bam_set_output_pass).  eqx: the final CIGAR of every record in =/X form (CIGAR_EQX, in
    the tags' word).  oc: the input's CIGAR as OC:Z on every read whose alignment changed; the input's own OC is dropped, so an
    unchanged read has none (TAG_OC, in the tags' word).
    A spec that breaks one of _RULES is not made: OutputSpecError, a ValueError."""
    out_format: str = "sam"
    bai: object = None
    eof: bool = True
    compress: str = "none"
    records: str = "reference"
    md: bool = False
    cs: object = None
    de: bool = False
    pass_mask: int = 0
    eqx: bool = False
    oc: bool = False

    def __post_init__(self):
        broken = [k for k, (is_broken, _, _) in _RULES.items() if is_broken(self)]
        if broken:
            text = _RULES[broken[0]][1]
            raise OutputSpecError(text, next((_RULES[k][2] for k in _CLI_ORDER if k in broken), text))

    @classmethod
    def from_args(cls, args, **overrides):
        """The spec realign's command line asks for (argparser's names; an option the namespace lacks is off); bai and eof, which
        the command line does not say, come as overrides."""
        said = dict(out_format=getattr(args, "out_format", "sam"), compress=getattr(args, "bam_compress", "none"),
                    records=getattr(args, "records", "reference"), md=bool(getattr(args, "md", False)), cs=getattr(args, "cs", None),
                    de=bool(getattr(args, "de", False)), pass_mask=PASS_FLAGS if getattr(args, "pass_through", False) else 0,
                    eqx=bool(getattr(args, "eqx", False)), oc=bool(getattr(args, "oc", False)))
        return cls(**{**said, **overrides})

    @property
    def format_word(self):
        """NPORE_OUT_SAM / NPORE_OUT_BAM"""
        return {"sam": 0, "bam": 1}[self.out_format]

    @property
    def flags(self):
        """the flags of npore_bam_set_output"""
        return ((0 if self.out_format != "bam" else OUT_EOF if self.eof else OUT_PART) | _COMPRESS[self.compress]
                | (OUT_FULL if self.records == "full" else 0) | (OUT_MD if self.md else 0))

    @property
    def tags(self):
        """the word of npore_bam_set_output_tags"""
        return _CS[self.cs] | (TAG_DE if self.de else 0) | (CIGAR_EQX if self.eqx else 0) | (TAG_OC if self.oc else 0)


def marshal_finals(idx, finals, status):
    """The reads `idx` with their final CIGAR strings and status words as the format_* / write_file entries take them: (the
    contiguous arrays, to be held while the pointers are in use; the arguments idx, n, text, offsets, lengths, status).  The
    joined text ends in a NUL."""
    idx = np.ascontiguousarray(idx, np.int64)
    fb = [f.encode() for f in finals]
    fo = np.zeros(len(idx) + 1, np.int64)
    np.cumsum([len(f) for f in fb], out=fo[1:])
    fl = np.ascontiguousarray(np.diff(fo))
    buf = np.frombuffer(b"".join(fb) + b"\0", np.uint8)
    st = np.ascontiguousarray(status, np.int32)
    return (idx, buf, fo, fl, st), (idx.ctypes.data, len(idx), buf.ctypes.data, fo.ctypes.data, fl.ctypes.data, st.ctypes.data)


class OnePassUnsupported(RuntimeError):
    """NativeBam.realign_sequential cannot serve these regions / this file in one pass (take the indexed path)."""


class StaleIndex(RuntimeError):
    """The .bai beside the BAM declares a contig empty on which the one-pass walk met a record: the default regions made
    from it would leave reads out.  The message names the index; the run ends (no other reader is taken: the regions are
    the index's too)."""


class NativeBam:
    """A BAM file inflated and indexed by the library (same attributes as BamFile where realign needs them)."""

    def __init__(self, path, threads=0, share=None, stream=None, one_pass=False):
        """stream: None = the library decides (files above NPORE_BAM_STREAM_MB, default 1 GB, are STREAMED: no
        inflated copy, 22 bytes of index per record, each batch inflates the blocks its reads lie in), True / False force it.
        share: with several processes per node (one per GPU, torch.distributed.run) local rank 0 does the expensive
        part once and leaves it under /dev/shm for the other local ranks -- the record index of a streamed file
        (npore_bam_save_index), the inflated stream of a small one (npore_bam_dump_inflated); None = do so when
        LOCAL_WORLD_SIZE > 1."""
        from . import _lib
        self._lib = _lib.load()
        self._shared = None
        self.path = path
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if stream is None and os.environ.get("NPORE_BAM_STREAM") in ("0", "1"):
            stream = os.environ["NPORE_BAM_STREAM"] == "1"
        mode = 3 if one_pass else 0 if stream is None else (2 if stream else 1)
        self.one_pass = bool(one_pass)
        if one_pass:
            share = False
        if share is None:
            share = local_world > 1 and os.path.isdir("/dev/shm") and os.environ.get("NPORE_SHARE_BAM", "1") != "0"
        will_stream = mode == 2 or (mode == 0 and self._auto_streams(path))
        self.handle = None
        if share and local_world > 1 and will_stream:
            self.handle = self._open_with_shared_index(path, local_rank, threads)
        elif share and local_world > 1:
            path_to_open = self._shared_copy(path, local_rank, threads)
            self.handle = self._lib.npore_bam_open_mode(os.fsencode(path_to_open), threads, 1, None)
        if not self.handle:
            self.handle = self._lib.npore_bam_open_mode(os.fsencode(path), threads, mode, None)
        if not self.handle:
            msg = _lib.last_error()
            print(f"\nERROR: BAM file '{path}' not found." if "not found" in msg else f"\nERROR: {msg}.")
            sys.exit(1)
        self.streamed = bool(self._lib.npore_bam_is_streamed(self.handle))
        n = self._lib.npore_bam_n_refs(self.handle)
        self.references = [self._lib.npore_bam_ref_name(self.handle, i).decode() for i in range(n)]
        self.lengths = [int(self._lib.npore_bam_ref_len(self.handle, i)) for i in range(n)]
        self.n_records = int(self._lib.npore_bam_n_records(self.handle))

    @staticmethod
    def is_bgzf(path):
        try:
            with open(path, "rb") as fh:
                return fh.read(2) == b"\x1f\x8b"
        except OSError:
            return False

    @staticmethod
    def _auto_streams(path):
        try:
            with open(path, "rb") as fh:
                gz = fh.read(2) == b"\x1f\x8b"
            return gz and os.path.getsize(path) > int(os.environ.get("NPORE_BAM_STREAM_MB", "1024")) * (1 << 20)
        except OSError:
            return False

    _opens = {}          # (path, local rank) -> how many times this process has opened it for sharing (the same in every local rank)

    @classmethod
    def _shm_key(cls, path):
        """Name of the files local rank 0 leaves for the other local ranks.  Besides the file's identity it holds only
        what the LAUNCHER hands to every local rank alike -- the rendezvous (MASTER_ADDR : MASTER_PORT), torchrun's run
        id, a batch system's job id -- and the count of this process's opens of the path (SPMD code opens the same
        files in the same order on every rank; a second NativeBam of the same file in one run then does not find the
        first one's `.skip`).  Nothing per-process goes in (rounds 3 - 4 hashed the parent's pid: local ranks started
        by per-rank wrapper scripts have different parents and never met).  Two launches that share all of this share
        the key; local rank 0 removes what an earlier one left (`_announce_maker`), and a rank whose key does diverge
        for a reason not foreseen here gives up after a grace period (`_wait_for_maker`)."""
        import hashlib
        st = os.stat(path)
        ap = os.path.abspath(path)
        who = (ap, os.environ.get("LOCAL_RANK", "0"))
        gen = cls._opens[who] = cls._opens.get(who, 0) + 1
        job = ":".join(os.environ.get(k, "") for k in ("MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID", "SLURM_JOB_ID",
                                                         "SLURM_STEP_ID", "PBS_JOBID", "LSB_JOBID", "NPORE_JOB_ID"))
        ident = f"{ap}:{st.st_size}:{st.st_mtime_ns}:{job}:{gen}"
        return hashlib.sha1(ident.encode()).hexdigest()[:16]

    @staticmethod
    def _announce_maker(key):
        """local rank 0: its pid where the waiting ranks can see whether it is still alive; stale leftovers of the key removed"""
        for ext in (".idx", ".raw", ".skip"):
            try:
                os.remove(f"/dev/shm/npore_bam_{key}{ext}")
            except OSError:
                pass
        tmp = f"/dev/shm/npore_bam_{key}.pid.tmp"
        with open(tmp, "w") as fh:
            fh.write(str(os.getpid()))
        os.replace(tmp, f"/dev/shm/npore_bam_{key}.pid")

    @staticmethod
    def _wait_for_maker(key, data, skip, timeout):
        """other local ranks: True once `data` is there; False if the maker gave up (`skip`), died, never showed up
        (no pid file within NPORE_SHARE_GRACE_S, 30 s: the ranks' keys differ, or local rank 0 is not running this
        code -- the caller then opens the file itself), or `timeout` passed"""
        import time
        pidfile = f"/dev/shm/npore_bam_{key}.pid"
        grace = float(os.environ.get("NPORE_SHARE_GRACE_S", "30"))
        t0 = time.time()
        seen_maker = False
        while time.time() - t0 < timeout:
            if os.path.exists(data):
                return True
            if os.path.exists(skip):
                return False
            try:
                pid = int(open(pidfile).read())                # (no pid file yet: the maker has not started)
                seen_maker = True
            except (OSError, ValueError):
                pid = None
            if not seen_maker and time.time() - t0 > grace:
                return False
            if pid is not None:
                try:
                    os.kill(pid, 0)
                except ProcessLookupError:                     # the maker is gone: what it left is all there will be
                    return os.path.exists(data)
                except OSError:
                    pass
            time.sleep(0.05)
        return False

    def _open_with_shared_index(self, path, local_rank, threads):
        """Streamed file, several local ranks: local rank 0 makes the record index (one pass over the file) and saves
        it under /dev/shm; the others wait for it and open with it.  Returns a handle or None (caller opens normally)."""
        try:
            key = self._shm_key(path)
        except OSError:
            return None
        ix, skip = f"/dev/shm/npore_bam_{key}.idx", f"/dev/shm/npore_bam_{key}.skip"
        if local_rank == 0:
            self._announce_maker(key)
            h = self._lib.npore_bam_open_mode(os.fsencode(path), threads, 2, None)
            if not h or self._lib.npore_bam_save_index(h, os.fsencode(ix + ".tmp")) != 0:
                open(skip, "w").close()
                self._shared = (ix, skip, key)
                return h or None
            os.replace(ix + ".tmp", ix)
            self._shared = (ix, skip, key)
            return h
        if self._wait_for_maker(key, ix, skip, float(os.environ.get("NPORE_SHARE_WAIT_S", "3600"))):
            return self._lib.npore_bam_open_mode(os.fsencode(path), threads, 2, os.fsencode(ix)) or None
        return None

    def _shared_copy(self, path, local_rank, threads):
        """Path to open: the inflated copy under /dev/shm (local rank 0 makes it, the others wait for it), or
        `path` itself when sharing is not possible (no room, or the maker gave up: a `.skip` marker)."""
        import shutil
        try:
            key = self._shm_key(path)
        except OSError:
            return path
        raw, skip = f"/dev/shm/npore_bam_{key}.raw", f"/dev/shm/npore_bam_{key}.skip"
        if local_rank == 0:
            self._announce_maker(key)
            self._shared = (raw, skip, key)
            h = self._lib.npore_bam_open_mode(os.fsencode(path), threads, 1, None)
            if not h:
                open(skip, "w").close()
                return path
            ok = False
            try:
                size = int(self._lib.npore_bam_inflated_size(h))
                if size * 4 <= shutil.disk_usage("/dev/shm").free:
                    ok = self._lib.npore_bam_dump_inflated(h, os.fsencode(raw + ".tmp")) == 0
            finally:
                self._lib.npore_bam_close(h)
            if not ok:
                open(skip, "w").close()
                return path
            os.replace(raw + ".tmp", raw)
            return raw
        return raw if self._wait_for_maker(key, raw, skip, float(os.environ.get("NPORE_SHARE_WAIT_S", "1800"))) else path

    def refs_with_reads(self):
        return {i for i in range(len(self.references)) if self._lib.npore_bam_ref_has_reads(self.handle, i)}

    def select(self, regions, max_reads=0, pass_mask=0):
        """Record indices of the reads get_read_data would yield for [(contig, start, stop)]; pass_mask (a subset of
        PASS_FLAGS): with the records of those flag bits, which a --pass_through run writes as they came (npore_bam_select_pass)."""
        ids = {n: i for i, n in enumerate(self.references)}
        rid = np.array([ids.get(c, -2) for c, _, _ in regions], np.int32)
        beg = np.array([s for _, s, _ in regions], np.int64)
        end = np.array([e for _, _, e in regions], np.int64)
        # two calls: the count first (cap = 0 writes nothing), then exactly that many entries -- a read overlapping
        # several regions is listed once per region, so n_records * n_regions is the only a-priori bound
        args = (self.handle, len(regions), rid.ctypes.data, beg.ctypes.data, end.ctypes.data, int(max_reads or 0))
        if pass_mask:
            return self._select_pass(args, int(pass_mask))
        k = self._lib.npore_bam_select(*args, None, 0)
        if k < 0:
            from . import _lib
            raise RuntimeError(_lib.last_error())
        out = np.zeros(max(int(k), 1), np.int64)
        k2 = self._lib.npore_bam_select(*args, out.ctypes.data, len(out))
        assert k2 == k
        return out[:k]

    def _select_pass(self, args, pass_mask):
        k = self._lib.npore_bam_select_pass(*args, pass_mask, None, 0)
        if k < 0:
            from . import _lib
            raise RuntimeError(_lib.last_error())
        out = np.zeros(max(int(k), 1), np.int64)
        k2 = self._lib.npore_bam_select_pass(*args, pass_mask, out.ctypes.data, len(out))
        assert k2 == k
        return out[:k]

    def fasta_map(self, fasta):
        """int32[n_refs]: index of each BAM reference in the FASTA (-1 if absent)."""
        pos = {n: i for i, n in enumerate(fasta.names)}
        return np.array([pos.get(n, -1) for n in self.references], np.int32)

    def pack(self, fasta, idx, threads=0):
        """(refs, ref_off, seqs, seq_off, cigs, cig_off) for npore_align_batch."""
        idx = np.ascontiguousarray(idx, np.int64)
        n = len(idx)
        ro, so, co = (np.zeros(n + 1, np.int64) for _ in range(3))
        self._check(self._lib.npore_bam_pack_sizes(self.handle, idx.ctypes.data, n, ro.ctypes.data, so.ctypes.data, co.ctypes.data))
        refs = np.zeros(int(ro[-1]) + 64, np.uint8)
        seqs = np.zeros(int(so[-1]) + 64, np.uint8)
        cigs = np.zeros(int(co[-1]) + 64, np.uint8)
        fmap = self.fasta_map(fasta)
        self._check(self._lib.npore_bam_pack(self.handle, fasta.handle, fmap.ctypes.data, idx.ctypes.data, n, refs.ctypes.data,
                                             ro.ctypes.data, seqs.ctypes.data, so.ctypes.data, cigs.ctypes.data,
                                             co.ctypes.data, threads))
        return refs, ro, seqs, so, cigs, co

    def format_sam(self, idx, finals, status, threads=0):
        """SAM text of the selected reads given their final collapsed CIGAR strings."""
        import ctypes as C
        _keep, reads = marshal_finals(idx, finals, status)
        sam, sam_len = C.c_void_p(), C.c_int64()
        self._check(self._lib.npore_bam_format_sam(self.handle, *reads, threads, C.byref(sam), C.byref(sam_len)))
        return C.string_at(sam.value, sam_len.value).decode() if sam_len.value else ""

    def format_bam(self, idx, finals, status, threads=0):
        """BAM records (bytes) of the selected reads given their final collapsed CIGAR strings (npore_bam_format_bam)."""
        import ctypes as C
        _keep, reads = marshal_finals(idx, finals, status)
        recs, recs_len = C.c_void_p(), C.c_int64()
        self._check(self._lib.npore_bam_format_bam(self.handle, *reads, threads, C.byref(recs), C.byref(recs_len)))
        return C.string_at(recs.value, recs_len.value) if recs_len.value else b""

    def format_bam_full(self, fasta, idx, finals, status, threads=0, md=False, cs=None, de=False, pass_mask=0, eqx=False, oc=False):
        """FULL records (bytes) of the selected reads given their final collapsed CIGAR strings (npore_bam_format_bam_full_pass,
        the widest entry of the ladder, whose narrower ones forward to it with zeros); md, cs, de, pass_mask, eqx, oc: as in
        OutputSpec."""
        import ctypes as C
        _keep, reads = marshal_finals(idx, finals, status)
        fmap = self.fasta_map(fasta)
        recs, recs_len = C.c_void_p(), C.c_int64()
        self._check(self._lib.npore_bam_format_bam_full_pass(self.handle, fasta.handle, fmap.ctypes.data, *reads, threads, C.byref(recs),
                                                             C.byref(recs_len), OUT_MD if md else 0, output_tags(cs, de, eqx, oc),
                                                             int(pass_mask)))
        return C.string_at(recs.value, recs_len.value) if recs_len.value else b""

    def set_output(self, out_format="sam", *more, **kw):
        """What the NEXT realign_file / realign_sequential / write_file on this handle appends to its output path (the setting
        holds for that one run): one OutputSpec, or the fields of one, in its order."""
        spec = out_format if isinstance(out_format, OutputSpec) else OutputSpec(out_format, *more, **kw)
        self._check(self._lib.npore_bam_set_output(self.handle, spec.format_word, os.fsencode(spec.bai) if spec.bai else None, spec.flags))
        if spec.tags:
            self._check(self._lib.npore_bam_set_output_tags(self.handle, spec.tags))
        if spec.pass_mask:
            self._check(self._lib.npore_bam_set_output_pass(self.handle, int(spec.pass_mask)))

    def output_info(self):
        """Of the last BAM-mode run: records written, bytes of the record stream, index (1 written, 0 none asked for, -1 the
        records were not in coordinate order), size of the file."""
        info = np.zeros(4, np.int64)
        self._check(self._lib.npore_bam_output_info(self.handle, info.ctypes.data))
        return dict(zip(("records", "stream_bytes", "indexed", "file_bytes"), (int(x) for x in info)))

    def inflate_info(self):
        """Of the last confusion / purity / realign_sequential run on the handle, the BGZF inflation on the device
        (Context.set("device_inflate", 1); npore_bam_inflate_info): blocks inflated on the device, blocks it declined that
        the host inflated, blocks whose CRC failed and went to the host, launches, nanoseconds of the kernel alone,
        compressed bytes copied up, inflated bytes copied down, 1 if the device inflation was installed.  All zeros after a
        run that inflated on the host."""
        info = np.zeros(8, np.int64)
        self._check(self._lib.npore_bam_inflate_info(self.handle, info.ctypes.data))
        return tuple(int(x) for x in info)

    def _after_bam_run(self, out_format):
        if out_format == "bam" and self.output_info()["indexed"] < 0:
            print(NOT_SORTED_MSG)

    def write_file(self, idx, finals, status, out_path, batch_reads=4000, threads=0, bai=None, eof=True, compress="none"):
        """The host's part of a BAM-mode run alone (npore_bam_write_file, no GPU): the selected reads with their final
        CIGARs as records, made in batches of batch_reads and appended to out_path."""
        _keep, reads = marshal_finals(idx, finals, status)
        self.set_output("bam", bai, eof, compress)
        self._check(self._lib.npore_bam_write_file(self.handle, *reads[:2], int(batch_reads), *reads[2:], threads, os.fsencode(out_path)))
        self._after_bam_run("bam")
        return self.output_info()

    @staticmethod
    def bai_path(path):
        """the file's .bai index (`x.bam.bai`, or `x.bai` beside `x.bam`), or None"""
        for cand in (path + ".bai", os.path.splitext(path)[0] + ".bai"):
            if os.path.exists(cand):
                return cand
        return None

    def set_share(self, rank, world, bai=None):
        """Several processes on this one-pass handle: process `rank` of `world` will walk a contiguous stretch of the record
        stream, cut at virtual offsets of the .bai linear index (npore_bam_set_share).  Raises OnePassUnsupported when
        there is no usable index (every rank then takes the indexed reader: the decision depends on the files alone)."""
        import ctypes as C
        bai = bai or self.bai_path(self.path)
        rc = self._lib.npore_bam_set_share(self.handle, int(rank), int(world), os.fsencode(bai) if bai else None)
        if rc == -5:
            from . import _lib
            raise OnePassUnsupported(_lib.last_error())
        self._check(rc)
        info = np.zeros(4, np.int64)
        self._check(self._lib.npore_bam_share_info(self.handle, info.ctypes.data))
        return tuple(int(x) for x in info)

    def realign_sequential(self, ctx, fasta, regions, out_path, batch_reads=4000, max_reads=0, r=30, max_b_rows=20000,
                           indel_start=5.0, indel_extend=1.0, threads=0, bad_cap=1000, output=None, **output_kw):
        """ONE PASS over the file: inflate, filter by `regions` [(contig, start, stop)] (at most one per contig, in header
        order), batch, realign, write -- npore_bam_realign_sequential.  Returns (reads selected, [(ordinal, status)] of
        the first bad reads, (refused, inconsistent)) -- the reads selected include the records that pass through (pass_mask),
        which are not bad reads; raises OnePassUnsupported when the regions or the file's
        order rule the one-pass run out (the caller truncates the output and takes the indexed path).
        output, or its fields as keywords: the OutputSpec of this run ("bam": records instead of text)."""
        output = output or OutputSpec(**output_kw)
        ids = {n: i for i, n in enumerate(self.references)}
        rid = np.array([ids.get(c, -2) for c, _, _ in regions], np.int32)
        beg = np.array([s for _, s, _ in regions], np.int64)
        end = np.array([e for _, _, e in regions], np.int64)
        if len(rid) and ((rid < 0).any() or (np.diff(rid) <= 0).any()):
            raise OnePassUnsupported("regions are not one per contig in header order")
        counts = np.zeros(3, np.int64)
        bad_ord, bad_st = np.zeros(max(bad_cap, 1), np.int64), np.zeros(max(bad_cap, 1), np.int32)
        fmap = self.fasta_map(fasta)
        self.set_output(output)
        rc = self._lib.npore_bam_realign_sequential(ctx.handle, self.handle, fasta.handle, fmap.ctypes.data, len(regions), rid.ctypes.data,
                                                    beg.ctypes.data, end.ctypes.data, int(max_reads or 0), int(batch_reads), indel_start,
                                                    indel_extend, max_b_rows, r, threads, os.fsencode(out_path), counts.ctypes.data,
                                                    bad_ord.ctypes.data, bad_st.ctypes.data, bad_cap)
        if rc == -5:
            from . import _lib
            msg = _lib.last_error()
            # only what rules the ONE-PASS run out sends the caller to the indexed reader; a band or chunk height the
            # kernels do not cover (the same code) would fail there in the same way, after a whole indexing pass
            if "one-pass ingest" in msg or "not sorted by reference" in msg:
                raise OnePassUnsupported(msg)
        if rc != 0:
            from . import _lib
            if "the index is stale" in _lib.last_error():
                raise StaleIndex(_lib.last_error())
        self._check(rc)
        self._after_bam_run(output.out_format)
        nb = int(min(bad_cap, counts[1] + counts[2]))
        return int(counts[0]), list(zip(bad_ord[:nb].tolist(), bad_st[:nb].tolist())), (int(counts[1]), int(counts[2]))

    def realign_batch(self, ctx, fasta, idx, r=30, max_b_rows=20000, indel_start=5.0, indel_extend=1.0, threads=0):
        """(SAM text, status[n]) of one batch: pack -> GPU align -> standardise -> format, all in the library."""
        import ctypes as C
        idx = np.ascontiguousarray(idx, np.int64)
        n = len(idx)
        st = np.zeros(max(n, 1), np.int32)
        fmap = self.fasta_map(fasta)
        sam, sam_len = C.c_void_p(), C.c_int64()
        self._check(self._lib.npore_bam_realign_batch(ctx.handle, self.handle, fasta.handle, fmap.ctypes.data, idx.ctypes.data, n,
                                                      indel_start, indel_extend, max_b_rows, r, threads,
                                                      C.byref(sam), C.byref(sam_len), st.ctypes.data))
        # a view of the library's buffer (valid until the next call on this handle): no copy before the file write
        return (memoryview((C.c_char * sam_len.value).from_address(sam.value)) if sam_len.value else memoryview(b"")), st[:n]

    def realign_file(self, ctx, fasta, idx, out_sam, batch_reads=4000, r=30, max_b_rows=20000, indel_start=5.0,
                     indel_extend=1.0, threads=0, output=None, **output_kw):
        """All selected reads, batch by batch, appended to out_sam by the library with packing, GPU work and
        formatting/writing of neighbouring batches overlapped.  Returns status[n] (ST_PASSED: written as it came).
        output, or its fields as keywords: the OutputSpec of this run ("bam": records instead of text); with a pass_mask, idx
        comes from select(..., pass_mask=pass_mask)."""
        output = output or OutputSpec(**output_kw)
        idx = np.ascontiguousarray(idx, np.int64)
        st = np.zeros(max(len(idx), 1), np.int32)
        fmap = self.fasta_map(fasta)
        self.set_output(output)
        self._check(self._lib.npore_bam_realign_file(ctx.handle, self.handle, fasta.handle, fmap.ctypes.data, idx.ctypes.data,
                                                     len(idx), int(batch_reads), indel_start, indel_extend, max_b_rows, r,
                                                     threads, os.fsencode(out_sam), st.ctypes.data))
        self._after_bam_run(output.out_format)
        return st[:len(idx)]

    def timing(self):
        """Host wall time (ms) of the stages of the last realign_batch."""
        ms = np.zeros(4, np.float64)
        self._lib.npore_bam_last_timing(self.handle, ms.ctypes.data, 4)
        return dict(zip(("pack_ms", "align_ms", "standardize_ms", "format_ms"), ms.tolist()))

    def file_timing(self):
        """Stage clocks (ms) of the last realign_file: per-stage sums over the batches (stages overlap), the wall time
        of the call, the GPU's kernel and PCIe time (npore_bam_file_timing)."""
        ms = np.zeros(8, np.float64)
        self._lib.npore_bam_file_timing(self.handle, ms.ctypes.data, 8)
        return dict(zip(("fetch_pack_ms", "align_call_ms", "standardize_ms", "format_ms", "write_ms", "wall_ms", "gpu_kernels_ms",
                         "pcie_ms"), ms.tolist()))

    def _check(self, rc):
        if rc != 0:
            from . import _lib
            raise RuntimeError(f"libnpore_amd: {rc} {_lib.last_error()}")

    def close(self):
        if self.handle:
            self._lib.npore_bam_close(self.handle)
            self.handle = None
        if self._shared:                 # the maker takes the shared copy away; a rank that comes later inflates itself
            raw, skip, key = self._shared
            self._shared = None
            try:
                open(skip, "w").close()
            except OSError:
                pass
            for f in (raw, raw + ".tmp", f"/dev/shm/npore_bam_{key}.pid"):
                try:
                    os.remove(f)
                except OSError:
                    pass
            import atexit                # the marker for late comers goes when this process does
            atexit.register(lambda f=skip: os.path.exists(f) and os.remove(f))


def realign_native(ctx, bam, fasta, idx, out_sam, r=30, max_b_rows=20000, batch_reads=0, threads=0, output=None, **output_kw):
    """realign_reads() through the library; returns the number of reads handed in.  batch_reads > 0: the whole
    index list in overlapped batches written by the library itself; 0: one batch, text written here.
    threads: host threads of the parallel host stages (0 = all cores; one process per GPU: dist.host_threads_per_rank).
    output, or its fields as keywords: the OutputSpec of the run; "bam" needs batch_reads > 0: the library writes the file."""
    output = output or OutputSpec(**output_kw)
    if output.out_format == "bam" and batch_reads <= 0:
        raise ValueError("BAM output is written by the library's file pipeline: batch_reads must be positive")
    if len(idx) == 0 and output.out_format != "bam":
        return 0
    if batch_reads > 0:
        text, status = None, bam.realign_file(ctx, fasta, idx, out_sam, batch_reads=batch_reads, r=r, max_b_rows=max_b_rows,
                                              threads=threads, output=output)
    else:
        text, status = bam.realign_batch(ctx, fasta, idx, r=r, max_b_rows=max_b_rows, threads=threads)
    bad = np.nonzero(np.asarray(status) & ~ST_PASSED)[0]       # (a record that passed through is no bad read)
    for k in bad:
        if status[k] & 32:
            print(f"\nERROR: read #{int(idx[k])}: CIGAR does not match sequence lengths; skipped.")
        else:
            print(f"\nERROR: inconsistent traceback for read #{int(idx[k])} (status {int(status[k])})")   # src/aln.pyx:689-716
    if text is not None:
        with open(out_sam, "ab") as fh:
            fh.write(text)
    return len(idx)


# ---- confusion matrices (reference src/bam.pyx:166-200, 301-316, 351-499) ----------------------------------------
def get_pileups(bam_path, ctg, start, end):
    """Column 5 of `samtools mpileup -r ctg:start+1-end bam`, upper-cased, one string per reported position
    (reference src/bam.pyx:301-316).  Needs samtools on PATH, like the reference."""
    import shutil
    import subprocess
    if not shutil.which("samtools"):
        print("\nERROR: recalculating the confusion matrices needs `samtools` (mpileup) on PATH.")
        sys.exit(1)
    pile = subprocess.Popen(["samtools", "mpileup", "-r", f"{ctg}:{start + 1}-{end}", bam_path],
                            stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    for line in pile.stdout:
        f = line.decode("utf-8").rstrip("\n").split("\t")
        yield (f[4] if len(f) > 4 else "").upper().strip()


def calc_confusion_matrices(range_tuple, pileups=None, refs=None, np_info=None, threads=0):
    """Reference src/bam.pyx:351-499 for one range (ctg, start, end): (subs[5,5], nps[max_n,max_l+1,max_l+1],
    inss[max_l+1], dels[max_l+1]) int64 counts of the basecaller's errors against the reference.
    pileups: iterable of column-5 strings (default: samtools, get_pileups); refs: {contig: sequence} (default
    cfg.args.refs); np_info: get_np_info of refs[ctg][start:end+1] (default: aln.get_np_info, on the GPU).
    The character loop runs in the library (csrc/confusion.hpp) on all host cores."""
    import ctypes as C
    from . import _lib, aln
    from .cig import bases_to_int
    lib = _lib.load()
    ctg, start, end = range_tuple
    refs = cfg.args.refs if refs is None else refs
    max_n, max_l = int(cfg.args.max_n), int(cfg.args.max_l)
    contig = refs[ctg]
    if pileups is None:
        pileups = get_pileups(cfg.args.bam, ctg, start, end)
    lines = [p.upper().strip().encode() for p in pileups]
    if np_info is None:
        np_info = aln.get_np_info(bases_to_int(contig[start:end + 1]))
    np_info = np.ascontiguousarray(np_info, dtype=np.int32)
    codes = np.ascontiguousarray(bases_to_int(contig[start:end]), dtype=np.uint8)
    # (the character loop only looks at ref_text[pos+1 .. pos+1+max_n) of the range's positions; Python's slice clipping
    # at the contig end is what the reference's contig[...] slices do there)
    text = contig[start:end + max_n + 1].upper().encode()
    off = np.zeros(len(lines) + 1, np.int64)
    np.cumsum([len(x) for x in lines], out=off[1:])
    buf = b"".join(lines) + b"\0"
    subs = np.zeros((cfg.nbases, cfg.nbases), np.int64)
    nps = np.zeros((max_n, max_l + 1, max_l + 1), np.int64)
    inss = np.zeros(max_l + 1, np.int64)
    dels = np.zeros(max_l + 1, np.int64)
    bad = C.c_int64(0)
    rc = lib.npore_confusion_counts(buf, off.ctypes.data, len(lines), codes.ctypes.data, len(codes), text, len(text),
                                    np_info.ctypes.data, len(np_info), max_n, max_l, subs.ctypes.data, nps.ctypes.data,
                                    inss.ctypes.data, dels.ctypes.data, C.byref(bad), threads)
    if rc:
        raise RuntimeError(_lib.last_error())
    if bad.value:
        print(f"ERROR: unexpected character in {bad.value} pileup line(s) of {ctg}:{start}-{end}.")   # src/bam.pyx:473-476
    return subs, nps, inss, dels


CMS_TALLIES = ("records", "records_flagged", "records_refskip", "records_malformed", "adjacent_indels", "entries_ambiguous",
               "entries_lowq", "entries_counted", "batches", "kernel_ns")


def confusion_from_bam(ctx, bam, fasta, ranges, min_bq=13, exclude_flags=0x704):
    """The four count matrices of calc_confusion_matrices straight from the BAM records, counted on the GPU
    (npore_bam_confusion; the rule: csrc/confusion_rec.hpp) -- no pileup text, no samtools.
    ctx: an aln.Context (an annotation-only one will do; max_n / max_l are its own); bam: a path or a NativeBam; fasta: a
    path or a NativeFasta; ranges: [(contig, start, stop)] as bed.get_ranges(cfg.args.regions, chunk_width) makes them.
    A path is read in ONE PASS where the reader's rules allow it (a BGZF file sorted by reference), else through the
    record index.  min_bq / exclude_flags: the defaults of `samtools mpileup` (-Q 13; UNMAP, SECONDARY, QCFAIL, DUP).
    Position-true: a position nobody covers adds nothing (the text route shifts behind a coverage gap); no depth cap
    (mpileup -d) and no handling of overlapping mates.  Returns (subs, nps, inss, dels, tallies): int64 matrices
    and a dict of CMS_TALLIES -- `adjacent_indels` counts the I / D operations that follow another I / D (or lead a read)
    and are not counted, because pileup programs place their markers differently."""
    from . import _lib
    lib = _lib.load()
    own_fa = not isinstance(fasta, NativeFasta)
    fa = NativeFasta(fasta) if own_fa else fasta
    max_n, max_l = ctx.max_n, ctx.max_l

    def run(b):
        ids = {n: i for i, n in enumerate(b.references)}
        rid = np.array([ids.get(c, -1) for c, _, _ in ranges], np.int32)
        beg = np.array([s for _, s, _ in ranges], np.int64)
        end = np.array([e for _, _, e in ranges], np.int64)
        subs = np.zeros((cfg.nbases, cfg.nbases), np.int64)
        nps = np.zeros((max_n, max_l + 1, max_l + 1), np.int64)
        inss, dels, tallies = np.zeros(max_l + 1, np.int64), np.zeros(max_l + 1, np.int64), np.zeros(16, np.int64)
        fmap = b.fasta_map(fa)
        rc = lib.npore_bam_confusion(ctx.handle, b.handle, fa.handle, fmap.ctypes.data, len(ranges), rid.ctypes.data, beg.ctypes.data,
                                     end.ctypes.data, int(min_bq), int(exclude_flags), subs.ctypes.data, nps.ctypes.data,
                                     inss.ctypes.data, dels.ctypes.data, tallies.ctypes.data)
        if rc == -5 and b.one_pass:
            raise OnePassUnsupported(_lib.last_error())
        if rc:
            raise RuntimeError(f"libnpore_amd: {rc} {_lib.last_error()}")
        return subs, nps, inss, dels, dict(zip(CMS_TALLIES, tallies.tolist()))

    try:
        if isinstance(bam, NativeBam):
            return run(bam)
        if NativeBam.is_bgzf(bam) and os.environ.get("NPORE_BAM_ONE_PASS", "1") != "0":
            b = NativeBam(bam, one_pass=True)
            try:
                return run(b)
            except OnePassUnsupported:
                pass                             # (not sorted by reference: nothing was added, the indexed reader counts)
            finally:
                b.close()
        b = NativeBam(bam, share=False)
        try:
            return run(b)
        finally:
            b.close()
    finally:
        if own_fa:
            fa.close()


def get_confusion_matrices():
    """Reference src/bam.pyx:166-200: the cached count matrices of --stats_dir, or (--recalc_cms) counted from the
    BAM range by range (cfg.args.regions cut into --chunk_width pieces), summed and cached there.
    Loading defaults to the shipped guppy5_stats; a recount is written to --stats_dir (default ./stats, like the
    reference) and NEVER into the package's data directory.  Several processes (torch.distributed.run): rank 0
    recounts and writes (temp file + rename), the others wait at a barrier and load."""
    shipped = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "guppy5_stats")
    names = ("subs", "nps", "inss", "dels")
    if not getattr(cfg.args, "recalc_cms", False):
        d = cfg.args.stats_dir or shipped
        print("> loading confusion matrices")
        return tuple(np.load(os.path.join(d, f"{k}_cm.npy")) for k in names)
    d = cfg.args.stats_dir or "./stats"
    if os.path.realpath(d) == os.path.realpath(shipped):
        print("\nERROR: --recalc_cms would overwrite the shipped guppy5_stats tables; give another --stats_dir.")
        sys.exit(1)
    from . import dist as dist_mod

    def recount():
        print("> calculating confusion matrices")
        from .bed import get_ranges
        total = None
        ranges = get_ranges(cfg.args.regions, cfg.args.chunk_width)
        if getattr(cfg.args, "cms_source", "mpileup") == "bam" and ranges:
            # straight from the records, on the GPU (confusion_from_bam): an annotation-only context of its own
            from . import aln
            ctx = aln.Context(None, None, device=int(getattr(cfg.args, "device", 0)) % max(aln.device_count(), 1))
            ctx.set("device_inflate", getattr(cfg.args, "bam_inflate", "host") == "device")
            try:
                *total, tallies = confusion_from_bam(ctx, cfg.args.bam, cfg.args.ref, ranges, min_bq=cfg.args.cms_min_bq,
                                                     exclude_flags=cfg.args.cms_exclude_flags)
            finally:
                ctx.close()
            total = tuple(total)
            print(f"    {tallies['records']} records, {tallies['entries_counted']} bases counted in {len(ranges)} chunks; left out: "
                  f"{tallies['entries_lowq']} bases below the quality bound, {tallies['entries_ambiguous']} ambiguous letters, "
                  f"{tallies['adjacent_indels']} adjacent INDELs, {tallies['records_flagged']} records by flags, "
                  f"{tallies['records_refskip']} with N / P, {tallies['records_malformed']} malformed.")
            ranges = []
        for k, rg in enumerate(ranges):
            res = calc_confusion_matrices(rg)
            total = res if total is None else tuple(a + b for a, b in zip(total, res))
            print(f"\r    {k + 1} of {len(ranges)} chunks processed.", end="", flush=True)
        print(" ")
        if total is None:
            total = calc_confusion_matrices(("", 0, 0), pileups=[], refs={"": ""},
                                            np_info=np.zeros((0, 2, int(cfg.args.max_n)), np.int32))
        os.makedirs(d, exist_ok=True)
        for k, m in zip(names, total):
            tmp = os.path.join(d, f".{k}_cm.{os.getpid()}.tmp.npy")
            np.save(tmp, m)
            os.replace(tmp, os.path.join(d, f"{k}_cm.npy"))
        return total

    # several ranks: rank 0 recounts; the others learn whether it succeeded (no barrier that never comes, no 30-minute
    # default timeout on a step that takes hours on a genome)
    total = dist_mod.rank0_then_all(recount)
    if total is None:
        total = tuple(np.load(os.path.join(d, f"{k}_cm.npy")) for k in names)
    if getattr(cfg.args, "recalc_exit", False):
        sys.exit(0)
    return total


def write_bai(bam_path, bai_path=None, bins=False):
    """A .bai for a BAM file (tests / benchmarks; `samtools index` makes the real ones): the LINEAR index -- per
    reference and 16 kb window the virtual offset (block offset << 16 | offset in the block) of the first record that
    overlaps the window, SAM specification 5.2 -- which is all npore_bam_set_share reads; no bins unless `bins`: then
    every bin with its chunks, neighbouring records of a bin merged into one (the --python_io BAM writer)."""
    raw = open(bam_path, "rb").read()
    blocks, p, u = [], 0, 0                      # (compressed offset, inflated offset) of every BGZF block
    parts = []
    while p < len(raw):
        xlen = struct.unpack_from("<H", raw, p + 10)[0]
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        data = zlib.decompress(raw[p + 12 + xlen:p + bsize - 8], -15)
        blocks.append((p, u))
        parts.append(data)
        u += len(data)
        p += bsize
    data = b"".join(parts)
    starts = np.array([b[1] for b in blocks], np.int64)
    coffs = np.array([b[0] for b in blocks], np.int64)
    l_text, = struct.unpack_from("<i", data, 4)
    q = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, q); q += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, q); q += 8 + l_name
    lin = [dict() for _ in range(n_ref)]
    binned = [dict() for _ in range(n_ref)]
    sizes = [len(x) for x in parts]

    def voff_end(e):
        """where a record ends: in the member that holds its last byte, or (that member being full) at the next one's start"""
        k = int(np.searchsorted(starts, e - 1, side="right")) - 1
        if e - int(starts[k]) == sizes[k] == 0xFF00 and k + 1 < len(blocks):
            return int(coffs[k + 1]) << 16
        return (int(coffs[k]) << 16) | (e - int(starts[k]))
    ref_len_of_op = (1, 0, 1, 1, 0, 0, 0, 1, 1)  # MIDNSHP=X consume the reference?
    while q + 4 <= len(data):
        bs, = struct.unpack_from("<i", data, q)
        rid, pos, l_rn, _mq, _bin, n_cig, _flag, _l_seq = struct.unpack_from("<iiBBHHHi", data, q + 4)
        k = int(np.searchsorted(starts, q, side="right")) - 1
        while starts[k] == q and k > 0 and starts[k - 1] == q:      # (empty blocks: the first of them)
            k -= 1
        v = (int(coffs[k]) << 16) | (q - int(starts[k]))
        if rid >= 0:
            cig = struct.unpack_from(f"<{n_cig}I", data, q + 36 + l_rn)
            end = pos + max(1, sum((c >> 4) * ref_len_of_op[c & 15] for c in cig))
            for w in range(pos >> 14, ((end - 1) >> 14) + 1):
                lin[rid].setdefault(w, v)
            if bins:
                chunks = binned[rid].setdefault(reg2bin(pos, end), [])
                ve = voff_end(q + 4 + bs)
                if chunks and chunks[-1][1] == v:
                    chunks[-1][1] = ve
                else:
                    chunks.append([v, ve])
        q += 4 + bs
    out = bytearray(b"BAI\1" + struct.pack("<i", n_ref))
    for d, bn in zip(lin, binned):
        out += struct.pack("<i", len(bn))                            # (no bins unless asked for)
        for b_id in sorted(bn):
            out += struct.pack("<Ii", b_id, len(bn[b_id]))
            for c0, c1 in bn[b_id]:
                out += struct.pack("<QQ", c0, c1)
        n_intv = (max(d) + 1) if d else 0
        out += struct.pack("<i", n_intv)
        last = 0
        for w in range(n_intv):                                      # (windows without a record: the previous entry, as samtools does)
            last = d.get(w, last)
            out += struct.pack("<Q", last)
    bai_path = bai_path or bam_path + ".bai"
    with open(bai_path, "wb") as fh:
        fh.write(bytes(out))
    return bai_path


def read_bai(path):
    """[(bins {bin: [(chunk_beg, chunk_end)]}, linear [ioffset])] per reference of a .bai file."""
    raw = open(path, "rb").read()
    if raw[:4] != b"BAI\1":
        raise ValueError(f"'{path}' is not a .bai file")
    n_ref, = struct.unpack_from("<i", raw, 4)
    q, out = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", raw, q); q += 4
        bins = {}
        for _ in range(n_bin):
            b_id, n_chunk = struct.unpack_from("<Ii", raw, q); q += 8
            v = struct.unpack_from(f"<{2 * n_chunk}Q", raw, q); q += 16 * n_chunk
            bins[b_id] = list(zip(v[0::2], v[1::2]))
        n_intv, = struct.unpack_from("<i", raw, q); q += 4
        out.append((bins, list(struct.unpack_from(f"<{n_intv}Q", raw, q)))); q += 8 * n_intv
    return out


def pack_bai(refs):
    """read_bai's list as the bytes of a .bai file."""
    out = bytearray(b"BAI\1" + struct.pack("<i", len(refs)))
    for bins, lin in refs:
        out += struct.pack("<i", len(bins))
        for b_id in sorted(bins):
            out += struct.pack("<Ii", b_id, len(bins[b_id]))
            for c0, c1 in bins[b_id]:
                out += struct.pack("<QQ", c0, c1)
        out += struct.pack("<i", len(lin)) + struct.pack(f"<{len(lin)}Q", *lin)
    return bytes(out)


def merge_bai_parts(parts):
    """One index from the index sidecars of the parts of a file, [(read_bai list, where the part begins in the file)] in
    file order: compressed offsets shifted (a sidecar counts from PART_BASE), a bin's chunk lists joined, per linear window the first
    entry (a part's windows in front of its first record hold 0; those it filled forward lie in front of every later
    part's records), empty windows filled forward again.  None when the parts are not in coordinate order (a later part
    has records on an earlier reference than the part before)."""
    n_ref = max((len(p) for p, _ in parts), default=0)
    merged = [({}, []) for _ in range(n_ref)]
    last_ref = -1
    for refs, shift in parts:
        shift -= PART_BASE
        used = [k for k, (bins, lin) in enumerate(refs) if bins or any(lin)]
        if used and used[0] < last_ref:
            return None
        if used:
            last_ref = used[-1]
        for k, (bins, lin) in enumerate(refs):
            mb, ml = merged[k]
            for b_id, chunks in bins.items():
                mb.setdefault(b_id, []).extend((c0 + (shift << 16), c1 + (shift << 16)) for c0, c1 in chunks)
            ml.extend([0] * (len(lin) - len(ml)))
            for w, v in enumerate(lin):
                if v and not ml[w]:
                    ml[w] = v + (shift << 16)
    for _, ml in merged:
        last = 0
        for w, v in enumerate(ml):
            last = ml[w] = v or last
    return merged


def write_bam(path, references, records, level=6):
    """Write a BAM file (tests / benchmarks).  references: [(name, length)]; records: dicts with
    name, flag, ref_id, pos, mapq, cigar [(op, len)], seq (str over =ACMGRSVTWYHKDBN), qual (bytes or None),
    hp (int or None); optional: tags (raw tag bytes written in front of HP), long_cigar (True: the CIGAR goes out as
    the placeholder <l_seq>S<reflen>N with the real words in a CG:B,I tag behind HP, as for every record of more than
    65 535 operations; "i": the same with subtype i; "front": the CG tag in front of `tags` and HP), next_ref_id, next_pos,
    tlen (the mate fields; -1, -1, 0 without)."""
    ref_len_of_op = (1, 0, 1, 1, 0, 0, 0, 1, 1)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in references)
    out = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(references)))
    for n, l in references:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    code = {c: i for i, c in enumerate(_SEQ16)}
    for r in records:
        name = r["name"].encode() + b"\0"
        seq = r["seq"]
        nib = np.array([code[c] for c in seq] + ([0] if len(seq) & 1 else []), np.uint8)
        packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes() if len(seq) else b""
        qual = r.get("qual")
        qual = bytes([0xFF]) * len(seq) if qual is None else bytes(qual)
        cig = np.array([(ln << 4) | op for op, ln in r["cigar"]], "<u4").tobytes()
        aux = bytes(r.get("tags", b"")) + (b"" if r.get("hp") is None else b"HPC" + bytes([r["hp"]]))
        long_cigar = r.get("long_cigar") or len(r["cigar"]) > MAX_CIGAR_OPS
        if long_cigar:
            cg = b"CGB" + (b"i" if long_cigar == "i" else b"I") + struct.pack("<I", len(r["cigar"])) + cig
            aux = cg + aux if long_cigar == "front" else aux + cg
            reflen = sum(ln * ref_len_of_op[op] for op, ln in r["cigar"])
            cig = struct.pack("<II", (len(seq) << 4) | 4, (reflen << 4) | 3)
        body = struct.pack("<iiBBHHHiiii", r["ref_id"], r["pos"], len(name), r.get("mapq", 60), 4680, len(cig) // 4,
                           r["flag"], len(seq), r.get("next_ref_id", -1), r.get("next_pos", -1), r.get("tlen", 0)) + name + cig + packed + qual + aux
        out += struct.pack("<i", len(body)) + body
    with open(path, "wb") as fh:
        for p in range(0, len(out), 0xFF00):      # BGZF blocks of < 64 KiB
            chunk = bytes(out[p:p + 0xFF00])
            comp = zlib.compressobj(level, zlib.DEFLATED, -15)
            data = comp.compress(chunk) + comp.flush()
            fh.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(data) + 25))
            fh.write(data)
            fh.write(struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))   # BGZF EOF block
