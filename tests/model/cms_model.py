"""TEST INFRASTRUCTURE for the recount of the confusion matrices from BAM records (npore_amd/csrc/confusion_rec.hpp).

Three independent statements of the same rule meet here:
  * write_pileups(): a Python pileup writer that implements the rule of confusion_rec.hpp entry by entry and writes one
    column-5 line per position of a range (an empty line where nothing is counted), with its own tallies -- also of the
    branches of the counting loop an input exercises;
  * expected(): those lines through bam.calc_confusion_matrices, the character loop pinned to the reference's compiled
    code by tests/golden/cms.json, summed over the ranges;
  * twin_count(): confusion_rec.hpp itself compiled by g++ (tests/model/confusion_rec.cpp), built lazily like bam_walk.py.
make_random_bam() is the seeded generator of the random inputs."""
import argparse
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
TALLY_NAMES = ("records", "records_flagged", "records_refskip", "records_malformed", "adjacent_indels", "entries_ambiguous",
               "entries_lowq", "entries_counted")
M_OPS = (0, 7, 8)


def build(force=False):
    so = os.path.join(_HERE, "libconfusion_rec.so")
    csrc = os.path.join(_HERE, "..", "..", "npore_amd", "csrc")
    deps = [os.path.join(_HERE, "confusion_rec.cpp")] + [
        os.path.join(csrc, f) for f in ("confusion_rec.hpp", "bam_reader.hpp", "hostio.hpp", "inflate.hpp", "crc32.hpp", "glue.hpp",
                                        "std_stream.hpp")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", so, deps[0], "-lz", "-lpthread"])
    return so


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(build())
        lib.cms_twin_count.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 5 + \
            [C.c_int, C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 5
        lib.cms_twin_count.restype = C.c_int
        lib.cms_twin_last_error.restype = C.c_char_p
        _LIB = lib
    return _LIB


def planes_of(info):
    """get_np_info's int32 [len, 2, max_n] as the byte planes the device writes: [max_n, len] of L | start << 7"""
    info = np.asarray(info)
    L, idx = info[:, 0, :], info[:, 1, :]
    return np.ascontiguousarray(((L & 0x7F) | (((L != 0) & (idx == 0)) << 7)).astype(np.uint8).T)


INFO_HOOK = None      # tests: callable(seq, info) -> info, applied to every annotation the writer, expected() and the twin use


def _oracle_info(seq, max_n, max_l):
    import oracle
    from npore_amd.cig import bases_to_int
    info = oracle.get_np_info(bases_to_int(seq), max_n=max_n, max_l=max_l)
    return INFO_HOOK(seq, info) if INFO_HOOK else info


def _clip(refs, rg):
    c, st, en = rg
    return c, max(0, st), min(en, len(refs[c]))


def twin_count(bam_path, references, refs, ranges, max_n, max_l, min_bq=13, exclude_flags=0x704):
    """confusion_rec.hpp on the host: (subs, nps, inss, dels, tallies dict).  references: the BAM header's names;
    refs: {contig: upper-cased sequence}; ranges: [(contig, start, stop)]."""
    lib = load()
    ids = {n: i for i, n in enumerate(references)}
    text = "".join(refs.get(n, "") for n in references).encode()
    off = np.zeros(len(references) + 1, np.int64)
    np.cumsum([len(refs.get(n, "")) for n in references], out=off[1:])
    planes, ann, at = [], [], 0
    for rg in ranges:
        c, st, en = _clip(refs, rg)
        ann.append(at)
        if st < en:
            pl = planes_of(_oracle_info(refs[c][st:en + 1], max_n, max_l))
            planes.append(pl.reshape(-1))
            at += pl.size
    planes = np.concatenate(planes + [np.zeros(8, np.uint8)])
    rid = np.array([ids.get(c, -1) for c, _, _ in ranges], np.int32)
    beg = np.array([s for _, s, _ in ranges], np.int64)
    end = np.array([e for _, _, e in ranges], np.int64)
    ann = np.array(ann, np.int64)
    subs = np.zeros((5, 5), np.int64)
    nps = np.zeros((max_n, max_l + 1, max_l + 1), np.int64)
    inss, dels, tallies = np.zeros(max_l + 1, np.int64), np.zeros(max_l + 1, np.int64), np.zeros(16, np.int64)
    rc = lib.cms_twin_count(os.fsencode(bam_path), text, off.ctypes.data, len(references), len(ranges), rid.ctypes.data, beg.ctypes.data,
                            end.ctypes.data, ann.ctypes.data, planes.ctypes.data, max_n, max_l, min_bq, exclude_flags,
                            subs.ctypes.data, nps.ctypes.data, inss.ctypes.data, dels.ctypes.data, tallies.ctypes.data)
    if rc:
        raise RuntimeError(f"{rc}: {lib.cms_twin_last_error().decode()}")
    return subs, nps, inss, dels, dict(zip(TALLY_NAMES, tallies.tolist()))


def write_pileups(records, references, refs, ranges, max_n, max_l, min_bq=13, exclude_flags=0x704):
    """The rule of confusion_rec.hpp as a pileup writer.  records: bam.BamFile(...).records.  Returns (lines, tallies):
    lines[k] = the column-5 strings of range k, one per position; tallies: the record / entry tallies of TALLY_NAMES and
    the branches of the counting loop the input reached."""
    tallies = collections.Counter({k: 0 for k in TALLY_NAMES})
    clipped = [_clip(refs, rg) if rg[0] in refs else (rg[0], 0, 0) for rg in ranges]
    cols = [[[] for _ in range(st, en)] for _, st, en in clipped]
    infos = [_oracle_info(refs[c][st:en + 1], max_n, max_l) if st < en else None for c, st, en in clipped]
    for rec in records:
        if rec.ref_id < 0 or rec.ref_id >= len(references):
            continue
        ctg = references[rec.ref_id]
        mine = [(k, st, en) for k, (c, st, en) in enumerate(clipped) if c == ctg and st < en]
        pos = rec.reference_start
        rl = sum(n for op, n in rec.cigar if op in (0, 2, 3, 7, 8))
        ql = sum(n for op, n in rec.cigar if op in (0, 1, 4, 7, 8))
        if pos < 0 or rl <= 0 or not any(pos < en and pos + rl > st for _, st, en in mine):
            continue
        if rec.flag & exclude_flags:
            tallies["records_flagged"] += 1
            continue
        if any(op in (3, 6) for op, _ in rec.cigar):
            tallies["records_refskip"] += 1
            continue
        if ql != len(rec.seq):
            tallies["records_malformed"] += 1
            continue
        tallies["records"] += 1
        contig, clen = refs[ctg], len(refs[ctg])
        vis, r, q = [], pos, 0                     # the operations one sees: S, H and empty ones stepped over
        for op, n in rec.cigar:
            if n > 0 and op not in (4, 5):
                vis.append((op, n, r, q))
            r += n if op in (0, 2, 3, 7, 8) else 0
            q += n if op in (0, 1, 4, 7, 8) else 0
        for k, (op, n, r0, q0) in enumerate(vis):
            if op in (1, 2) and (k == 0 or vis[k - 1][0] not in M_OPS):
                tallies["adjacent_indels"] += 1
            if op not in M_OPS:
                continue
            for t in range(n):
                a, b, qv = r0 + t, rec.seq[q0 + t], rec.qual[q0 + t]
                kind, kk, ins = "", 0, ""
                if t == n - 1 and k + 1 < len(vis) and vis[k + 1][0] in (1, 2):
                    nop, kk, _, nq = vis[k + 1]
                    kind, ins = ("+", rec.seq[nq:nq + kk]) if nop == 1 else ("-", "N" * kk)
                if not 0 <= a < clen:
                    continue
                for g, st, en in mine:
                    if not st <= a < en:
                        continue
                    if qv != 0xFF and qv < min_bq:
                        tallies["entries_lowq"] += 1
                        tallies["lowq_with_marker"] += bool(kind)
                        continue
                    if b not in "ACGTN":
                        tallies["entries_ambiguous"] += 1
                        continue
                    tallies["entries_counted"] += 1
                    cols[g][a - st].append(b + (f"{kind}{kk}{ins}" if kind else ""))
                    tallies["on_range_last_position"] += a == en - 1
                    # which branches of the counting loop this entry reaches
                    info, p = infos[g], a - st + 1
                    starts = [m for m in range(1, max_n + 1) if p < len(info) and info[p, 0, m - 1] != 0 and info[p, 1, m - 1] == 0]
                    if kind:
                        tallies["indel_k_ge_max_l"] += kk >= max_l
                        cnv = False
                        for m in starts:
                            L = int(info[p, 0, m - 1])
                            if kind == "-" and kk % m == 0 and kk <= L * m:
                                cnv = True
                                tallies["copy_deletion"] += 1
                            if kind == "+" and kk % m == 0 and contig[a + 1:a + 1 + m] * (kk // m) == ins:
                                cnv = True
                                tallies["copy_insertion"] += 1
                        tallies["noncopy_indel_at_start"] += bool(starts) and not cnv
                        # the unit contig[a+1 : a+1+m] of a period that divides k is cut short by the contig's end (the loop
                        # itself compares only at a polymer start, and a start has three whole repeats inside the contig)
                        tallies["insertion_unit_clipped"] += kind == "+" and any(kk % m == 0 and a + 1 + m > clen for m in range(1, max_n + 1))
    lines = [["".join(x) for x in c] for c in cols]
    return lines, tallies


def expected(bam_path, refs, ranges, max_n, max_l, min_bq=13, exclude_flags=0x704):
    """((subs, nps, inss, dels), writer tallies): the writer's lines through the G7-pinned character loop, summed over
    the ranges, the annotation from the oracle."""
    from npore_amd import bam, cfg
    f = bam.BamFile(bam_path)
    lines, tallies = write_pileups(f.records, f.references, refs, ranges, max_n, max_l, min_bq, exclude_flags)
    total = [np.zeros((5, 5), np.int64), np.zeros((max_n, max_l + 1, max_l + 1), np.int64), np.zeros(max_l + 1, np.int64),
             np.zeros(max_l + 1, np.int64)]
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=max_n, max_l=max_l)
    try:
        for rg, ln in zip(ranges, lines):
            if rg[0] not in refs:
                continue
            c, st, en = _clip(refs, rg)
            if st >= en:
                continue
            res = bam.calc_confusion_matrices((c, st, en), pileups=ln, refs=refs, np_info=_oracle_info(refs[c][st:en + 1], max_n, max_l))
            total = [a + b for a, b in zip(total, res)]
    finally:
        cfg.args = old
    return tuple(total), tallies


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def tallies_agree(got, want):
    return all(int(got[k]) == int(want[k]) for k in TALLY_NAMES)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def engineered_contig():
    """the second contig of tests/golden/make_golden_cms.py"""
    return "ACGT" + "A" * 7 + "CG" * 5 + "TTAGGG" * 4 + "ACGTAC" + "T" * 120 + "GATTACA"


def engineered_records():
    """Reads on the engineered contig that carry, as records, what make_golden_cms.py wrote as lines: copies gained and
    lost at the homopolymer, the dinucleotide and the hexamer repeat, others, lengths beyond max_l, an insertion on the
    contig's last bases."""
    ctg = engineered_contig()
    out = []

    def read(pos, parts, flag=0, qual=None):
        """parts: ('M', n) takes the contig's bases, ('X', bases) other bases, ('I', bases), ('D', n), ('S', bases)"""
        cigar, seq, r = [], "", pos
        for kind, v in parts:
            if kind == "M":
                cigar.append((0, v)); seq += ctg[r:r + v]; r += v
            elif kind == "X":
                cigar.append((8, len(v))); seq += v; r += len(v)
            elif kind == "I":
                cigar.append((1, len(v))); seq += v
            elif kind == "D":
                cigar.append((2, v)); r += v
            elif kind == "S":
                cigar.append((4, len(v))); seq += v
        out.append({"name": f"e{len(out)}", "flag": flag, "ref_id": 0, "pos": pos, "cigar": cigar, "seq": seq,
                    "qual": qual if qual is None else bytes(qual[:len(seq)] + [30] * max(0, len(seq) - len(qual)))})

    n = len(ctg)
    for ins in ("A", "AA", "C", "AAAAAAA"):
        read(0, [("M", 4), ("I", ins), ("M", 30)])
    for d in (1, 2, 3, 7, 8):
        read(1, [("M", 3), ("D", d), ("M", 40)])
    for ins in ("CG", "CGCG", "GC", "CGC", "CGCGCGCGCGCG"):
        read(2, [("M", 9), ("I", ins), ("M", 25)], flag=16)
    for d in (2, 4, 10, 12, 3):
        read(0, [("S", "TTT"), ("M", 11), ("D", d), ("M", 30)])
    for ins in ("TTAGGG", "TTAGGA", "TTAGGGTTAGGG", "TTA"):
        read(5, [("M", 16), ("I", ins), ("M", 40)])
    for d in (6, 12, 24, 30, 5):
        read(5, [("M", 16), ("D", d), ("M", 20)])
    read(40, [("M", 11), ("I", "T" * 150), ("M", 60)])               # beyond max_l, inside the long homopolymer
    read(40, [("M", 11), ("D", 110), ("M", 5)])
    read(45, [("M", 6), ("I", "T"), ("M", 20)])                      # at the homopolymer's start (it begins at 51)
    read(45, [("M", 6), ("D", 1), ("M", 20)])
    read(45, [("M", 6), ("D", 120), ("M", 3)])
    read(45, [("M", 6), ("I", "T" * 101), ("M", 30)])
    read(n - 20, [("M", 19), ("I", "AA"), ("M", 1)])                 # the unit of the compare is cut by the contig's end
    read(n - 20, [("M", 20), ("I", "GG")])
    read(n - 30, [("M", 10), ("X", "NRYN"), ("M", 16)])              # N and IUPAC letters
    read(0, [("M", 20), ("D", 2), ("I", "AC"), ("M", 20)])           # adjacent: the I sits on nothing
    read(0, [("I", "GG"), ("M", 30)])                                # leading I
    read(3, [("M", 1), ("I", "A"), ("M", 30)], qual=[30, 2, 30])
    read(0, [("M", 4), ("I", "A"), ("M", 30)], qual=[30, 30, 30, 3])  # a low-quality entry takes its marker with it
    read(0, [("M", 11), ("S", "TT"), ("I", "CG"), ("M", 25)])          # malformed, but walked: an S in front of the I (its bases are not the I's)
    read(0, [("M", 50)], flag=0x400)
    read(0, [("M", 50)], flag=0x800)
    out.sort(key=lambda r: r["pos"])
    return [("eng", n)], {"eng": ctg}, out


def make_random_bam(path, seed, n_contigs=3, n_reads=60, max_l=100):
    """A seeded random BAM (bam.write_bam): contigs rich in n-polymers, reads with soft and hard clips, both strands, flags
    of the exclude set and supplementary reads, qualities on both sides of 13, missing qualities, IUPAC letters, copy-number
    and other INDELs at polymer starts, INDELs of max_l and more, adjacent INDELs, reads on a contig's first and last base.
    Returns (references [(name, length)], refs {name: sequence})."""
    from npore_amd import bam
    rng = np.random.default_rng(seed)
    refs, references = {}, []
    for c in range(n_contigs):
        parts = []
        while sum(map(len, parts)) < 500 + 150 * c:
            u = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 5))))
            parts.append(u * int(rng.integers(3, 9)) if rng.random() < .5 else "".join(rng.choice(list("ACGT"), size=int(rng.integers(3, 12)))))
        if c == 0:
            parts.append("A" * (max_l + 20) if max_l <= 20 else "A" * 30)
        seq = "".join(parts)
        if c == 1:
            seq = seq[:200] + "N" + seq[201:]
        refs[f"c{c}"] = seq
        references.append((f"c{c}", len(seq)))
    # where the polymers start (annotation of the whole contig): half of the INDELs are put there
    starts = []
    for c in range(n_contigs):
        info = _oracle_info(refs[f"c{c}"], 6, max_l)
        starts.append({int(p): [int(m) + 1 for m in np.nonzero((info[p, 0] != 0) & (info[p, 1] == 0))[0]]
                       for p in np.nonzero(((info[:, 0] != 0) & (info[:, 1] == 0)).any(axis=1))[0]})
    records = []
    for k in range(n_reads):
        rid = int(rng.integers(0, n_contigs))
        ctg = refs[f"c{rid}"]
        clen = len(ctg)
        span = int(rng.integers(40, min(300, clen)))
        mode = k % 6
        pos = 0 if mode == 0 else clen - span if mode == 1 else int(rng.integers(0, clen - span))
        cigar, seq, r, end = [], [], pos, pos + span
        if rng.random() < .3:
            cigar.append((5, int(rng.integers(1, 9))))
        if rng.random() < .4:
            s = int(rng.integers(1, 12))
            cigar.append((4, s)); seq.append("".join(rng.choice(list("ACGT"), size=s)))
        prev = None
        while r < end:
            m = int(min(end - r, rng.integers(1, 25)))
            ahead = [p for p in range(r + 1, min(end, r + 40)) if p in starts[rid]]
            if ahead and rng.random() < .5:
                m = ahead[0] - r                             # the match ends in front of a polymer's start
            chunk = list(ctg[r:r + m])
            for i in range(m):
                u = rng.random()
                if u < .04:
                    chunk[i] = "ACGT"[int(rng.integers(0, 4))]
                elif u < .05:
                    chunk[i] = "NRYKM"[int(rng.integers(0, 5))]
            cigar.append((int(rng.choice([0, 0, 7, 8])), m)); seq.append("".join(chunk)); r += m
            prev = "M"
            if r >= end and mode != 2:
                break
            u = rng.random()
            n_indel = 2 if u < .08 else 1                    # (two in a row: an adjacent pair)
            for _ in range(n_indel):
                v, unit_n = rng.random(), int(rng.integers(1, 5))
                if r in starts[rid] and rng.random() < .8:
                    unit_n = int(rng.choice(starts[rid][r]))
                if rng.random() < .5:                        # insertion
                    if v < .5:
                        ins = ctg[r:r + unit_n] * int(rng.integers(1, 4))       # copies of what follows
                    elif v < .55:
                        ins = "".join(rng.choice(list("ACGT"), size=max_l + int(rng.integers(0, 3))))
                    else:
                        ins = "".join(rng.choice(list("ACGTN"), size=int(rng.integers(1, 7))))
                    if ins:
                        cigar.append((1, len(ins))); seq.append(ins)
                else:
                    d = unit_n * int(rng.integers(1, 4)) if v < .6 else max_l + int(rng.integers(0, 3)) if v < .65 else int(rng.integers(1, 9))
                    d = min(d, clen - r - 1)
                    if d > 0 and r + d < end + 200 and r + d < clen:
                        cigar.append((2, d)); r += d
            if r >= clen - 1:
                break
        if cigar[-1][0] in (1, 2):                           # close with a match so that the record ends on the contig
            m = min(3, clen - r)
            if m > 0:
                cigar.append((0, m)); seq.append(ctg[r:r + m]); r += m
        if rng.random() < .4:
            s = int(rng.integers(1, 12))
            cigar.append((4, s)); seq.append("".join(rng.choice(list("ACGT"), size=s)))
        if rng.random() < .3:
            cigar.append((5, int(rng.integers(1, 9))))
        seq = "".join(seq)
        fl = 16 if rng.random() < .5 else 0
        u = rng.random()
        fl |= 0x800 if u < .1 else 0x100 if u < .15 else 0x400 if u < .2 else 0x200 if u < .25 else 0x4 if u < .28 else 0
        qual = None if rng.random() < .15 else bytes(int(x) for x in rng.choice([2, 7, 12, 13, 14, 30, 40], size=len(seq)))
        records.append({"name": f"r{k}", "flag": fl, "ref_id": rid, "pos": pos, "cigar": cigar, "seq": seq, "qual": qual})
    # a few fixed reads so that no branch hangs on the dice: an insertion on a contig's last bases, a record with N
    c0 = refs["c0"]
    n0 = len(c0)
    records.append({"name": "tail_ins", "flag": 0, "ref_id": 0, "pos": n0 - 30, "cigar": [(0, 29), (1, 2), (0, 1)],
                    "seq": c0[n0 - 30:n0 - 1] + "AA" + c0[n0 - 1], "qual": bytes([40] * 32)})
    records.append({"name": "lowq_marker", "flag": 0, "ref_id": 0, "pos": 10, "cigar": [(0, 20), (2, 3), (0, 20)],
                    "seq": c0[10:30] + c0[33:53], "qual": bytes([40] * 19 + [3] + [40] * 20)})
    records.append({"name": "skip", "flag": 0, "ref_id": 0, "pos": 5, "cigar": [(0, 20), (3, 30), (0, 20)],
                    "seq": c0[5:25] + c0[55:75], "qual": None})
    records.sort(key=lambda r: (r["ref_id"], r["pos"]))
    bam.write_bam(path, references, records)
    return references, refs


def whole_contig_ranges(references, chunk_width):
    from npore_amd.bed import get_ranges
    return get_ranges([(n, 0, l) for n, l in references], chunk_width)


RANDOM_CASES = [(seed, max_l, chunk_width) for seed in (1, 2, 3) for max_l, chunk_width in ((100, 100000), (5, 61), (100, 17))]
BRANCHES = ("copy_deletion", "copy_insertion", "noncopy_indel_at_start", "indel_k_ge_max_l", "insertion_unit_clipped",
            "on_range_last_position", "lowq_with_marker")


def long_cigar_records(seed=11):
    """Reads whose CIGARs span several of the kernel's tiles of 256 operations (every real ONT read does): returns
    (references, refs, records, facts).  Built operation by operation so that, in record 0,
      * operation 255 (the last slot of the first tile) is a match whose marker, the I at 256, lies in the next tile;
      * the D at 511 and the I at 512 are an adjacent pair across a tile border (the I sits on nothing);
      * one match operation is longer than 256 positions;
    record 1 has a leading S (so the tiles are cut one operation later) and a D marker across the first border, record 2
    a leading H and S, an I at 767 | 768.  facts: per record the list of (op, len), for the tests to assert the above."""
    rng = np.random.default_rng(seed)
    parts = []
    while sum(map(len, parts)) < 9000:
        u = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 4))))
        parts.append(u * int(rng.integers(3, 8)) if rng.random() < .5 else "".join(rng.choice(list("ACGT"), size=int(rng.integers(2, 9)))))
    ctg = "".join(parts)
    references, refs = [("long", len(ctg))], {"long": ctg}
    records, facts = [], []

    def build(name, pos, lead, forced, n_ops, long_at):
        """lead: clips in front; forced: {index: (op, len)}; other operations alternate match / indel"""
        cigar, seq, r = list(lead), [], pos
        for op, n in lead:
            if op == 4:
                seq.append("".join(rng.choice(list("ACGT"), size=n)))
        while len(cigar) < n_ops:
            j = len(cigar)
            if j in forced:
                op, n = forced[j]
            elif cigar and cigar[-1][0] in M_OPS:
                op, n = (1, int(rng.integers(1, 4))) if rng.random() < .5 else (2, int(rng.integers(1, 4)))
            else:
                op, n = int(rng.choice([0, 7, 8])), (300 if j == long_at else int(rng.integers(1, 9)))
            if op in M_OPS:
                chunk = list(ctg[r:r + n])
                for i in range(n):
                    if rng.random() < .05:
                        chunk[i] = "ACGT"[int(rng.integers(0, 4))]
                seq.append("".join(chunk)); r += n
            elif op == 1:
                # half of the insertions repeat what follows (copies where a polymer starts there)
                seq.append((ctg[r:r + n] if rng.random() < .5 else "".join(rng.choice(list("ACGT"), size=n))))
            elif op == 2:
                r += n
            cigar.append((op, n))
        assert r < len(ctg)
        seq = "".join(seq)
        qual = bytes(int(x) for x in rng.choice([5, 12, 13, 20, 40], size=len(seq), p=[.05, .05, .1, .3, .5]))
        records.append({"name": name, "flag": 0, "ref_id": 0, "pos": pos, "cigar": cigar, "seq": seq, "qual": qual})
        facts.append(cigar)

    build("tiles0", 3, [], {254: (2, 2), 255: (0, 6), 256: (1, 2), 510: (7, 4), 511: (2, 3), 512: (1, 2), 513: (0, 5), 301: (0, 300), 302: (2, 1)}, 700, -1)
    build("tiles1", 40, [(4, 5)], {255: (0, 3), 256: (8, 4), 257: (2, 2), 258: (0, 4), 101: (7, 280), 102: (1, 2)}, 600, -1)
    build("tiles2", 200, [(5, 7), (4, 3)], {766: (1, 1), 767: (0, 7), 768: (1, 3), 769: (0, 2), 513: (0, 300), 514: (2, 2)}, 900, -1)
    records.sort(key=lambda r: r["pos"])
    return references, refs, records, facts
