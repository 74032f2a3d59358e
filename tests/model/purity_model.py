"""TEST INFRASTRUCTURE for the Gini purity of pileups from BAM records (npore_amd/csrc/purity_rec.hpp).

Independent statements of the same thing meet here:
  * compute_purity(): a Python model of the reference's function (src/purity.py:11-84), pinned to the reference's own
    floats by tests/golden/purity.json;
  * write_columns(): the rule of purity_rec.hpp as a pileup writer -- records -> one mpileup column-5 string per merged
    position, with `^` + mapping quality, `$`, lower case on the reverse strand, `*`, +k / -k markers;
  * expected(): those columns, upper-cased as the reference does, through compute_purity and the reference's FLOAT
    binning int(x * 100 - 0.00001), plus the per-position integers counted from the column text;
  * twin(): purity_rec.hpp itself compiled by g++ (tests/model/purity_rec.cpp), built lazily like cms_model's."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
TALLY_NAMES = ("records", "records_flagged", "records_refskip", "records_malformed", "insertions_without_entry",
               "entries_ambiguous", "entries_lowq", "entries_counted", "star_entries", "insertions_counted",
               "insertions_hashed", "positions_covered", "positions_too_deep")
M_OPS = (0, 7, 8)


def compute_purity(col):
    """the reference's compute_purity on a str: (bases score, insertions score) or None"""
    bases, inss = collections.defaultdict(int), collections.defaultdict(int)
    i = 0
    while i < len(col):
        c = col[i]
        if c == "^":
            i += 2
        elif c == "$":
            i += 1
        elif c in "ACGT*":
            bases[c] += 1
            i += 1
        elif c in "-+":
            i += 1
            k = 0
            while col[i] in "0123456789":
                k = 10 * k + int(col[i])
                i += 1
            if c == "+":
                inss[col[i:i + k]] += 1
            i += k
        else:
            break
    n = sum(bases.values())
    if not n:
        return None
    bases_score = 0
    for b in "ACGT*":
        bases_score += (bases[b] / n) ** 2
    not_inss = n - sum(inss.values())
    inss_score = (not_inss / n) ** 2
    for v in inss.values():
        inss_score += (v / n) ** 2
    return bases_score, inss_score


def column_integers(col):
    """(n, S_b, t, S_i) of an upper-cased column, counted from its text"""
    col = re.sub(r"\^.", "", col).replace("$", "")
    inss = collections.Counter()
    out, i = [], 0
    while i < len(col):
        c = col[i]
        if c in "+-":
            m = re.match(r"\d+", col[i + 1:])
            k, i = int(m.group()), i + 1 + len(m.group())
            if c == "+":
                inss[col[i:i + k]] += 1
            i += k
        else:
            out.append(c)
            i += 1
    assert set(out) <= set("ACGT*"), col
    cnt = collections.Counter(out)
    n, t = len(out), sum(inss.values())
    return n, sum(v * v for v in cnt.values()), t, (n - t) ** 2 + sum(v * v for v in inss.values())


def merge_ranges(ranges, lengths, order):
    """[(contig, start, stop)] of the merged, clipped ranges: contigs in header order, ascending, disjoint"""
    out = []
    for c in order:
        iv = sorted((max(0, s), min(e, lengths[c])) for cc, s, e in ranges if cc == c)
        cur = None
        for s, e in iv:
            if s >= e:
                continue
            if cur and s <= cur[2]:
                cur[2] = max(cur[2], e)
            else:
                cur = [c, s, e]
                out.append(cur)
    return [tuple(x) for x in out]


def write_columns(records, references, lengths, ranges, min_bq=13, exclude_flags=0x704):
    """The rule of purity_rec.hpp as a pileup writer.  records: bam.BamFile(...).records.  Returns (columns, tallies):
    columns = one mpileup column-5 string per merged position (contigs in header order), NOT upper-cased."""
    tallies = collections.Counter({k: 0 for k in TALLY_NAMES})
    size = dict(zip(references, lengths))
    merged = merge_ranges(ranges, size, references)
    dense, total = {}, 0                           # contig -> [(st, en, dense offset)]
    for c, s, e in merged:
        dense.setdefault(c, []).append((s, e, total))
        total += e - s
    cols = [[] for _ in range(total)]

    def where(ctg, a):
        for s, e, off in dense.get(ctg, ()):
            if s <= a < e:
                return off + a - s
        return None

    for rec in records:
        if rec.ref_id < 0 or rec.ref_id >= len(references):
            continue
        ctg = references[rec.ref_id]
        pos = rec.reference_start
        rl = sum(n for op, n in rec.cigar if op in (0, 2, 3, 7, 8))
        ql = sum(n for op, n in rec.cigar if op in (0, 1, 4, 7, 8))
        if pos < 0 or rl <= 0 or not any(pos < e and pos + rl > s for s, e, _ in dense.get(ctg, ())):
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
        rev = bool(rec.flag & 16)
        case = (lambda x: x.lower()) if rev else (lambda x: x)
        mapq = chr(33 + min(rec.mapping_quality, 93))
        vis, r, q = [], pos, 0                     # the operations one sees: S, H and empty ones stepped over
        for op, n in rec.cigar:
            if n > 0 and op not in (4, 5):
                vis.append((op, n, r, q))
            r += n if op in (0, 2, 3, 7, 8) else 0
            q += n if op in (0, 1, 4, 7, 8) else 0
        entries = []                               # (position, text) of the entries that are counted
        for k, (op, n, r0, q0) in enumerate(vis):
            if op == 1 and (k == 0 or vis[k - 1][0] not in M_OPS):
                tallies["insertions_without_entry"] += 1
            if op == 2:
                qv = rec.qual[q0 - 1] if q0 > 0 else 0xFF
                for t in range(n):
                    at = where(ctg, r0 + t)
                    if at is None:
                        continue
                    if qv != 0xFF and qv < min_bq:
                        tallies["entries_lowq"] += 1
                        continue
                    tallies["entries_counted"] += 1
                    tallies["star_entries"] += 1
                    entries.append((at, "*"))
            if op not in M_OPS:
                continue
            for t in range(n):
                at = where(ctg, r0 + t)
                if at is None:
                    continue
                b, qv = rec.seq[q0 + t], rec.qual[q0 + t]
                if qv != 0xFF and qv < min_bq:
                    tallies["entries_lowq"] += 1
                    continue
                if b not in "ACGT":
                    tallies["entries_ambiguous"] += 1
                    continue
                tallies["entries_counted"] += 1
                text = case(b)
                if t == n - 1 and k + 1 < len(vis) and vis[k + 1][0] in (1, 2):
                    nop, kk, _, nq = vis[k + 1]
                    if nop == 1:
                        text += f"+{kk}{case(rec.seq[nq:nq + kk])}"
                        tallies["insertions_counted"] += 1
                        tallies["insertions_hashed"] += kk > 14
                    else:
                        text += f"-{kk}{case('N' * kk)}"
                entries.append((at, text))
        for i, (at, text) in enumerate(entries):   # `^` and `$` on the read's first and last entry that is written
            if i == 0:
                text = "^" + mapq + text
            if i == len(entries) - 1:
                text += "$"
            cols[at].append(text)
    columns = ["".join(c) for c in cols]
    tallies["positions_covered"] = sum(1 for c in columns if c)
    return columns, tallies


def float_bin(x):
    return int(x * 100 - 0.00001)


def expected(bam_path, ranges, min_bq=13, exclude_flags=0x704):
    """(rows int64 [P, 4], base_hist, ins_hist, scores float64 [covered, 2], tallies) from the writer's columns: the
    histograms by the reference's float expression, the rows from the text"""
    from npore_amd import bam
    f = bam.BamFile(bam_path)
    return expected_of(f.records, f.references, f.lengths, ranges, min_bq, exclude_flags)


def expected_of(records, references, lengths, ranges, min_bq=13, exclude_flags=0x704):
    columns, tallies = write_columns(records, references, lengths, ranges, min_bq, exclude_flags)
    rows = np.zeros((len(columns), 4), np.int64)
    hb, hi, scores = np.zeros(100, np.int64), np.zeros(100, np.int64), []
    for k, col in enumerate(columns):
        col = col.upper()
        res = compute_purity(col)
        if res is None:
            assert not col
            continue
        rows[k] = column_integers(col)
        hb[float_bin(res[0])] += 1
        hi[float_bin(res[1])] += 1
        scores.append(res)
    return rows, hb, hi, np.array(scores, np.float64).reshape(-1, 2), tallies


def range_sets(references):
    """whole contigs; pieces of 17 and 61; overlapping and unsorted ranges; a range that leaves the contig"""
    whole = [(n, 0, l) for n, l in references]
    pieces = lambda w: [(n, s, min(s + w, l)) for n, l in references for s in range(0, l, w)]
    n0, l0 = references[0]
    odd = [(n0, l0 // 2, l0 + 50), (n0, 5, 40), (n0, 20, 60), (n0, 0, 7), (n0, l0, l0 + 5), (references[-1][0], -10, 33)]
    return [whole, pieces(17), pieces(61), odd]


def build(force=False):
    so = os.path.join(_HERE, "libpurity_rec.so")
    csrc = os.path.join(_HERE, "..", "..", "npore_amd", "csrc")
    deps = [os.path.join(_HERE, "purity_rec.cpp")] + [
        os.path.join(csrc, f) for f in ("purity_rec.hpp", "confusion_rec.hpp", "bam_reader.hpp", "hostio.hpp", "inflate.hpp", "crc32.hpp",
                                        "glue.hpp", "std_stream.hpp")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", so, deps[0], "-lz", "-lpthread"])
    return so


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(build())
        lib.pur_twin.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 3 + \
            [C.c_int64, C.c_void_p]
        lib.pur_twin.restype = C.c_int
        lib.pur_twin_last_error.restype = C.c_char_p
        lib.pur_twin_key.argtypes = [C.c_void_p, C.c_int64, C.c_uint32]
        lib.pur_twin_key.restype = C.c_uint64
        lib.pur_twin_bin.argtypes = [C.c_uint64, C.c_uint64]
        lib.pur_twin_bin.restype = C.c_int
        _LIB = lib
    return _LIB


def twin(bam_path, references, ranges, n_positions, min_bq=13, exclude_flags=0x704):
    """purity_rec.hpp on the host: (rows, base_hist, ins_hist, tallies dict)"""
    lib = load()
    ids = {n: i for i, n in enumerate(references)}
    rid = np.array([ids.get(c, -1) for c, _, _ in ranges], np.int32)
    beg = np.array([s for _, s, _ in ranges], np.int64)
    end = np.array([e for _, _, e in ranges], np.int64)
    hb, hi, tallies = np.zeros(100, np.int64), np.zeros(100, np.int64), np.zeros(16, np.int64)
    rows = np.zeros((n_positions, 4), np.int64)
    rc = lib.pur_twin(os.fsencode(bam_path), len(ranges), rid.ctypes.data, beg.ctypes.data, end.ctypes.data, min_bq, exclude_flags,
                      hb.ctypes.data, hi.ctypes.data, rows.ctypes.data, n_positions, tallies.ctypes.data)
    if rc:
        raise RuntimeError(f"{rc}: {lib.pur_twin_last_error().decode()}")
    return rows, hb, hi, dict(zip(TALLY_NAMES, tallies.tolist()))


_CODE = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}


def key_of(s):
    """pur_key of the letters s (BAM's 4-bit codes), through the twin"""
    nib = [_CODE[c] for c in s] + [0]
    packed = np.array([(nib[i] << 4) | nib[i + 1] for i in range(0, len(nib) - 1, 2)] + [0], np.uint8)
    return int(load().pur_twin_key(packed.ctypes.data, 0, len(s)))


def tallies_agree(got, want):
    return all(int(got[k]) == int(want[k]) for k in TALLY_NAMES)


def window_records(seed=5):
    """Reads for the window tests on one contig of 400 bases with purity_window = 64: a record spanning three windows, an
    insertion on a window's last position (63 | 64), a deletion across a window border (126..130), many reads inserting at
    one position.  Returns (references, records)."""
    rng = np.random.default_rng(seed)
    ctg = "".join(rng.choice(list("ACGT"), size=400))
    out = []

    def read(pos, parts, flag=0, q=30):
        cigar, seq, r = [], "", pos
        for kind, v in parts:
            if kind == "M":
                cigar.append((0, v)); seq += ctg[r:r + v]; r += v
            elif kind == "I":
                cigar.append((1, len(v))); seq += v
            elif kind == "D":
                cigar.append((2, v)); r += v
        out.append({"name": f"w{len(out)}", "flag": flag, "ref_id": 0, "pos": pos, "cigar": cigar, "seq": seq, "qual": bytes([q] * len(seq))})

    read(10, [("M", 200)])                                           # windows 0..3
    read(20, [("M", 44), ("I", "AC"), ("M", 100)])                   # the entry at 63 carries the insertion
    read(20, [("M", 44), ("I", "AC"), ("M", 10)], flag=16)
    read(30, [("M", 34), ("I", "ACG"), ("M", 60)])
    read(100, [("M", 26), ("D", 5), ("M", 80)])                      # deleted 126..130 over the border 127 | 128
    read(100, [("M", 26), ("D", 5), ("M", 80)], q=5)                 # ... dropped whole by quality
    read(120, [("M", 8), ("D", 70), ("M", 30)])                      # a deletion that covers a whole window
    read(190, [("M", 2), ("I", "T" * 20), ("M", 200)])
    read(300, [("M", 100)])
    out.sort(key=lambda r: r["pos"])
    return [("win", 400)], out


def deep_insertion_records(n_reads):
    """n_reads reads inserting at ONE position (49) and a fifth as many that do not: three distinct short strings and two of
    length 20 that differ in their last letter -- buckets larger than a wave."""
    rng = np.random.default_rng(n_reads)
    ctg = "".join(rng.choice(list("ACGT"), size=120))
    kinds = ["A", "AC", "TTT", "ACGTACGTACGTACGTACGA", "ACGTACGTACGTACGTACGC"]
    out = []
    for k in range(n_reads + n_reads // 5):
        ins = kinds[k % 5] if k < n_reads else None
        pos = int(rng.integers(0, 30))
        if ins is None:
            cigar, seq = [(0, 100 - pos)], ctg[pos:100]
        else:
            cigar, seq = [(0, 50 - pos), (1, len(ins)), (0, 40)], ctg[pos:50] + ins + ctg[50:90]
        out.append({"name": f"d{k}", "flag": 16 if k % 2 else 0, "ref_id": 0, "pos": pos, "cigar": cigar, "seq": seq,
                    "qual": bytes([30] * len(seq))})
    out.sort(key=lambda r: r["pos"])
    return [("deep", 120)], out
