"""Inputs shared by tests/test_long_cigar.py and tests/test_gpu_long_cigar.py: a small BAM whose records exist twice, plain
and as placeholder + CG tag (SAM specification 4.2.2), the records that look like long-CIGAR records and are none, and the
pack arrays a record must give -- written down from the rule (csrc/hostio.hpp rec_cigar), not from a run."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from npore_amd import bam

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
CONSUMES_REF = (M, D, N, 7, 8)
CONSUMES_QUERY = (M, I, S, 7, 8)
# a Z tag and a B,c array: what a tag walk has to step over
FILLER = b"XZZhello\0" + b"XBBc" + struct.pack("<I", 3) + bytes([1, 255, 3])


def random_contig(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


def small_records(seed=3):
    """(references, {contig: bases}, records): ten short reads of 3 - 9 operations -- clips of odd and even length, H
    outside S, with and without qualities and HP.  Every record names how its CG copy is written (`cg`: True = CG behind
    HP, "front" = CG first, "i" = subtype i) and carries filler tags in front of HP."""
    rng = np.random.default_rng(seed)
    contig = random_contig(rng, 4000)
    shapes = [
        [(S, 3), (M, 40), (I, 2), (M, 55), (S, 2)],                      # odd leading clip, trailing clip
        [(H, 4), (S, 5), (M, 30), (D, 3), (M, 61)],                      # H + S
        [(M, 50), (I, 1), (M, 20), (D, 2), (M, 33)],
        [(S, 1), (M, 25), (D, 1), (M, 25), (I, 3), (M, 25), (D, 4), (M, 30), (S, 7)],
        [(M, 70), (D, 5), (M, 70)],
        [(S, 2), (M, 64), (I, 4), (M, 64), (S, 1), (H, 9)],              # S + H at the end
        [(M, 20), (I, 1), (M, 20), (I, 1), (M, 20), (D, 1), (M, 90)],
        [(H, 2), (M, 100), (D, 2), (M, 100), (H, 3)],
        [(S, 9), (M, 120), (I, 5), (M, 60)],
        [(M, 33), (D, 7), (M, 44), (S, 4)],
    ]
    how = [True, "front", "i", True, "front", True, "i", True, "front", True]
    records, pos = [], 30
    for k, cigar in enumerate(shapes):
        seq, at = [], pos
        for op, ln in cigar:
            if op in (M, 7, 8):
                seg = list(contig[at:at + ln])
                for j in range(0, ln, 17):                               # a substitution now and then
                    seg[j] = "ACGT"[("ACGT".index(seg[j]) + 1) % 4]
                seq += seg
            elif op in (I, S):
                seq += list(random_contig(rng, ln))
            if op in CONSUMES_REF:
                at += ln
        seq = "".join(seq)
        records.append(dict(name=f"read{k}", flag=16 if k % 3 == 1 else 0, ref_id=0, pos=pos, mapq=20 + k, cigar=cigar, seq=seq,
                            qual=None if k == 4 else bytes(rng.integers(5, 50, len(seq)).tolist()), hp=None if k == 6 else k % 3,
                            tags=FILLER if k % 2 else b"", cg=how[k]))
        pos += 250 + 13 * k
    return [("ctg", len(contig))], {"ctg": contig}, records


def as_plain(records):
    return [{k: v for k, v in r.items() if k != "cg"} for r in records]


def as_long(records):
    return [dict({k: v for k, v in r.items() if k != "cg"}, long_cigar=r["cg"]) for r in records]


def ref_len(cigar):
    return sum(ln for op, ln in cigar if op in CONSUMES_REF)


def lookalikes(seed=4):
    """(records, [the CIGAR each must be read with]): records that begin like a long-CIGAR record and are none -- in every
    one the record's OWN CIGAR stands, which is how the code without the feature read them."""
    rng = np.random.default_rng(seed)
    real = [(M, 30), (I, 2), (M, 28)]
    words = b"".join(struct.pack("<I", ln << 4 | op) for op, ln in real)
    l_seq, rl = 60, 58
    place = [(S, l_seq), (N, rl)]

    def rec(k, cigar, tags, hp=1):
        seq = random_contig(rng, l_seq)
        return dict(name=f"not{k}", flag=0, ref_id=0, pos=100 + 200 * k, mapq=30, cigar=cigar, seq=seq,
                    qual=bytes(rng.integers(5, 50, l_seq).tolist()), hp=hp, tags=tags)
    records = [
        rec(0, place, b""),                                                           # placeholder without a tag
        rec(1, place, b"CGZ30M2I28M\0"),                                              # CG of another type
        rec(2, place, b"CGBI" + struct.pack("<I", 1) + words[:4]),                    # fewer words than n_cigar_op
        rec(3, place, FILLER + b"CGBI" + struct.pack("<I", 5) + words, hp=None),     # the array leaves the record
        rec(4, [(S, l_seq - 1), (N, rl)], b"CGBI" + struct.pack("<I", 3) + words),    # first operation shorter than l_seq
        rec(5, place, b"CGBS" + struct.pack("<I", 3) + words[:6]),                    # an array of 16-bit values
    ]
    return records, [r["cigar"] for r in records]


def expected_pack(record, cigar, contig):
    """(reference codes, query codes, expanded CIGAR) of `record` read with `cigar`: the contig under the alignment -- N where
    the alignment runs past the contig's end --, the bases without the soft clips, the operations without S and H
    ('NACGT-' -> 0..5)."""
    code = {c: i for i, c in enumerate("NACGT-")}
    lead = cigar[0][1] if cigar[0][0] == S else cigar[1][1] if len(cigar) > 1 and cigar[0][0] == H and cigar[1][0] == S else 0
    trail = 0
    if len(cigar) > 1 and cigar[-1][0] == S:
        trail = cigar[-1][1]
    if len(cigar) > 2 and cigar[-1][0] == H and cigar[-2][0] == S:
        trail = cigar[-2][1]
    seq = record["seq"]
    sl = max(0, len(seq) - lead - trail)
    refs = [code.get(c, 0) for c in contig[record["pos"]:record["pos"] + ref_len(cigar)]]
    refs += [0] * (ref_len(cigar) - len(refs))                 # zeros (N) where the slice leaves the contig (unpack)
    seqs = [code.get(c, 0) for c in seq[lead:lead + sl]]
    ops = "".join("MIDNSHP=X"[op] * ln for op, ln in cigar if op not in (S, H))
    return np.array(refs, np.uint8), np.array(seqs, np.uint8), ops.encode()


def collapsed(cigar):
    return "".join(f"{ln}{'MIDNSHP=X'[op]}" for op, ln in cigar if op not in (S, H))


def native_pack_per_read(nb, nf, idx):
    refs, ro, seqs, so, cigs, co = nb.pack(nf, idx)
    return [(refs[ro[k]:ro[k + 1]], seqs[so[k]:so[k + 1]], cigs[co[k]:co[k + 1]].tobytes()) for k in range(len(idx))]


def write_fasta(path, refs):
    with open(path, "w") as fh:
        for n, s in refs.items():
            fh.write(f">{n}\n")
            for k in range(0, len(s), 80):
                fh.write(s[k:k + 80] + "\n")
    return path


def ultra_long_read(seed=1, units=36000):
    """One read of `5=1D` x units on a random contig (every sixth reference base lost; 2 * units operations on the way in)
    between two ordinary 2 kb reads: (references, refs, records)."""
    rng = np.random.default_rng(seed)
    n_ref = 6 * units
    contig = random_contig(rng, n_ref + 400)
    arr = np.frombuffer(contig.encode(), np.uint8)
    body = arr[100:100 + n_ref].reshape(units, 6)[:, :5].reshape(-1).tobytes().decode()
    quals = bytes(rng.integers(10, 40, len(body)).astype(np.uint8))
    short = lambda name, pos: dict(name=name, flag=0, ref_id=0, pos=pos, mapq=60, cigar=[(M, 1000), (I, 1), (M, 999)],
                                   seq=contig[pos:pos + 1000] + "A" + contig[pos + 1000:pos + 1999],
                                   qual=bytes(rng.integers(10, 40, 2000).astype(np.uint8)), hp=1)
    records = [short("before", 40),
               dict(name="ultra", flag=0, ref_id=0, pos=100, mapq=60, cigar=[(7, 5), (D, 1)] * units, seq=body, qual=quals, hp=2),
               short("after", n_ref - 3000)]
    return [("big", len(contig))], {"big": contig}, records


def _model_lib(name, extra_deps=()):
    """tests/model/<name>.cpp built lazily with g++, like the other host twins"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "model")
    csrc = os.path.join(here, "..", "..", "npore_amd", "csrc")
    so, src = os.path.join(here, f"lib{name}.so"), os.path.join(here, f"{name}.cpp")
    deps = [src] + [os.path.join(csrc, f) for f in ("bam_reader.hpp", "hostio.hpp", "inflate.hpp", "crc32.hpp", "glue.hpp") + tuple(extra_deps)]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", so, src, "-lz", "-lpthread"])
    return C.CDLL(so)


def stage_twin():
    """tests/model/stage_twin.cpp: stage_twin_compare"""
    lib = _model_lib("stage_twin", ("staged_head.hpp",))
    lib.stage_twin_compare.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64]
    lib.stage_twin_compare.restype = C.c_int64
    return lib


def _twins():
    lib = _model_lib("long_cigar_twins", ("confusion_rec.hpp", "purity_rec.hpp", "std_stream.hpp"))
    lib.cms_cg_twin_count.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 5 + \
        [C.c_int, C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 5
    lib.cms_cg_twin_count.restype = C.c_int
    lib.pur_cg_twin.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 3 + \
        [C.c_int64, C.c_void_p]
    lib.pur_cg_twin.restype = C.c_int
    lib.long_cigar_twins_last_error.restype = C.c_char_p
    return lib


def twin_count(bam_path, references, refs, ranges, max_n, max_l, min_bq=13, exclude_flags=0x704):
    """cms_model.twin_count through tests/model/long_cigar_twins.cpp (every record read with its real CIGAR): (subs, nps,
    inss, dels, tallies dict).  references: the BAM header's names; refs: {contig: sequence}; ranges: [(contig, start, stop)]."""
    from model import cms_model
    lib = _twins()
    ids = {n: i for i, n in enumerate(references)}
    text = "".join(refs.get(n, "") for n in references).encode()
    off = np.zeros(len(references) + 1, np.int64)
    np.cumsum([len(refs.get(n, "")) for n in references], out=off[1:])
    planes, ann, at = [], [], 0
    for c, st, en in ranges:
        st, en = max(0, st), min(en, len(refs[c]))
        ann.append(at)
        if st < en:
            pl = cms_model.planes_of(cms_model._oracle_info(refs[c][st:en + 1], max_n, max_l))
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
    rc = lib.cms_cg_twin_count(os.fsencode(bam_path), text, off.ctypes.data, len(references), len(ranges), rid.ctypes.data, beg.ctypes.data,
                               end.ctypes.data, ann.ctypes.data, planes.ctypes.data, max_n, max_l, min_bq, exclude_flags,
                               subs.ctypes.data, nps.ctypes.data, inss.ctypes.data, dels.ctypes.data, tallies.ctypes.data)
    if rc:
        raise RuntimeError(f"{rc}: {lib.long_cigar_twins_last_error().decode()}")
    return subs, nps, inss, dels, dict(zip(cms_model.TALLY_NAMES, tallies.tolist()))


def purity_twin(bam_path, references, ranges, n_positions, min_bq=13, exclude_flags=0x704):
    """purity_model.twin through tests/model/long_cigar_twins.cpp: (rows, base_hist, ins_hist, tallies dict)"""
    from model import purity_model
    lib = _twins()
    ids = {n: i for i, n in enumerate(references)}
    rid = np.array([ids.get(c, -1) for c, _, _ in ranges], np.int32)
    beg = np.array([s for _, s, _ in ranges], np.int64)
    end = np.array([e for _, _, e in ranges], np.int64)
    hb, hi, tallies = np.zeros(100, np.int64), np.zeros(100, np.int64), np.zeros(16, np.int64)
    rows = np.zeros((n_positions, 4), np.int64)
    rc = lib.pur_cg_twin(os.fsencode(bam_path), len(ranges), rid.ctypes.data, beg.ctypes.data, end.ctypes.data, min_bq, exclude_flags,
                         hb.ctypes.data, hi.ctypes.data, rows.ctypes.data, n_positions, tallies.ctypes.data)
    if rc:
        raise RuntimeError(f"{rc}: {lib.long_cigar_twins_last_error().decode()}")
    return rows, hb, hi, dict(zip(purity_model.TALLY_NAMES, tallies.tolist()))
