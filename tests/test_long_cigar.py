"""Long CIGARs (SAM specification 4.2.2: more than 65 535 operations do not fit n_cigar_op; the record carries the
placeholder `<l_seq>S<reflen>N` and its real CIGAR in the tag CG:B,I), host side: the rule that resolves the tag on the
way in (csrc/hostio.hpp rec_cigar, bam.resolve_long_cigar) and the record the writers make on the way out
(csrc/bam_reader.hpp bam_record_into, bam.bam_record).  No GPU here: the final CIGARs are given."""
import struct

import numpy as np
import pytest

from model import cms_model, purity_model
from npore_amd import bam
from test_bam_out import Hdr, check_index, header_len, members, split_records
import long_cigar_cases as lc


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("long_cigar_small")
    references, refs, records = lc.small_records()
    plain, cg = str(tmp / "plain.bam"), str(tmp / "cg.bam")
    bam.write_bam(plain, references, lc.as_plain(records))
    bam.write_bam(cg, references, lc.as_long(records))
    fa = lc.write_fasta(str(tmp / "ref.fa"), refs)
    return dict(tmp=tmp, references=references, refs=refs, records=records, plain=plain, cg=cg, fa=fa)


def raw_records(path):
    data = bam._bgzf_decompress(path)
    return [r for _, r in split_records(data[header_len(data):])]


def test_cg_copy_is_written_as_placeholder_and_tag(small):
    """the test's own premise: the CG copy's records carry two placeholder words and the tag where the case says"""
    for rec, raw in zip(small["records"], raw_records(small["cg"])):
        l_rn, n_cig = raw[12], struct.unpack_from("<H", raw, 16)[0]
        l_seq, = struct.unpack_from("<i", raw, 20)
        assert n_cig == 2 and 3 <= len(rec["cigar"]) <= 9
        assert struct.unpack_from("<II", raw, 36 + l_rn) == (l_seq << 4 | 4, lc.ref_len(rec["cigar"]) << 4 | 3)
        aux = raw[36 + l_rn + 8 + (l_seq + 1) // 2 + l_seq:]
        sub = b"i" if rec["cg"] == "i" else b"I"
        tag = b"CGB" + sub + struct.pack("<I", len(rec["cigar"]))
        words = b"".join(struct.pack("<I", ln << 4 | op) for op, ln in rec["cigar"])
        hp = b"" if rec["hp"] is None else b"HPC" + bytes([rec["hp"]])
        assert aux == (tag + words + rec["tags"] + hp if rec["cg"] == "front" else rec["tags"] + hp + tag + words)
    for raw, rec in zip(raw_records(small["plain"]), small["records"]):
        assert struct.unpack_from("<H", raw, 16)[0] == len(rec["cigar"])


def test_python_and_native_reader_resolve_the_tag(small):
    contig = small["refs"]["ctg"]
    fp, fc = bam.BamFile(small["plain"]), bam.BamFile(small["cg"])
    assert len(fp.records) == len(fc.records) == len(small["records"])
    for rec, a, b in zip(small["records"], fp.records, fc.records):
        for field in bam.BamRecord.__slots__:
            assert getattr(a, field) == getattr(b, field), (rec["name"], field)
        assert b.cigar == rec["cigar"] and b.seq == rec["seq"] and b.hp == rec["hp"]
    nf = bam.NativeFasta(small["fa"])
    packs, sams = [], []
    finals = [lc.collapsed(r["cigar"]) for r in small["records"]]
    for path in (small["plain"], small["cg"]):
        nb = bam.NativeBam(path)
        idx = nb.select([("ctg", 0, len(contig))])
        assert len(idx) == len(small["records"])
        packs.append(lc.native_pack_per_read(nb, nf, idx))
        sams.append(nb.format_sam(idx, finals, np.zeros(len(idx), np.int32)))
        nb.close()
    nf.close()
    for rec, p, c in zip(small["records"], *packs):
        want = lc.expected_pack(rec, rec["cigar"], contig)
        for got in (p, c):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], rec["name"]
    assert sams[0] == sams[1] and sams[0].count("\n") == len(small["records"])
    for rec, line in zip(small["records"], sams[0].splitlines()):
        f = line.split("\t")
        clip = lc.expected_pack(rec, rec["cigar"], contig)[1]
        assert f[0] == rec["name"] and int(f[8]) == lc.ref_len(rec["cigar"]) and len(f[9]) == len(clip)


def test_lookalikes_keep_their_own_cigar(small, tmp_path):
    contig = small["refs"]["ctg"]
    records, cigars = lc.lookalikes()
    path = str(tmp_path / "not.bam")
    bam.write_bam(path, small["references"], records)
    for r, own in zip(bam.BamFile(path).records, cigars):
        assert r.cigar == own, r.query_name
    nb, nf = bam.NativeBam(path), bam.NativeFasta(small["fa"])
    idx = nb.select([("ctg", 0, len(contig))])
    assert len(idx) == len(records)
    for rec, own, got in zip(records, cigars, lc.native_pack_per_read(nb, nf, idx)):
        want = lc.expected_pack(rec, own, contig)
        assert len(want[1]) in (0, 1) and want[2] == b"N" * 58                 # a clipped read over a skip, as ever
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], rec["name"]
    nb.close(); nf.close()


def test_staged_heads_of_both_copies_agree(small, tmp_path):
    """What the kernels are handed (csrc/hostio.hpp stage_record_head) is the same for a record and its CG copy from the
    fixed fields on, and the one reader of a staged head gives the real CIGAR and the bases behind it."""
    lib = lc.stage_twin()
    n = len(small["records"])
    ops = np.zeros(n, np.int64)
    assert lib.stage_twin_compare(small["plain"].encode(), small["cg"].encode(), ops.ctypes.data, n) == n
    assert ops.tolist() == [len(r["cigar"]) for r in small["records"]]
    # more than 65 535 operations: the count's high half (a 70 001-operation record against itself)
    big = str(tmp_path / "big.bam")
    rng = np.random.default_rng(2)
    cigar = [(lc.M, 1), (lc.I, 1)] * 35000 + [(lc.M, 1)]
    bam.write_bam(big, [("ctg", 80000)], [dict(name="big", flag=0, ref_id=0, pos=5, mapq=1, cigar=cigar, seq=lc.random_contig(rng, 70001),
                                                 qual=None, hp=3)], level=1)
    one = np.zeros(1, np.int64)
    assert lib.stage_twin_compare(big.encode(), big.encode(), one.ctypes.data, 1) == 1 and one[0] == 70001


# ---- the output boundary ---------------------------------------------------------------------------------------------------
N_OPS = (65535, 65536, 70001)


@pytest.fixture(scope="module")
def boundary(tmp_path_factory):
    """three reads of n bases under `<(n + 1) / 2>M<n / 2>I`, their final CIGARs `1M1I1M1I...` of n operations (the same
    reference length: the index entries come from the input's)"""
    tmp = tmp_path_factory.mktemp("long_cigar_boundary")
    rng = np.random.default_rng(9)
    contig = lc.random_contig(rng, 80000)
    records, finals, rds = [], [], []
    for k, n in enumerate(N_OPS):
        pos = 100 + 50 * k
        seq = lc.random_contig(rng, n)
        qual = bytes(rng.integers(3, 45, n).astype(np.uint8))
        records.append(dict(name=f"b{n}", flag=0, ref_id=0, pos=pos, mapq=50, cigar=[(lc.M, (n + 1) // 2), (lc.I, n // 2)], seq=seq, qual=qual, hp=(None, 1, 200)[k]))
        finals.append(("1M1I" * (n // 2 + 1))[:2 * n])
        rds.append((f"b{n}", 0, "ctg", pos, 50, f"{(n + 1) // 2}M{n // 2}I", pos + (n + 1) // 2, seq, "".join(chr(33 + q) for q in qual), "", (0, 1, 200)[k]))
    path = str(tmp / "in.bam")
    bam.write_bam(path, [("ctg", len(contig))], records)
    return dict(tmp=tmp, path=path, finals=finals, rds=rds, records=records, clen=len(contig))


def test_output_boundary(boundary):
    nb = bam.NativeBam(boundary["path"])
    idx = nb.select([("ctg", 0, boundary["clen"])])
    st = np.zeros(3, np.int32)
    assert len(idx) == 3
    stream = nb.format_bam(idx, boundary["finals"], st)
    recs = [r for _, r in split_records(stream)]
    for n, rec, rd, final in zip(N_OPS, recs, boundary["rds"], boundary["finals"]):
        assert rec == bam.bam_record(rd, final, ["ctg"]), n
        l_rn, n_cig = rec[12], struct.unpack_from("<H", rec, 16)[0]
        words = np.array([(1 << 4) | (k & 1) for k in range(n)], "<u4").tobytes()
        hb = 1
        if n <= 0xFFFF:
            assert n_cig == n and rec[36 + l_rn:36 + l_rn + 4 * n] == words
            assert len(rec) == 36 + l_rn + 4 * n + (n + 1) // 2 + n + 3 + hb
        else:
            assert n_cig == 2 and struct.unpack_from("<II", rec, 36 + l_rn) == (n << 4 | 4, (n + 1) // 2 << 4 | 3)
            assert len(rec) == 36 + l_rn + 8 + (n + 1) // 2 + n + 3 + hb + 8 + 4 * n
            aux = rec[36 + l_rn + 8 + (n + 1) // 2 + n:]
            assert aux[:2] == b"HP" and aux[3 + hb:] == b"CGBI" + struct.pack("<I", n) + words
    # the file, its index, and back in
    out = str(boundary["tmp"] / "out.bam")
    bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
    info = nb.write_file(idx, boundary["finals"], st, out, batch_reads=2, bai=out + ".bai")
    nb.close()
    assert info["records"] == 3 and info["indexed"] == 1
    data = bam._bgzf_decompress(out)
    assert data[header_len(data):] == stream
    assert len(members(out)) > 6                                   # every record spans several members
    check_index(out, out + ".bai")
    back = bam.BamFile(out).records
    for n, r in zip(N_OPS, back):
        assert r.cigar == [(k & 1, 1) for k in range(n)] and len(r.seq) == n
    # ... and through the native reader: the written file packs as its CIGARs say
    nb2 = bam.NativeBam(out)
    idx2 = nb2.select([("ctg", 0, boundary["clen"])])
    ro, so, co = (np.zeros(4, np.int64) for _ in range(3))
    nb2._check(nb2._lib.npore_bam_pack_sizes(nb2.handle, idx2.ctypes.data, 3, ro.ctypes.data, so.ctypes.data, co.ctypes.data))
    nb2.close()
    assert np.diff(ro).tolist() == [(n + 1) // 2 for n in N_OPS] and np.diff(so).tolist() == list(N_OPS) == np.diff(co).tolist()


# ---- recount and purity: the host twins ----------------------------------------------------------------------------------
def test_recount_and_purity_twins_see_the_same_records(small):
    """tests/model/long_cigar_twins.cpp reads every record with its real CIGAR: on the plain copy it gives what the older
    twins give (which read the record's own words), and the same on the CG copy"""
    references, refs = small["references"], small["refs"]
    names = [n for n, _ in references]
    ranges = [("ctg", 0, references[0][1]), ("ctg", 100, 900)]
    old = cms_model.twin_count(small["plain"], names, refs, ranges, 6, 100)
    a = lc.twin_count(small["plain"], names, refs, ranges, 6, 100)
    b = lc.twin_count(small["cg"], names, refs, ranges, 6, 100)
    assert cms_model.same(a[:4], old[:4]) and a[4] == old[4]
    assert cms_model.same(a[:4], b[:4]) and a[4] == b[4]
    assert b[4]["records_refskip"] == 0 and b[4]["records_malformed"] == 0 and b[4]["entries_counted"] > 0
    assert cms_model.twin_count(small["cg"], names, refs, ranges, 6, 100)[4]["records_refskip"] > 0      # (the older twin: placeholders)
    ranges = [("ctg", 0, references[0][1])]
    pold = purity_model.twin(small["plain"], names, ranges, references[0][1])
    pa = lc.purity_twin(small["plain"], names, ranges, references[0][1])
    pb = lc.purity_twin(small["cg"], names, ranges, references[0][1])
    for x, y, z in zip(pa[:3], pb[:3], pold[:3]):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert pa[3] == pb[3] == pold[3] and pb[3]["records_refskip"] == 0 and pb[3]["records"] == len(small["records"])
    # ... and what the Python statement of the rule expects, which reads the file through BamFile
    want = purity_model.expected(small["cg"], ranges)
    assert np.array_equal(pb[0], want[0]) and purity_model.tallies_agree(pb[3], want[4])
