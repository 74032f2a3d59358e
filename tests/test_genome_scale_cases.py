"""The inputs of tests/genome_scale_cases.py on the CPU: that they cross what they claim -- every level of the bin scheme,
every placement at every border, contigs in two orders, mates of every form, reads past a contig's end -- and that the host
side (npore_bam_pack, npore_bam_format_bam, npore_bam_format_bam_full, npore_bam_write_file) equals the Python statements
on them.  No GPU: the final CIGARs are given (bam_full_cases.simple_final)."""
import argparse
import struct

import numpy as np
import pytest

from npore_amd import bam, cfg
from test_bam_out import check_index, spec_reg2bin, split_records, write_native
import bam_full_cases as fc
import genome_scale_cases as gs
import long_cigar_cases as lc


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("genome")
    bp, dp, fa = gs.write_inputs(tmp)
    references, refs, records, decoy = gs.case()
    finals = []
    for k, rec in enumerate(records):
        rc, sc, _ = lc.expected_pack(rec, rec["cigar"], refs[references[rec["ref_id"]][0]])
        finals.append(fc.simple_final(len(rc), len(sc), k))
    status = np.array([32 if r["_bad"] else 0 for r in records], np.int32)
    return tmp, bp, dp, fa, finals, status


def open_pair(bp, fa):
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    return nb, nf, nb.select(gs.whole_regions())


def index_conditions(bai):
    """what the index of the fixture must hold, whoever wrote the file: references 0, 1 and 3 have bins, the decoy has none;
    chrBig's linear index reaches its last 16 kb window"""
    assert [bool(bins) for bins, _ in bai] == [True, True, False, True]
    assert len(bai[1][1]) == 4097 == ((gs.BIG_LEN - 1) >> 14) + 1 and not bai[2][1]
    assert {0, 1, 9, 73, 585, 4681 + 4096} <= set(bai[1][0])


def test_inputs_cross_what_they_claim(files):
    tmp, bp, dp, fa, finals, status = files
    references, refs, records, decoy = gs.case()
    nb, nf, idx = open_pair(bp, fa)
    assert nb.fasta_map(nf).tolist() == gs.FASTA_MAP == [2, 1, -1, 0]
    assert nb.references == [n for n, _ in references] and nf.names == gs.FASTA_ORDER and "decoy" not in nf
    assert idx.tolist() == list(range(len(records))) == gs.overlapping(records, gs.whole_regions())
    nb.close(); nf.close()
    big = refs[gs.BIG]
    assert len(big) == gs.BIG_LEN and big[0] == "N" and big[(1 << 25)] == "N" and set(big[-gs.HALF:]) <= set("ACGT")
    bins = {spec_reg2bin(r["pos"], r["pos"] + gs.ref_len(r)) for r in records if r["ref_id"] == 1}
    # (the contig ends 8 192 bases behind 2^26: 4681 + 4096 is its last bin -- every bin from 4681 + 4096 on that it has)
    assert {0, 1, 9, 73, 585} <= bins and {4681 + 4095, 4681 + 4096} <= bins and max(bins) == 4681 + ((gs.BIG_LEN - 1) >> 14)
    for b in gs.BORDERS:
        for which in gs.PLACEMENTS:
            r, = [r for r in records if r["_place"] == (b, which)]
            start, stop = r["pos"], r["pos"] + gs.ref_len(r)
            assert 100 <= stop - start <= 300 and (start, stop) == gs.placement(b, which, stop - start)
            crosses = start < b < stop
            assert crosses == (which in "acd") and (which != "b" or stop == b) and (which != "c" or stop == b + 1)
            assert (which != "d" or start == b - 1) and (which != "e" or start == b) and (which != "f" or start == b + 7)
    # mates: none, same contig, another contig, unmapped; next_pos beyond 2^26; every clip shape, both strands, no qualities
    mates = {(r.get("next_ref_id", -1) == r["ref_id"], r.get("next_ref_id", -1) < 0, "next_pos" in r) for r in records}
    assert mates == {(False, True, False), (True, False, True), (False, False, True), (False, True, True)}
    assert any(r["ref_id"] == 1 and r.get("next_ref_id") == 3 for r in records)
    assert sum(r.get("next_pos", -1) > 1 << 26 for r in records) >= 3 and any(r.get("tlen", 0) < 0 for r in records)
    assert {r["flag"] for r in records} == {0, 16} and any(r["qual"] is None for r in records)
    assert {tuple(op for op, _ in r["cigar"][:2] if op in (4, 5)) for r in records} >= {(), (4,), (5, 4), (5,)}
    assert len({r["_hp"] for r in records}) == 7
    # batches of 5: the first holds alpha and chrBig, the last chrBig and zeta
    rid = [r["ref_id"] for r in records]
    assert rid == sorted(rid) and set(rid[:gs.BATCH]) == {0, 1} and set(rid[(len(rid) - 1) // gs.BATCH * gs.BATCH:]) == {1, 3}
    over = [(r["ref_id"], r["_over"]) for r in records if r["_over"]]
    assert over == [(0, 30), (1, 25)] and sum(r["_bad"] for r in records) == 1
    bad, = [r for r in records if r["_bad"]]
    assert bad["ref_id"] == 1 and 1 << 20 < bad["pos"] < 1 << 23
    assert len(decoy) == 1 and decoy[0]["ref_id"] == 2
    # the range sets: shuffled, both sides of every border, past the end; the long range and its pieces
    sets = gs.range_sets()
    assert [s for c, s, e in sets["borders"][:5]] != sorted(s for c, s, e in sets["borders"][:5])
    assert {e for c, s, e in sets["halves"]} >= set(gs.BORDERS) and {s for c, s, e in sets["halves"]} >= set(gs.BORDERS)
    assert all(any(c == gs.BIG and e > gs.BIG_LEN for c, s, e in v) for v in sets.values())
    c, lo, hi = gs.LONG_RANGE
    assert hi - lo == (1 << 26) - (1 << 20) + 2000 > 6.6e7 and hi > 1 << 26 and sum(e - s for _, s, e in gs.long_range_pieces()) == 10_000
    for r in records:                                         # every read of chrBig lies in a piece, or wholly outside the range
        if r["ref_id"] == 1:
            s, e = r["pos"], r["pos"] + gs.ref_len(r)
            assert any(ps <= s and e <= pe for _, ps, pe in gs.long_range_pieces()) or e <= lo or s >= hi


def test_host_pack_equals_the_python_statement(files):
    tmp, bp, dp, fa, finals, status = files
    references, refs, records, decoy = gs.case()
    nb, nf, idx = open_pair(bp, fa)
    got = lc.native_pack_per_read(nb, nf, idx)
    for k, (rec, (rc, sc, ops)) in enumerate(zip(records, got)):
        contig = refs[references[rec["ref_id"]][0]]
        w_rc, w_sc, w_ops = lc.expected_pack(rec, rec["cigar"], contig)
        assert np.array_equal(rc, w_rc) and np.array_equal(sc, w_sc) and ops == w_ops, (k, rec["name"])
        if rec["_over"]:                                      # N behind the contig's last base, and bases in front of it
            assert len(w_rc) == gs.ref_len(rec) and not w_rc[-rec["_over"]:].any() and w_rc[:-rec["_over"]].all()
            assert rec["pos"] + len(w_rc) == len(contig) + rec["_over"]
    nb.close(); nf.close()
    # a read on the contig the FASTA lacks
    nb, nf = bam.NativeBam(dp, stream=False), bam.NativeFasta(fa)
    one = nb.select([("decoy", 0, 300)])
    assert one.tolist() == [0]
    with pytest.raises(RuntimeError, match="not in the FASTA"):
        nb.pack(nf, one)
    nb.close(); nf.close()


def test_host_records_equal_the_python_statements(files):
    tmp, bp, dp, fa, finals, status = files
    references, refs, records, decoy = gs.case()
    nb, nf, idx = open_pair(bp, fa)
    kept = [k for k, r in enumerate(records) if not r["_bad"]]
    # the reference form: bam.bam_record of the independent decoder's view of the input
    bf = bam.BamFile(bp)
    old = cfg.args
    cfg.args = argparse.Namespace(max_reads=0, regions=gs.whole_regions())
    try:
        rds = list(bam.get_read_data(bf, refs))
    finally:
        cfg.args = old
    assert len(rds) == len(records)
    got = nb.format_bam(idx, finals, status)
    assert got == b"".join(bam.bam_record(rds[k], finals[k], bf.references) for k in kept)
    raws = fc.input_records(bp)
    full = nb.format_bam_full(nf, idx, finals, status)
    want = []
    for k in kept:
        rc, sc, _ = lc.expected_pack(records[k], records[k]["cigar"], refs[references[records[k]["ref_id"]][0]])
        want.append(bam.full_record(raws[k], rc, sc, finals[k]))
    assert full == b"".join(want)
    for stream, is_full in ((got, False), (full, True)):
        out = split_records(stream)
        assert len(out) == len(kept)
        for (_, rec), k in zip(out, kept):
            r = records[k]
            f = struct.unpack_from("<iiBBHHHiiii", rec, 4)
            assert (f[0], f[1]) == (r["ref_id"], r["pos"]) and f[4] == spec_reg2bin(r["pos"], r["pos"] + gs.ref_len(r)), (k, is_full)
            mate = (r.get("next_ref_id", -1), r.get("next_pos", -1), r.get("tlen", 0)) if is_full else (-1, -1, gs.ref_len(r))
            assert f[8:11] == mate, (k, is_full)
    # as a file with its index
    path = str(tmp / "host.bam")
    info = write_native(nb, idx, finals, status, path, gs.BATCH)
    assert info["records"] == len(kept) and info["indexed"] == 1
    index_conditions(check_index(path, path + ".bai"))
    nb.close(); nf.close()
