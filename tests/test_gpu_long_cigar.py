"""Long CIGARs on the GPU (see tests/test_long_cigar.py for the rule): records whose real CIGAR lies in the CG tag go
through the file pipeline, the recount and the purity pass like their plain copies (the staged head:
csrc/hostio.hpp stage_record_head, csrc/staged_head.hpp), and a final CIGAR of more than 65 535 operations leaves as
placeholder + CG tag from emit_bam_records_kernel (csrc/bam_emit_kernels.hpp), byte for byte what the host twin and
bam.bam_record write."""
import argparse
import re

import numpy as np
import pytest

import oracle
from oracle import glue_literal
from model import cms_model, purity_model
from npore_amd import aln, bam, cfg, cig, purity
from test_bam_out import Hdr, check_index, decoded_lines, header_len, members, split_records
import long_cigar_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gpu_long_cigar_small")
    references, refs, records = lc.small_records()
    plain, cg = str(tmp / "plain.bam"), str(tmp / "cg.bam")
    bam.write_bam(plain, references, lc.as_plain(records))
    bam.write_bam(cg, references, lc.as_long(records))
    fa = lc.write_fasta(str(tmp / "ref.fa"), refs)
    return dict(tmp=tmp, references=references, refs=refs, records=records, plain=plain, cg=cg, fa=fa)


def record_stream(path):
    data = bam._bgzf_decompress(path)
    return data[header_len(data):]


def run_file(ctx, path, fa, regions, out, one_pass, out_format, compress="none", r=30, batch_reads=4):
    """one file run; returns the status bits that were set"""
    nf = bam.NativeFasta(fa)
    nb = bam.NativeBam(path, one_pass=one_pass, share=False)
    try:
        if out_format == "bam":
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        kw = dict(batch_reads=batch_reads, r=r, out_format=out_format, bai=out + ".bai" if out_format == "bam" else None, compress=compress)
        if one_pass:
            n, bad, _ = nb.realign_sequential(ctx, nf, regions, out, **kw)
            return n, bad
        idx = nb.select(regions)
        st = nb.realign_file(ctx, nf, idx, out, **kw)
        return len(idx), [(int(k), int(st[k])) for k in np.nonzero(st)[0]]
    finally:
        nb.close(); nf.close()


@pytest.mark.parametrize("device_pack", [True, False])
def test_small_cg_copy_equals_plain_copy(ctx, small, tmp_path, monkeypatch, device_pack):
    if not device_pack:
        monkeypatch.setenv("NPORE_DEVICE_PACK", "0")
    regions = [("ctg", 0, small["references"][0][1] - 1)]
    n = len(small["records"])
    first = None
    for one_pass in (True, False):
        for fmt in ("sam", "bam"):
            outs = []
            for copy in ("plain", "cg"):
                out = str(tmp_path / f"{copy}_{int(one_pass)}.{fmt}")
                assert run_file(ctx, small[copy], small["fa"], regions, out, one_pass, fmt) == (n, []), (copy, one_pass, fmt)
                outs.append(open(out).read() if fmt == "sam" else record_stream(out))
            assert outs[0] == outs[1], (one_pass, fmt)
            if fmt == "sam":
                assert outs[0].count("\n") == n
                first = first or outs[0]
                assert outs[0] == first
            else:
                out = str(tmp_path / f"cg_{int(one_pass)}.bam")
                check_index(out, out + ".bai")
                assert "".join(decoded_lines(out, small["refs"])) == first


def test_small_recount_and_purity(small):
    references, refs = small["references"], small["refs"]
    names = [n for n, _ in references]
    ranges = [("ctg", 0, references[0][1]), ("ctg", 100, 900)]
    c2 = aln.Context(None, None, max_n=6, max_l=100, device=0)
    try:
        want = lc.twin_count(small["cg"], names, refs, ranges, 6, 100)
        for one_pass in (True, False):
            got = []
            for copy in ("plain", "cg"):
                h = bam.NativeBam(small[copy], one_pass=one_pass, share=False)
                try:
                    got.append(bam.confusion_from_bam(c2, h, small["fa"], ranges))
                finally:
                    h.close()
            for g in got:
                assert cms_model.same(g[:4], want[:4]) and cms_model.tallies_agree(g[4], want[4])
                assert g[4]["records_refskip"] == 0 and g[4]["records"] == want[4]["records"] > 0
        ranges = [("ctg", 0, references[0][1])]
        pw = lc.purity_twin(small["cg"], names, ranges, references[0][1])
        c2.set("purity_window", 64)
        spans = [(r["pos"] // 64, (r["pos"] + lc.ref_len(r["cigar"]) - 1) // 64) for r in small["records"]]
        assert all(b > a for a, b in spans)                      # every record is carried across a window border
        for one_pass in (True, False):
            for copy in ("plain", "cg"):
                h = bam.NativeBam(small[copy], one_pass=one_pass, share=False)
                try:
                    hb, hi, tallies, rows, _ = purity.purity_from_bam(c2, h, ranges, per_position=True)
                finally:
                    h.close()
                assert np.array_equal(rows, pw[0]) and np.array_equal(hb, pw[1]) and np.array_equal(hi, pw[2]), (one_pass, copy)
                assert purity_model.tallies_agree(tallies, pw[3]) and tallies["records_refskip"] == 0
                assert tallies["records"] == len(small["records"]) and tallies["windows"] > 10
    finally:
        c2.close()


# ---- one read of 180 kb: 72 000 operations on the way in, more than 65 535 on the way out ------------------------------------
@pytest.fixture(scope="module")
def ultra(tmp_path_factory, tables):
    tmp = tmp_path_factory.mktemp("gpu_long_cigar_ultra")
    references, refs, records = lc.ultra_long_read()
    path = str(tmp / "ultra.bam")
    bam.write_bam(path, references, records, level=1)
    assert len(records[1]["cigar"]) == 72000
    fa = lc.write_fasta(str(tmp / "big.fa"), refs)
    sub, nps = tables
    finals = []
    for r in records:
        ref, seq, ops = lc.expected_pack(r, r["cigar"], refs["big"])
        a = oracle.align(ref, seq, ops, sub, nps, r=10, max_b_rows=20000)
        finals.append(cig.collapse_cigar(glue_literal.standardize(a, ref, seq)))
    return dict(tmp=tmp, references=references, refs=refs, records=records, path=path, fa=fa, finals=finals)


def test_ultra_long_read(ctx, ultra):
    tmp, finals = ultra["tmp"], ultra["finals"]
    n_ops = [len(re.findall(r"\d+[MID]", f)) for f in finals]
    assert n_ops[1] > 65535 and max(n_ops[0], n_ops[2]) < 100, n_ops           # the premise: the read crosses the limit on the way out, too
    regions = [("big", 0, ultra["references"][0][1] - 1)]
    sam = str(tmp / "u.sam")
    assert run_file(ctx, ultra["path"], ultra["fa"], regions, sam, True, "sam", r=10) == (3, [])
    lines = open(sam).read().splitlines()
    assert [l.split("\t")[0] for l in lines] == ["before", "ultra", "after"]
    assert [l.split("\t")[5] for l in lines] == finals
    # the records: device == host twin == the Python statement, stored and coded members
    nb = bam.NativeBam(ultra["path"])
    idx = nb.select(regions)
    st = np.zeros(3, np.int32)
    want = nb.format_bam(idx, finals, st)
    old = cfg.args
    cfg.args = argparse.Namespace(max_reads=0, regions=regions)
    try:
        rds = list(bam.get_read_data(bam.BamFile(ultra["path"]), ultra["refs"]))
    finally:
        cfg.args = old
    nb.close()
    assert want == b"".join(bam.bam_record(rd, f, ["big"]) for rd, f in zip(rds, finals))
    recs = [r for _, r in split_records(want)]
    assert [int.from_bytes(r[16:18], "little") for r in recs] == [n_ops[0], 2, n_ops[2]]
    assert len(recs[1]) > 6 * 65280                                              # a record that spans several members
    outs = {}
    for compress in ("none", "huffman"):
        for one_pass in (True, False):
            out = str(tmp / f"u_{compress}_{int(one_pass)}.bam")
            assert run_file(ctx, ultra["path"], ultra["fa"], regions, out, one_pass, "bam", compress, r=10) == (3, [])
            assert record_stream(out) == want, (compress, one_pass)
            members(out)
            check_index(out, out + ".bai")
        outs[compress] = out
    # ... and back in: the Python reader, and the native one through a second run to SAM
    want_cigars = [[(int(n), "MID".index(op)) for n, op in re.findall(r"(\d+)([MID])", f)] for f in finals]
    for compress, out in outs.items():
        assert [[(ln, op) for op, ln in r.cigar] for r in bam.BamFile(out).records] == want_cigars
    back = str(tmp / "back.sam")
    assert run_file(ctx, outs["huffman"], ultra["fa"], regions, back, True, "sam", r=10)[0] == 3
    again = [l.split("\t") for l in open(back).read().splitlines()]
    assert [f[0] for f in again] == ["before", "ultra", "after"]
    assert all(f[9] == l.split("\t")[9] and f[8] == l.split("\t")[8] for f, l in zip(again, lines))


def test_ultra_long_read_recount_and_purity(ultra):
    references, refs = ultra["references"], ultra["refs"]
    names = [n for n, _ in references]
    ranges = [("big", 0, references[0][1])]
    c2 = aln.Context(None, None, max_n=6, max_l=100, device=0)
    try:
        want = lc.twin_count(ultra["path"], names, refs, ranges, 6, 100)
        got = bam.confusion_from_bam(c2, ultra["path"], ultra["fa"], ranges)
        assert cms_model.same(got[:4], want[:4]) and cms_model.tallies_agree(got[4], want[4])
        assert got[4]["records_refskip"] == 0 and got[4]["records"] == 3 and got[4]["entries_counted"] > 150000      # (180 000 bases, a tenth of them below min_bq)
        pw = lc.purity_twin(ultra["path"], names, ranges, references[0][1])
        hb, hi, tallies, rows, _ = purity.purity_from_bam(c2, ultra["path"], ranges, per_position=True)
        assert np.array_equal(rows, pw[0]) and np.array_equal(hb, pw[1]) and np.array_equal(hi, pw[2])
        assert purity_model.tallies_agree(tallies, pw[3]) and tallies["records_refskip"] == 0 and tallies["records"] == 3
    finally:
        c2.close()
