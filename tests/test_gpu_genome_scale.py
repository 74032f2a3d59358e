"""The device record paths at genome coordinates, on many contigs (tests/genome_scale_cases.py; tests/test_genome_scale_cases.py
shows on the CPU what the inputs cross): unpack_records_kernel's contig table by BAM reference id and its 64-bit position
arithmetic, bam_reg2bin_dev at every level of the bin scheme, refID and the mate fields of the emitted records, the index,
region selection above 2^26, a contig the FASTA lacks, two ranks, and the range tables of the purity and confusion counts.
Every comparison is exact (bytes, integers, status bits) but the purity scores' bound of test_gpu_purity._same.
Every child process runs under its own time limit."""
import argparse
import os
import struct

import numpy as np
import pytest

import oracle
from model import cms_model as m
from model import purity_model as pm
from npore_amd import aln, bam, cfg, cig
from test_bam_out import Hdr, check_index, members, spec_reg2bin, split_records
from test_genome_scale_cases import index_conditions
from test_gpu_bam_full import realign_cli, record_stream
from test_gpu_confusion_rec import _device as recount_device
from test_gpu_purity import _device as purity_device, _same as purity_same
import bam_full_cases as fc
import genome_scale_cases as gs
import long_cigar_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the FASTA (68 MB) and the two BAMs, written once"""
    tmp = tmp_path_factory.mktemp("genome")
    return (tmp,) + gs.write_inputs(tmp)


@pytest.fixture(scope="module")
def args():
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=gs.whole_regions(), max_reads=0)
    yield
    cfg.args = old


def _finals(text, st):
    it = iter(text.splitlines())
    return ["" if s & 32 else next(it).split("\t")[5] for s in st]


@pytest.fixture(scope="module")
def route(ctx, files, args):
    """test 1's run, which the other tests build on: (SAM text, status, final CIGARs) at batch_reads = 5, device_pack = 1"""
    tmp, bp, dp, fa = files
    nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
    idx = nb.select(gs.whole_regions())
    sam = tmp / "route.sam"
    st = nb.realign_file(ctx, nf, idx, str(sam), batch_reads=gs.BATCH, r=30)
    nb.close(); nf.close()
    text = sam.read_text()
    return text, st.copy(), _finals(text, st)


def _contig_of(rec):
    return gs.case()[1][gs.HEADER[rec["ref_id"]][0]]


# ---- 1. unpack and align ------------------------------------------------------------------------------------------------------
def test_unpack_and_align_against_the_oracle(ctx, tables, files, route):
    """the SAM route with the device's and the host's packer: the same text and status; every CIGAR is the oracle's on the codes
    the Python statement slices from the contig the read's refID names -- N past the contig's end"""
    tmp, bp, dp, fa = files
    text, st, finals = route
    records = gs.case()[2]
    sub, nps = tables
    assert len(st) == len(records)
    nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
    idx = nb.select(gs.whole_regions())
    ctx.set("device_pack", 0)
    try:
        sam = tmp / "host_pack.sam"
        st0 = nb.realign_file(ctx, nf, idx, str(sam), batch_reads=gs.BATCH, r=30)
    finally:
        ctx.set("device_pack", 1)
    nb.close(); nf.close()
    assert sam.read_text() == text and np.array_equal(st0, st)
    lines = iter(text.splitlines())
    for k, rec in enumerate(records):
        rc, sc, ops = lc.expected_pack(rec, rec["cigar"], _contig_of(rec))
        if rec["_bad"]:
            with pytest.raises(ValueError):
                oracle.align(rc, sc, ops, sub, nps, r=30)
            assert st[k] == 32
            continue
        raw, wst = oracle.align(rc, sc, ops, sub, nps, r=30, return_status=True)
        f = next(lines).split("\t")
        assert (f[0], f[2], int(f[3])) == (rec["name"], gs.HEADER[rec["ref_id"]][0], rec["pos"] + 1), k
        assert f[5] == cig.collapse_cigar(cig.standardize(raw, rc, sc)), (k, rec["name"], rec["_place"], rec["_over"])
        assert st[k] == wst, (k, st[k], wst)
    assert next(lines, None) is None and ((st & 32) != 0).sum() == 1


# ---- 2. / 3. records of both forms, and their index ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["reference", "full"])
def test_records_and_index(ctx, files, route, form):
    """the record stream of every configuration is the host twin's of test 1's final CIGARs (and, FULL, the Python statement's);
    bins by spec_reg2bin, refID and mate fields the input's; all files and indices of one form byte-identical; the index
    holds the walk of check_index and reaches chrBig's last window"""
    tmp, bp, dp, fa = files
    text, st, finals = route
    references, refs, records, _ = gs.case()
    regions = gs.whole_regions()
    nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
    idx = nb.select(regions)
    if form == "full":
        want = nb.format_bam_full(nf, idx, finals, st)
        raws, out = fc.input_records(bp), []
        for raw, rec, fin, s in zip(raws, records, finals, st):
            if not s & 32:
                rc, sc, _ = lc.expected_pack(rec, rec["cigar"], _contig_of(rec))
                out.append(bam.full_record(raw, rc, sc, fin))
        assert want == b"".join(out)
    else:
        want = nb.format_bam(idx, finals, st)
    kept = [k for k, r in enumerate(records) if not r["_bad"]]
    got = split_records(want)
    assert len(got) == len(kept)
    for (_, rec), k in zip(got, kept):
        r = records[k]
        f = struct.unpack_from("<iiBBHHHiiii", rec, 4)
        assert (f[0], f[1]) == (r["ref_id"], r["pos"]) and f[4] == spec_reg2bin(r["pos"], r["pos"] + gs.ref_len(r)), k
        assert f[8:11] == ((r.get("next_ref_id", -1), r.get("next_pos", -1), r.get("tlen", 0)) if form == "full" else (-1, -1, gs.ref_len(r))), k
    files_of, kw = {}, dict(r=30, out_format="bam", records=form)

    def run(name, **more):
        out = str(tmp / f"{form}_{name}")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        stb = nb.realign_file(ctx, nf, idx, out, bai=out + ".bai", **kw, **more)
        assert np.array_equal(stb, st), name
        assert record_stream(out) == want, name
        if "compress" not in more:
            files_of[name] = (open(out, "rb").read(), open(out + ".bai", "rb").read())
        return out

    dev = run("b5.bam", batch_reads=gs.BATCH)
    assert nb.output_info()["records"] == len(kept)
    run("b1000.bam", batch_reads=1000)
    for key in ("device_pack", "device_glue"):
        ctx.set(key, 0)
        try:
            run(f"no_{key}.bam", batch_reads=gs.BATCH)
        finally:
            ctx.set(key, 1)
    ctx.set("tb_budget_mb", 2)
    try:
        run("groups.bam", batch_reads=12)
    finally:
        ctx.set("tb_budget_mb", 0)
    one = bam.NativeBam(bp, one_pass=True)
    out = str(tmp / f"{form}_onepass.bam")
    bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
    n_sel, bad, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=gs.BATCH, bai=out + ".bai", **kw)
    one.close()
    assert n_sel == len(records) and bad == [(k, 32) for k, r in enumerate(records) if r["_bad"]]
    files_of["onepass.bam"] = (open(out, "rb").read(), open(out + ".bai", "rb").read())
    assert len(set(files_of.values())) == 1, [k for k, v in files_of.items() if v != files_of["b5.bam"]]
    members(dev)
    index_conditions(check_index(dev, dev + ".bai"))
    for compress in ("huffman", "match"):
        out = run(f"{compress}.bam", batch_reads=gs.BATCH, compress=compress)
        index_conditions(check_index(out, out + ".bai"))
    nb.close(); nf.close()


# ---- 4. regions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_no", range(len(gs.region_sets())))
def test_regions_at_genome_coordinates(ctx, files, route, case_no):
    """regions that start above 2^26, end exactly on a border, skip alpha, leave chrBig's end: the indexed reader selects what the
    overlap rule selects, and the one-pass reader writes the same file"""
    tmp, bp, dp, fa = files
    text, st, finals = route
    records = gs.case()[2]
    what, regions = gs.region_sets()[case_no]
    want_idx = gs.overlapping(records, regions)
    assert 0 < len(want_idx) < len(records)
    nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
    idx = nb.select(regions)
    assert idx.tolist() == want_idx, what
    outs = []
    for name in ("indexed", "onepass"):
        out = str(tmp / f"region{case_no}_{name}.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        if name == "indexed":
            stb = nb.realign_file(ctx, nf, idx, out, batch_reads=gs.BATCH, r=30, out_format="bam", bai=out + ".bai")
            assert np.array_equal(stb, st[want_idx])
        else:
            one = bam.NativeBam(bp, one_pass=True)
            n_sel, bad, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=gs.BATCH, r=30, out_format="bam", bai=out + ".bai")
            one.close()
            assert n_sel == len(want_idx) and bad == [(j, 32) for j, k in enumerate(want_idx) if records[k]["_bad"]]
        outs.append((open(out, "rb").read(), open(out + ".bai", "rb").read()))
        assert record_stream(out) == nb.format_bam(idx, [finals[k] for k in want_idx], st[want_idx]), (what, name)
        check_index(out, out + ".bai")
    assert outs[0] == outs[1], what
    nb.close(); nf.close()


# ---- 5. a read on a contig that the FASTA lacks ---------------------------------------------------------------------------------
def test_contig_missing_from_the_fasta(ctx, files, route):
    """the file pipeline refuses the read with either packer, writes no record, and the context goes on as before"""
    tmp, bp, dp, fa = files
    text, st, finals = route
    nb, nf = bam.NativeBam(dp), bam.NativeFasta(fa)
    one = nb.select([("decoy", 0, 300)])
    assert one.tolist() == [0]
    for device_pack in (1, 0):
        ctx.set("device_pack", device_pack)
        try:
            sam = tmp / f"decoy{device_pack}.sam"
            with pytest.raises(RuntimeError, match="not in the FASTA"):
                nb.realign_file(ctx, nf, one, str(sam), batch_reads=gs.BATCH, r=30)
            assert not sam.exists() or sam.read_text() == ""
            out = str(tmp / f"decoy{device_pack}.bam")
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            with pytest.raises(RuntimeError, match="not in the FASTA"):
                nb.realign_file(ctx, nf, one, out, batch_reads=gs.BATCH, r=30, out_format="bam", records="full")
            assert split_records(record_stream(out)) == []
        finally:
            ctx.set("device_pack", 1)
    nb.close()
    nb = bam.NativeBam(bp)
    idx = nb.select(gs.whole_regions())[:gs.BATCH]
    sam = tmp / "after_decoy.sam"
    st5 = nb.realign_file(ctx, nf, idx, str(sam), batch_reads=gs.BATCH, r=30)
    nb.close(); nf.close()
    assert np.array_equal(st5, st[:gs.BATCH]) and not st5.any()
    assert sam.read_text() == "".join(text.splitlines(keepends=True)[:gs.BATCH])


def test_contig_missing_from_the_fasta_late_in_a_run(ctx, files, route):
    """the same refusal several batches into a run, with earlier batches on the device: the decoy's read among the main
    records, in coordinate order -- behind chrBig's.  The call fails, the text holds whole batches in front of the decoy's
    and nothing else, and the context goes on as before"""
    tmp, bp, dp, fa = files
    text, st, finals = route
    references, refs, records, decoy = gs.case()
    mixed = sorted(gs.plain(records) + decoy, key=lambda r: (r["ref_id"], r["pos"]))
    at = [r["name"] for r in mixed].index("onDecoy")
    assert at // gs.BATCH >= 3 and mixed[:at] == gs.plain(records)[:at]
    mp = str(tmp / "mixed.bam")
    bam.write_bam(mp, references, mixed)
    bam.write_bai(mp)
    lines = text.splitlines(keepends=True)
    # the text of the first j whole batches, for every j in front of the decoy's batch (a refused read has no line)
    prefixes = ["".join(lines[:int(((st[:j * gs.BATCH] & 32) == 0).sum())]) for j in range(at // gs.BATCH + 1)]
    everything = [(n, 0, l) for n, l in gs.HEADER]
    nf = bam.NativeFasta(fa)
    for how in ("device_pack", "host_pack", "one_pass"):
        ctx.set("device_pack", 0 if how == "host_pack" else 1)
        nb = bam.NativeBam(mp, one_pass=how == "one_pass")
        sam = tmp / f"mixed_{how}.sam"
        try:
            with pytest.raises(RuntimeError, match="not in the FASTA"):
                if how == "one_pass":
                    nb.realign_sequential(ctx, nf, everything, str(sam), batch_reads=gs.BATCH, r=30)
                else:
                    idx = nb.select(everything)
                    assert len(idx) == len(mixed)
                    nb.realign_file(ctx, nf, idx, str(sam), batch_reads=gs.BATCH, r=30)
        finally:
            ctx.set("device_pack", 1)
            nb.close()
        got = sam.read_text() if sam.exists() else ""
        assert got in prefixes, (how, len(got), [len(p) for p in prefixes])
        nb = bam.NativeBam(bp)
        idx = nb.select(gs.whole_regions())
        again = tmp / f"after_mixed_{how}.sam"
        st_again = nb.realign_file(ctx, nf, idx, str(again), batch_reads=gs.BATCH, r=30)
        nb.close()
        assert np.array_equal(st_again, st) and again.read_text() == text, how
    nf.close()


# ---- 6. two ranks ---------------------------------------------------------------------------------------------------------------
def test_two_ranks_at_genome_coordinates(files):
    tmp, bp, dp, fa = files
    records = gs.case()[2]
    common = ["--bam", bp, "--ref", fa, "--out_format", "bam", "--records", "full", "--batch_reads", str(gs.BATCH)]
    b1, b2 = str(tmp / "single"), str(tmp / "two")
    realign_cli(common + ["--out_prefix", b1], 300)
    out = realign_cli(common + ["--out_prefix", b2], 600,
                      launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                "--master-port", str(29700 + os.getpid() % 100)])
    assert "no .bai index" not in out.stdout
    one = record_stream(b1 + ".bam")
    assert record_stream(b2 + ".bam") == one
    got = split_records(one)
    kept = [r for r in records if not r["_bad"]]
    assert [struct.unpack_from("<ii", rec, 4) for _, rec in got] == [(r["ref_id"], r["pos"]) for r in kept]
    for p in (b1, b2):
        members(p + ".bam")
        index_conditions(check_index(p + ".bam", p + ".bam.bai"))
    assert not any(os.path.exists(f"{b2}.part{k}.bam{ext}") for k in (0, 1) for ext in ("", ".bai"))


# ---- 7. pileup counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["borders", "halves"])
def test_purity_at_genome_coordinates(files, name):
    """purity_records_kernel's range table at positions above 2^26: the default window and windows of 64 dense positions, the
    one-pass and the indexed reader, against the pileup model"""
    tmp, bp, dp, fa = files
    ranges = gs.range_sets()[name]
    want = pm.expected(bp, ranges)
    assert want[4]["records"] >= 30 and want[4]["records_malformed"] == 1 and want[4]["star_entries"] > 0
    for one_pass in (True, False):
        for window in (None, 64):
            h = bam.NativeBam(bp, one_pass=one_pass, share=False)
            try:
                got = purity_device(bp, ranges, handle=h, window=window)
            finally:
                h.close()
            purity_same(got, want)


def test_purity_over_a_range_of_66_million_positions(files):
    """LONG_RANGE, 6.6e7 dense positions in windows of 2^22, no per-position rows: the histograms and tallies are the model's
    on gs.long_range_pieces() -- the 10 000 positions of the range that a read can touch (the reasoning stands there); the
    model itself is not run on 6.6e7 positions, each of which costs it a Python list"""
    from npore_amd import purity
    tmp, bp, dp, fa = files
    rows, hb, hi, scores, tallies = pm.expected(bp, gs.long_range_pieces())
    # (six reads and the refused one at each of the three borders in the range; read a alone covers 300 positions at each)
    assert tallies["records"] == 18 and tallies["records_malformed"] == 1 and tallies["positions_covered"] > 3 * 200
    for one_pass in (True, False):
        c = aln.Context(None, None, max_n=6, max_l=100, device=0)
        h = bam.NativeBam(bp, one_pass=one_pass, share=False)
        try:
            c.set("purity_window", 1 << 22)
            got = purity.purity_from_bam(c, h, [gs.LONG_RANGE])
        finally:
            h.close()
            c.close()
        assert np.array_equal(got[0], hb) and np.array_equal(got[1], hi)
        assert pm.tallies_agree(got[2], tallies), (got[2], dict(tallies))
        # (the pieces lie more than a window apart, and the range holds 16 windows)
        assert 3 <= got[2]["windows"] <= -(-(gs.LONG_RANGE[2] - gs.LONG_RANGE[1]) // (1 << 22)) == 16


@pytest.mark.parametrize("max_n,max_l", [(6, 100), (4, 20)])
def test_confusion_at_genome_coordinates(files, max_n, max_l):
    """confusion_records_kernel's range table and the contig slices behind it: the FASTA's order is not the header's, so a contig
    table taken in the wrong order counts against another contig's bases"""
    tmp, bp, dp, fa = files
    refs = gs.case()[1]
    for name, ranges in gs.range_sets().items():
        want, tallies = m.expected(bp, refs, ranges, max_n, max_l)
        assert tallies["records"] >= 30 and tallies["entries_counted"] > 3000
        for one_pass in (True, False):
            h = bam.NativeBam(bp, one_pass=one_pass, share=False)
            try:
                got = recount_device(bp, ranges, max_n, max_l, fa, handle=h)
            finally:
                h.close()
            assert m.same(got, want), (name, one_pass, [(int(a.sum()), int(b.sum())) for a, b in zip(got[:4], want)])
            assert m.tallies_agree(got[4], tallies), (name, one_pass, got[4], dict(tallies))
