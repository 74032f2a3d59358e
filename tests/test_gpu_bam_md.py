"""The MD tag of the FULL records (--records full --md) on the GPU: md_size_kernel and emit_md_kernel
(csrc/bam_emit_kernels.hpp, ONE walk with two sinks) against the host twin npore_bam_format_bam_full_md and the Python
statement bam.md_of -- on crafted final CIGARs through the debug entry, in the file pipeline in every configuration, with
coded members, on a read of more than 65 535 operations, through the CLI and with two ranks.  The rule is stated in
csrc/md_rec.hpp.  Every child process runs under its own time limit.
"""
import argparse
import os
import sys

import numpy as np
import pytest

from npore_amd import aln, bam, cfg
from conftest import GOLDEN, REPO
from test_bam_out import Hdr, check_index, decoded_lines, members, split_records
from test_gpu_bam_full import realign_cli, record_stream
import bam_full_cases as fc
import bam_md_cases as mc
import long_cigar_cases as lc
from full_record_driver import device_full

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, "data")


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


# ---- 1. crafted reads through the debug entry -----------------------------------------------------------------------------------
def test_crafted_reads_device_equals_host(ctx, tmp_path):
    references, refs, records, finals, pinned = mc.crafted_reads()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "md")
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in references])
    assert len(idx) == len(records)
    status = np.array([r["_status"] for r in records], np.int32)
    want = nb.format_bam_full(nf, idx, finals, status, md=True)
    want_len = []
    for r, fin in zip(records, finals):
        rc, sc, _ = lc.expected_pack(r, r["cigar"], refs[r["_ctg"]])
        text = bam.md_of(rc, sc, fin)
        assert pinned.get(r["name"], text) == text, r["name"]
        want_len.append(0 if r["_status"] else len(text))
    got, nm, md_len = device_full(ctx, nb, nf, idx, finals, status, entry="_md", md=True)
    print("md_len", md_len.tolist())
    assert md_len.tolist() == want_len
    assert got == want
    assert {1, 2, 3, 4, 6, 261} <= set(want_len) and 0 in want_len
    # 300 picks of the same reads in another order, in one call
    rng = np.random.default_rng(1)
    pick = rng.integers(0, len(records), 300)
    got, nm, md_len = device_full(ctx, nb, nf, idx[pick], [finals[k] for k in pick], status[pick], entry="_md", md=True)
    assert md_len.tolist() == [want_len[k] for k in pick]
    assert got == nb.format_bam_full(nf, idx[pick], [finals[k] for k in pick], status[pick], md=True)
    # flags = 0: the bytes of the entry point without the tag, md_len untouched
    got0, nm0, md0 = device_full(ctx, nb, nf, idx, finals, status, entry="_md", md=False)
    old, nm_old, _ = device_full(ctx, nb, nf, idx, finals, status, entry="")
    assert got0 == old == nb.format_bam_full(nf, idx, finals, status) and nm0.tolist() == nm_old.tolist()
    assert (md0 == -1).all()
    nb.close(); nf.close()


# ---- 2. the file pipeline -----------------------------------------------------------------------------------------------------
def test_file_pipeline_md(ctx, tmp_path):
    references, refs, records, cigars = fc.full_records()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records)
    clen, n = references[0][1], len(records)
    regions = [("ctg", 0, clen - 1)]
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=regions, max_reads=0)
    try:
        nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
        idx = nb.select(regions)
        assert len(idx) == n
        sam = tmp_path / "route.sam"
        st = nb.realign_file(ctx, nf, idx, str(sam), batch_reads=5, r=30)
        text = sam.read_text()
        assert ((st & 32) != 0).sum() == 1 and st[7] & 32 and text.count("\n") == n - 1
        finals, it = [], iter(text.splitlines())
        for k in range(n):
            finals.append("" if st[k] & 32 else next(it).split("\t")[5])
        # the record stream is the Python statement's
        for r in records:
            r.setdefault("_ctg", "ctg")
        want = mc.want_stream(fc.input_records(bp), records, refs, finals, st)
        assert want == nb.format_bam_full(nf, idx, finals, st, md=True)
        files = {}

        def run(name, **kw):
            out = str(tmp_path / name)
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            stb = nb.realign_file(ctx, nf, idx, out, r=30, out_format="bam", bai=out + ".bai", records="full", md=True, **kw)
            assert np.array_equal(stb, st), name
            assert record_stream(out) == want, name
            files[name] = (open(out, "rb").read(), open(out + ".bai", "rb").read())
            return out

        dev = run("dev.bam", batch_reads=5)
        assert nb.output_info()["records"] == n - 1
        run("dev_one_batch.bam", batch_reads=1000)
        for key in ("device_pack", "device_glue"):
            ctx.set(key, 0)
            try:
                run(f"no_{key}.bam", batch_reads=5)
            finally:
                ctx.set(key, 1)
        ctx.set("tb_budget_mb", 2)                           # every batch in several groups
        try:
            run("groups.bam", batch_reads=12)
        finally:
            ctx.set("tb_budget_mb", 0)
        one = bam.NativeBam(bp, one_pass=True)
        out = str(tmp_path / "onepass.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        n5, bad5, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=5, r=30, out_format="bam", bai=out + ".bai", records="full",
                                             md=True)
        assert n5 == n and bad5 == [(7, 32)]
        files["onepass.bam"] = (open(out, "rb").read(), open(out + ".bai", "rb").read())
        assert len(set(files.values())) == 1, [k for k, v in files.items() if v != files["dev.bam"]]
        check_index(dev, dev + ".bai")
        members(dev)
        assert "".join(fc.without_clips(decoded_lines(dev, bam.read_fasta(fa)))) == text
        # coded members: the same record stream
        for compress in ("huffman", "match"):
            assert record_stream(run(f"{compress}.bam", batch_reads=5, compress=compress)) == want
            check_index(str(tmp_path / f"{compress}.bam"), str(tmp_path / f"{compress}.bam.bai"))
        # the flag holds for one run: the next one on the handle without md writes today's FULL bytes
        out = str(tmp_path / "again.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        one.realign_sequential(ctx, nf, regions, out, batch_reads=5, r=30, out_format="bam", records="full")
        assert record_stream(out) == nb.format_bam_full(nf, idx, finals, st) != want
        one.close(); nb.close(); nf.close()
    finally:
        cfg.args = old


# ---- 3. a read of more than 65 535 operations ---------------------------------------------------------------------------------
def test_ultra_long_read_md(ctx, tmp_path):
    references, refs, records = lc.ultra_long_read()
    for k, r in enumerate(records):
        r["tags"] = b"RGZlong\0" + b"MDZ7\0" + b"MLBC" + (100 + k).to_bytes(4, "little") + bytes(100 + k)
    bp = str(tmp_path / "ultra.bam")
    bam.write_bam(bp, references, records, level=1)
    fa = lc.write_fasta(str(tmp_path / "big.fa"), refs)
    regions = [("big", 0, references[0][1] - 1)]
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=regions, max_reads=0)
    try:
        nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
        idx = nb.select(regions)
        sam = tmp_path / "u.sam"
        st = nb.realign_file(ctx, nf, idx, str(sam), batch_reads=4, r=10)
        assert not st.any()
        finals = [l.split("\t")[5] for l in sam.read_text().splitlines()]
        n_ops = [f.count("M") + f.count("I") + f.count("D") for f in finals]
        assert n_ops[1] > 65535 and max(n_ops[0], n_ops[2]) < 100, n_ops
        want = nb.format_bam_full(nf, idx, finals, st, md=True)
        out = str(tmp_path / "u.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        nb.realign_file(ctx, nf, idx, out, batch_reads=4, r=10, out_format="bam", bai=out + ".bai", records="full", md=True)
        assert record_stream(out) == want
        check_index(out, out + ".bai")
        rec = split_records(want)[1][1]
        f, _, words, _, aux = fc.parse_full(rec)
        assert f[5] == 2 and words == [len(records[1]["seq"]) << 4 | 4, 6 * 36000 << 4 | 3]
        tags = mc.parse_tags(aux)
        assert [t for t, _, _ in tags] == [b"RG", b"ML", b"HP", b"NM", b"MD", b"CG"]          # kept aux, NM, MD, CG
        cg = tags[-1][2]
        assert cg[:5] == b"I" + n_ops[1].to_bytes(4, "little") and len(cg) == 5 + 4 * n_ops[1]
        text, nm, _, _ = mc.md_and_nm(rec)
        contig = refs["big"]
        seq = records[1]["seq"]
        assert mc.rebuild_reference(text, seq, finals[1]) == contig[100:100 + 6 * 36000]
        assert nm == sum(c.isalpha() for c in text) + sum(int(x) for x in __import__("re").findall(r"(\d+)I", finals[1]))
        nb.close(); nf.close()
    finally:
        cfg.args = old


# ---- 4. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_md(tmp_path):
    import re
    common = ["--bam", os.path.join(DATA, "reads.bam"), "--ref", os.path.join(DATA, "ref.fasta"), "--out_format", "bam", "--records", "full", "--md"]
    p1, p2 = str(tmp_path / "one"), str(tmp_path / "ix")
    realign_cli(common + ["--out_prefix", p1], 300)
    realign_cli(common + ["--out_prefix", p2], 300, env=dict(os.environ, NPORE_BAM_ONE_PASS="0"))
    assert record_stream(p1 + ".bam") == record_stream(p2 + ".bam")
    refs = bam.read_fasta(os.path.join(DATA, "ref.fasta"))
    gold = [l for l in open(os.path.join(DATA, "npore_realigned.sam")) if not l.startswith("@")]
    assert fc.without_clips(decoded_lines(p1 + ".bam", refs)) == gold and len(gold) == 10
    # the MD reader rebuilds every read's reference slice from the FASTA
    final_of = {l.split("\t")[0]: l.split("\t") for l in gold}
    recs = split_records(record_stream(p1 + ".bam"))
    assert len(recs) == 10
    for _, rec in recs:
        f, name, words, body, aux = fc.parse_full(rec)
        text, nm, _, names = mc.md_and_nm(rec)
        line = final_of[name[:-1].decode()]
        seq, fin = line[9], line[5]
        contig = refs[line[2]]
        contig = contig if isinstance(contig, str) else "".join(contig)
        rl = sum(int(n) for n, op in re.findall(r"(\d+)([MD])", fin))
        if not re.search(r"[^ACGT]", seq + contig[f[1]:f[1] + rl].upper()):
            assert mc.rebuild_reference(text, seq, fin) == contig[f[1]:f[1] + rl].upper(), name
        assert nm == sum(c.isalpha() for c in text) + sum(int(n) for n in re.findall(r"(\d+)I", fin)), name
    for p in (p1, p2):
        members(p + ".bam")
        check_index(p + ".bam", p + ".bam.bai")


# ---- 5. two ranks ---------------------------------------------------------------------------------------------------------------
def test_two_ranks_md(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import bench_realign
    bp, fa, clen = bench_realign.build_inputs(str(tmp_path), 200, 0, 1500, 31, procs=2, tags=True)
    bam.write_bai(bp)
    common = ["--bam", bp, "--ref", fa, "--out_format", "bam", "--records", "full", "--md", "--batch_reads", "40"]
    b1, b2 = str(tmp_path / "single"), str(tmp_path / "two")
    realign_cli(common + ["--out_prefix", b1], 300)
    out = realign_cli(common + ["--out_prefix", b2], 600,
                      launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                "--master-port", str(29700 + os.getpid() % 100)])
    assert "no .bai index" not in out.stdout
    one = record_stream(b1 + ".bam")
    assert record_stream(b2 + ".bam") == one and len(split_records(one)) == 200
    assert all(mc.md_and_nm(r)[3][-2:] == [b"NM", b"MD"] for _, r in split_records(one))
    for p in (b1, b2):
        members(p + ".bam")
        check_index(p + ".bam", p + ".bam.bai")
