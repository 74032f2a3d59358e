"""FULL records (--records full) on the GPU: nm_count_kernel, place_bam_full_kernel and emit_bam_full_kernel
(csrc/bam_emit_kernels.hpp) against the host twin npore_bam_format_bam_full -- on crafted final CIGARs through the debug
entry, in the file pipeline in every configuration, with coded members, on a read of more than 65 535 operations, through
the CLI and with two ranks.  The format is stated in csrc/bam_reader.hpp ("FULL RECORD"), NM in csrc/nm_rec.hpp.
Every child process runs under its own time limit.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

from npore_amd import aln, bam, cfg
from conftest import GOLDEN, REPO
from test_bam_out import Hdr, check_index, decoded_lines, header_len, members, split_records
import bam_full_cases as fc
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


def record_stream(path):
    data = bam._bgzf_decompress(path)
    return data[header_len(data):]


# ---- 1. NM and records on crafted CIGARs ------------------------------------------------------------------------------------
def test_crafted_cigars_device_equals_host(ctx, tmp_path):
    references, refs, records, finals = fc.crafted_reads()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "nm")
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([("ctg", 0, references[0][1])])
    assert len(idx) == len(records)
    status = np.array([r["_status"] for r in records], np.int32)
    want = nb.format_bam_full(nf, idx, finals, status)
    got, nm, _ = device_full(ctx, nb, nf, idx, finals, status, entry="")
    want_nm = []
    for r, fin in zip(records, finals):
        rc, sc, _ = lc.expected_pack(r, r["cigar"], refs["ctg"])
        want_nm.append(0 if r["_status"] else bam.nm_of(rc, sc, fin))
    assert nm.tolist() == want_nm
    assert {255, 256, 65536} <= set(want_nm)
    assert got == want
    assert max(len(r) for _, r in split_records(got)) > 40000            # the 40 000-byte tag: a record that spans a member cut
    # 300 reads in one call (the same records again and again, in another order)
    rng = np.random.default_rng(1)
    pick = rng.integers(0, len(records), 300)
    got, nm, _ = device_full(ctx, nb, nf, idx[pick], [finals[k] for k in pick], status[pick], entry="")
    assert nm.tolist() == [want_nm[k] for k in pick]
    assert got == nb.format_bam_full(nf, idx[pick], [finals[k] for k in pick], status[pick])
    nb.close(); nf.close()


# ---- 2. the file pipeline -----------------------------------------------------------------------------------------------------
def test_file_pipeline_full_records(ctx, tmp_path):
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
        want = nb.format_bam_full(nf, idx, finals, st)
        assert want == fc.want_stream(fc.input_records(bp), records, cigars, refs["ctg"], finals, st)
        files = {}

        def run(name, **kw):
            out = str(tmp_path / name)
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            stb = nb.realign_file(ctx, nf, idx, out, r=30, out_format="bam", bai=out + ".bai", records="full", **kw)
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
        n5, bad5, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=5, r=30, out_format="bam", bai=out + ".bai", records="full")
        assert n5 == n and bad5 == [(7, 32)]
        files["onepass.bam"] = (open(out, "rb").read(), open(out + ".bai", "rb").read())
        assert len(set(files.values())) == 1, [k for k, v in files.items() if v != files["dev.bam"]]
        check_index(dev, dev + ".bai")
        members(dev)
        assert "".join(fc.without_clips(decoded_lines(dev, bam.read_fasta(fa)))) == text
        # the flag holds for one run: the next one on the handle writes the reference form again
        out = str(tmp_path / "again.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        one.realign_sequential(ctx, nf, regions, out, batch_reads=5, r=30, out_format="bam")
        assert record_stream(out) == nb.format_bam(idx, finals, st) != want
        # ---- 3. coded members: the same record stream
        for compress in ("huffman", "match"):
            assert record_stream(run(f"{compress}.bam", batch_reads=5, compress=compress)) == want
            check_index(str(tmp_path / f"{compress}.bam"), str(tmp_path / f"{compress}.bam.bai"))
        one.close(); nb.close(); nf.close()
    finally:
        cfg.args = old


# ---- 4. a read of more than 65 535 operations ---------------------------------------------------------------------------------
def test_ultra_long_read_full(ctx, tmp_path):
    references, refs, records = lc.ultra_long_read()
    for k, r in enumerate(records):
        r["tags"] = b"RGZlong\0" + b"NMi" + bytes(4) + b"MLBC" + (1000 + k).to_bytes(4, "little") + bytes(1000 + k)
        r.update(next_ref_id=0, next_pos=17 + k, tlen=-5)
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
        want = nb.format_bam_full(nf, idx, finals, st)
        out = str(tmp_path / "u.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        nb.realign_file(ctx, nf, idx, out, batch_reads=4, r=10, out_format="bam", bai=out + ".bai", records="full")
        assert record_stream(out) == want
        check_index(out, out + ".bai")
        recs = [r for _, r in split_records(want)]
        f, _, words, _, tags = fc.parse_full(recs[1])
        assert f[5] == 2 and words == [len(records[1]["seq"]) << 4 | 4, 6 * 36000 << 4 | 3] and (f[8], f[9], f[10]) == (0, 18, -5)
        kept = b"RGZlong\0" + b"MLBC" + (1001).to_bytes(4, "little") + bytes(1001) + b"HPC\x02"       # (the stale NM between them is gone)
        nm_len = {b"C": 4, b"S": 5, b"I": 7}[tags[len(kept) + 2:len(kept) + 3]]
        assert tags.startswith(kept + b"NM") and tags[len(kept) + nm_len:][:8] == b"CGBI" + n_ops[1].to_bytes(4, "little")
        assert len(tags) == len(kept) + nm_len + 8 + 4 * n_ops[1]
        nb.close(); nf.close()
    finally:
        cfg.args = old


# ---- 5. the CLI ---------------------------------------------------------------------------------------------------------------
def realign_cli(args, timeout, env=None, launcher=(), ok=True):
    cmd = [sys.executable] + list(launcher) + ["-m", "npore_amd.realign"] + args
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=timeout, env=env)
    assert (out.returncode == 0) == ok, out.stdout[-2000:] + out.stderr[-3000:]
    return out


def test_cli_full_records(tmp_path):
    common = ["--bam", os.path.join(DATA, "reads.bam"), "--ref", os.path.join(DATA, "ref.fasta"), "--out_format", "bam", "--records", "full"]
    p1, p2 = str(tmp_path / "one"), str(tmp_path / "ix")
    realign_cli(common + ["--out_prefix", p1], 300)
    realign_cli(common + ["--out_prefix", p2], 300, env=dict(os.environ, NPORE_BAM_ONE_PASS="0"))
    refs = bam.read_fasta(os.path.join(DATA, "ref.fasta"))
    gold = [l for l in open(os.path.join(DATA, "npore_realigned.sam")) if not l.startswith("@")]
    assert fc.without_clips(decoded_lines(p1 + ".bam", refs)) == gold and len(gold) == 10
    assert record_stream(p1 + ".bam") == record_stream(p2 + ".bam")
    # ... and they are the host twin's FULL records of the golden finals
    nb, nf = bam.NativeBam(os.path.join(DATA, "reads.bam"), stream=False), bam.NativeFasta(os.path.join(DATA, "ref.fasta"))
    idx = nb.select([(n, 0, l - 1) for n, l in zip(nb.references, nb.lengths)])
    final_of = {l.split("\t")[0]: l.split("\t")[5] for l in gold}
    names = [r[36:36 + r[12] - 1].decode() for r in fc.input_records(os.path.join(DATA, "reads.bam"))]
    assert record_stream(p1 + ".bam") == nb.format_bam_full(nf, idx, [final_of[names[k]] for k in idx], np.zeros(len(idx), np.int32))
    nb.close(); nf.close()
    for p in (p1, p2):
        members(p + ".bam")
        check_index(p + ".bam", p + ".bam.bai")
    # the two error exits: one line each
    for extra, word in ((["--out_format", "sam"], "--out_format bam"), (["--python_io"], "--python_io")):
        out = realign_cli(common + ["--out_prefix", str(tmp_path / "bad")] + extra, 120, ok=False)
        assert out.returncode == 1
        errors = [l for l in out.stdout.splitlines() if l.startswith("ERROR")]
        assert len(errors) == 1 and "--records full" in errors[0] and word in errors[0], out.stdout
        assert not os.path.exists(str(tmp_path / "bad.bam")) and not os.path.exists(str(tmp_path / "bad.sam"))


# ---- 6. two ranks ---------------------------------------------------------------------------------------------------------------
def test_two_ranks_full_records(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import bench_realign
    bp, fa, clen = bench_realign.build_inputs(str(tmp_path), 200, 0, 1500, 31, procs=2, tags=True)
    bam.write_bai(bp)
    common = ["--bam", bp, "--ref", fa, "--out_format", "bam", "--records", "full", "--batch_reads", "40"]
    b1, b2 = str(tmp_path / "single"), str(tmp_path / "two")
    realign_cli(common + ["--out_prefix", b1], 300)
    out = realign_cli(common + ["--out_prefix", b2], 600,
                      launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                "--master-port", str(29600 + os.getpid() % 100)])
    assert "no .bai index" not in out.stdout
    one = record_stream(b1 + ".bam")
    assert record_stream(b2 + ".bam") == one and len(split_records(one)) == 200
    assert all(b"RGZbench\0MLBC" in r and r[-4:-1] in (b"NMC",) or b"NMS" in r[-5:] for _, r in split_records(one))
    for p in (b1, b2):
        members(p + ".bam")
        check_index(p + ".bam", p + ".bam.bai")
    assert not os.path.exists(b2 + ".part0.bam") and not os.path.exists(b2 + ".part1.bam.bai")
