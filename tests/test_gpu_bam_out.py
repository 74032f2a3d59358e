"""BAM output (--out_format bam) on the GPU: the records built by emit_bam_records_kernel (csrc/bam_emit_kernels.hpp) in
the default file pipeline against the host twin npore_bam_format_bam and against the SAM route's text, through the CLI,
through the library's entry points, at full batch size, with two ranks, and back in as input.  The format is stated in
csrc/bam_reader.hpp ("BAM out: records and file, stated once"); the decoder is bam._bgzf_decompress + bam.BamFile.
Every child process runs under its own time limit.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

from npore_amd import aln, bam, cfg, synth
from conftest import GOLDEN, REPO
from test_bam_out import Hdr, check_index, decoded_lines, header_len, members, split_records

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, "data")


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


def realign_cli(args, timeout, env=None, launcher=()):
    cmd = [sys.executable] + list(launcher) + ["-m", "npore_amd.realign"] + args
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=timeout, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout


def record_stream(path):
    data = bam._bgzf_decompress(path)
    return data[header_len(data):]


def header_lines(path):
    return [l for l in bam.BamFile(path).text.splitlines() if not l.startswith("@PG")]


def file_behind_header(path):
    """The file's bytes from the member that holds the first record to the end (the header lies in members of its own)."""
    mem = members(path)
    data = b"".join(m[1] for m in mem)
    h, u = header_len(data), 0
    for off, payload, _ in mem:
        if u == h:
            return open(path, "rb").read()[off:]
        u += len(payload)
    raise AssertionError("the header does not end at a member boundary")


def index_relative(path):
    """The .bai with its virtual offsets counted from the first record's member (0 stays 0: no record)."""
    from test_bam_out import parse_bai
    shift = (os.path.getsize(path) - len(file_behind_header(path))) << 16
    return [({b: [(c0 - shift, c1 - shift) for c0, c1 in ch] for b, ch in bins.items()}, [v - shift if v else 0 for v in lin])
            for bins, lin in parse_bai(path + ".bai")]


def sam_records(path):
    return [l for l in open(path) if not l.startswith("@")]


# ---- 6. the CLI on the golden BAM -------------------------------------------------------------------------------------
def test_cli_golden_bam(tmp_path):
    common = ["--bam", os.path.join(DATA, "reads.bam"), "--ref", os.path.join(DATA, "ref.fasta"), "--out_format", "bam"]
    p1, p2, p3 = (str(tmp_path / n) for n in ("one", "ix", "py"))
    realign_cli(common + ["--out_prefix", p1], 300)
    realign_cli(common + ["--out_prefix", p2], 300, env=dict(os.environ, NPORE_BAM_ONE_PASS="0"))
    realign_cli(common + ["--out_prefix", p3, "--python_io"], 300)
    refs = bam.read_fasta(os.path.join(DATA, "ref.fasta"))
    gold = sam_records(os.path.join(DATA, "npore_realigned.sam"))
    assert decoded_lines(p1 + ".bam", refs) == gold and len(gold) == 10
    assert record_stream(p1 + ".bam") == record_stream(p2 + ".bam") == record_stream(p3 + ".bam")
    assert header_lines(p1 + ".bam") == header_lines(p2 + ".bam") == header_lines(p3 + ".bam")
    assert header_lines(p1 + ".bam") == [l.rstrip("\n") for l in open(os.path.join(DATA, "npore_realigned.sam")) if l.startswith("@") and not l.startswith("@PG")]
    for p in (p1, p2, p3):
        members(p + ".bam")
        check_index(p + ".bam", p + ".bam.bai")
    assert not os.path.exists(p1 + ".sam")


# ---- 7. device against host on a synthetic BAM ----------------------------------------------------------------------------
def clipped_bam(tmp_path):
    """Reads with soft clips of even and odd length, hard clips outside them, N / ambiguity codes, both strands, reads
    without qualities, HP tags of every integer width and none, and one read whose CIGAR disagrees with its sequence."""
    from test_bam_out import make_bam
    rng = np.random.default_rng(5)
    refs, seqs, cigs = synth.make_batch(77, 24, ref_len=1500, p_np=0.1)
    dec = lambda a: "".join("NACGT"[x] for x in a)
    contig, recs = [], []
    hps = [None, 0, 2, 255, 256, -1, -129, 70000]
    for k, (rf, sq, cg) in enumerate(zip(refs, seqs, cigs)):
        pos = len(contig) + 20
        contig += list("ACGT"[x] for x in rng.integers(0, 4, 20)) + list(dec(rf))
        cg = cg.decode() if isinstance(cg, (bytes, bytearray)) else cg if isinstance(cg, str) else "".join(chr(x) for x in cg)
        runs, last, cnt = [], None, 0
        for ch in cg:
            if ch == last:
                cnt += 1
            else:
                if last is not None:
                    runs.append(("MIDNSHP=XB".index(last), cnt))
                last, cnt = ch, 1
        runs.append(("MIDNSHP=XB".index(last), cnt))
        lead, trail = (0, 3, 4, 1)[k % 4], (2 if k % 3 == 0 else 0)
        cig = ([(4, lead)] if lead else []) + runs + ([(4, trail)] if trail else [])
        if k % 6 == 2:
            cig = [(5, 4)] + cig
        if k % 4 == 3:
            cig = cig + [(5, 7)]
        body = dec(sq)
        if k % 7 == 3:
            body = body[:11] + "N" + body[12:40] + "R" + body[41:]
        n = lead + len(sq) + trail
        recs.append(dict(name=f"r{k}", flag=16 if k % 4 == 1 else 0, ref_id=0, pos=pos, mapq=k, cigar=cig, seq="A" * lead + body + "C" * trail,
                         qual=None if k % 5 == 0 else bytes(rng.integers(0, 60, n).tolist()), hp=hps[k % len(hps)]))
    recs[7]["cigar"] = recs[7]["cigar"] + [(0, 5)]              # lengths now disagree: refused, not written
    contig = "".join(contig) + "ACGT" * 10
    (tmp_path / "c.fa").write_text(">ctg\n" + contig + "\n")
    make_bam(str(tmp_path / "s.bam"), [("ctg", len(contig))], recs)
    return str(tmp_path / "s.bam"), str(tmp_path / "c.fa"), len(contig), len(recs)


def test_device_records_equal_host_twin(ctx, tmp_path):
    bp, fa, clen, n = clipped_bam(tmp_path)
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
        assert ((st & 32) != 0).sum() == 1 and text.count("\n") == n - 1
        finals, it = [], iter(text.splitlines())
        for k in range(n):
            finals.append("" if st[k] & 32 else next(it).split("\t")[5])
        want = str(tmp_path / "want.bam")
        bam.create_bam_header(want, Hdr(nb.references, nb.lengths))
        nb.write_file(idx, finals, st, want, batch_reads=5, bai=want + ".bai")
        want_bytes = open(want, "rb").read()
        assert record_stream(want) == nb.format_bam(idx, finals, st)

        def run(name, **kw):
            out = str(tmp_path / name)
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            stb = nb.realign_file(ctx, nf, idx, out, r=30, out_format="bam", bai=out + ".bai", **kw)
            assert np.array_equal(stb, st), name
            assert open(out, "rb").read() == want_bytes, name
            assert open(out + ".bai", "rb").read() == open(want + ".bai", "rb").read(), name
            return out

        dev = run("dev.bam", batch_reads=5)
        assert nb.output_info()["records"] == n - 1 and nb.file_timing()["wall_ms"] > 0
        run("dev_one_batch.bam", batch_reads=1000)
        for key in ("device_pack", "device_glue"):
            ctx.set(key, 0)
            run(f"no_{key}.bam", batch_reads=5)
        ctx.set("device_pack", 1)
        ctx.set("device_glue", 1)
        ctx.set("tb_budget_mb", 2)                           # every batch in several groups: each places its records behind the one before
        try:
            run("groups.bam", batch_reads=12)
        finally:
            ctx.set("tb_budget_mb", 0)
        # the decoded records are the SAM route's text, byte for byte
        assert "".join(decoded_lines(dev, bam.read_fasta(fa))) == text
        check_index(dev, dev + ".bai")
        # one pass over the file writes the same; the mode holds for one run: the next one writes text again
        one = bam.NativeBam(bp, one_pass=True)
        out = str(tmp_path / "onepass.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        n5, bad5, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=5, r=30, out_format="bam", bai=out + ".bai")
        assert n5 == n and bad5 == [(7, 32)] and open(out, "rb").read() == want_bytes
        again = tmp_path / "again.sam"
        one.realign_sequential(ctx, nf, regions, str(again), batch_reads=5, r=30)
        assert again.read_text() == text
        one.close(); nb.close(); nf.close()
    finally:
        cfg.args = old


# ---- 8. - 10. full-size batches, two ranks, round trip ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_inputs(tmp_path_factory):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import bench_realign
    tmp = tmp_path_factory.mktemp("bam_out_big")
    bp, fa, clen = bench_realign.build_inputs(str(tmp), 6000, 0, 10000, 29)
    bam.write_bai(bp)
    return tmp, bp, fa, clen


def test_full_size_batches_ranks_and_round_trip(big_inputs):
    tmp, bp, fa, clen = big_inputs
    common = ["--bam", bp, "--ref", fa]
    sam, b1, b2, b3 = (str(tmp / n) for n in ("s", "b4000", "b3000", "two"))
    realign_cli(common + ["--out_prefix", sam], 600)
    realign_cli(common + ["--out_prefix", b1, "--out_format", "bam"], 600)
    realign_cli(common + ["--out_prefix", b2, "--out_format", "bam", "--batch_reads", "3000"], 600)
    # 8. decoded BAM == the SAM route's file; the index holds; the file does not depend on the batches
    want = sam_records(sam + ".sam")
    assert len(want) == 6000
    assert decoded_lines(b1 + ".bam", bam.NativeFastaSeqs(fa)) == want
    # (the header's @PG line holds the command line, --batch_reads and --out_prefix with it, as the SAM file's does: the
    # files are compared from the first record's member on, byte for byte, and their headers apart from @PG)
    assert file_behind_header(b1 + ".bam") == file_behind_header(b2 + ".bam")
    assert header_lines(b1 + ".bam") == header_lines(b2 + ".bam")
    assert index_relative(b1 + ".bam") == index_relative(b2 + ".bam")
    members(b1 + ".bam")
    check_index(b1 + ".bam", b1 + ".bam.bai")
    # 9. two ranks on the one card: the same stream, an index that holds
    out = realign_cli(common + ["--out_prefix", b3, "--out_format", "bam"], 900,
                      launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                "--master-port", str(29400 + os.getpid() % 100)])
    assert "no .bai index" not in out
    assert record_stream(b3 + ".bam") == record_stream(b1 + ".bam")
    members(b3 + ".bam")
    check_index(b3 + ".bam", b3 + ".bam.bai")
    assert not os.path.exists(b3 + ".part0.bam") and not os.path.exists(b3 + ".part1.bam.bai")
    # 10. the written BAM and its index back in: one pass, then two shares cut from its own index
    names = [l.split("\t")[0] for l in want]
    r1, r2 = str(tmp / "back1"), str(tmp / "back2")
    realign_cli(["--bam", b1 + ".bam", "--ref", fa, "--out_prefix", r1], 600)
    assert [l.split("\t")[0] for l in sam_records(r1 + ".sam")] == names
    out = realign_cli(["--bam", b1 + ".bam", "--ref", fa, "--out_prefix", r2], 900,
                      launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                "--master-port", str(29500 + os.getpid() % 100)])
    assert "indexed reader" not in out
    assert [l.split("\t")[0] for l in sam_records(r2 + ".sam")] == names
