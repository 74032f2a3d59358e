"""The ranks' shares and the default regions under a stale or foreign .bai, with the device behind them: the file and the
indexes of tests/bai_trust_cases.py, realigned at r = 30.  Either every rank refuses its share before anything is written,
or the ranks' parts one after the other are the single process's output, byte for byte; the tool under
torch.distributed.run with a stale index beside the BAM writes what one process writes with no index; an index that
declares a contig with reads empty ends the run with its name.  (The decision itself, over the whole family and at four
worlds: tests/test_bai_trust.py, on the CPU.)"""
import argparse
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bai_trust_cases as btc
from conftest import REPO
from npore_amd import aln, bam, cfg

pytestmark = pytest.mark.gpu
WORLD = 3
REGIONS = [("a", 0, 299_999), ("b", 0, 299_999)]


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


class Files:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, ctx):
    """the 400-read file, a FASTA for its two contigs, the index family as files in a directory of their own, and the
    single process's SAM (one pass, no index)"""
    tmp = tmp_path_factory.mktemp("gpu_bai_trust")
    f = Files()
    f.tmp = tmp
    f.bp, f.recs = btc.share_test_bam(tmp)
    f.raw = open(f.bp, "rb").read()
    f.stream = btc.Stream(f.raw)
    # the contigs: random bases with every read's own laid over its place, in file order (a later read overwrites what
    # it overlaps: each read agrees with the reference where no later one lies, and disagrees elsewhere)
    rng = np.random.default_rng(5)
    contigs = [rng.choice(list("ACGT"), ln) for _, ln in btc.REFS]
    for r in f.recs:
        contigs[r["ref_id"]][r["pos"]:r["pos"] + len(r["seq"])] = list(r["seq"])
    f.fa = str(tmp / "ref.fa")
    with open(f.fa, "w") as fh:
        for (name, ln), ctg in zip(btc.REFS, contigs):
            seq = "".join(ctg)
            fh.write(f">{name}\n" + "\n".join(seq[q:q + 60] for q in range(0, ln, 60)) + "\n")
    f.bytes = btc.index_family(tmp, f.bp, f.recs)
    os.mkdir(tmp / "idx")
    f.file = {}
    for name, raw in f.bytes.items():
        f.file[name] = str(tmp / "idx" / (name.replace("=", "_") + ".bai"))
        with open(f.file[name], "wb") as fh:
            fh.write(raw)
    assert bam.NativeBam.bai_path(f.bp) is None
    f.nf = bam.NativeFasta(f.fa)
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=REGIONS, max_reads=0)
    try:
        f.whole = str(tmp / "whole.sam")
        one = bam.NativeBam(f.bp, one_pass=True, share=False)
        n, bad, _ = one.realign_sequential(ctx, f.nf, REGIONS, f.whole, batch_reads=37, r=30)
        one.close()
        assert n == 400 and not bad
        yield f
    finally:
        cfg.args = old
        f.nf.close()


def _ranks(ctx, f, name, tag, **out_kw):
    """Every rank of WORLD on a one-pass handle of its own: set_share with the index `name`, then its part.  Returns
    (ranks that refused, [part path of the ranks that did not], reads written)."""
    refused, parts, total = [], [], 0
    for rank in range(WORLD):
        h = bam.NativeBam(f.bp, one_pass=True, share=False)
        try:
            try:
                has = h.set_share(rank, WORLD, bai=f.file[name])[0]
            except bam.OnePassUnsupported as e:
                assert f.file[name] in str(e)                    # the message names the index
                refused.append(rank)
                continue
            assert has == 1
            out = str(f.tmp / f"{tag}_r{rank}")
            kw = dict(out_kw, bai=out + ".bai") if out_kw else {}
            open(out, "wb").close()                              # (a rank's part begins empty: realign.py does the same)
            n, bad, _ = h.realign_sequential(ctx, f.nf, REGIONS, out, batch_reads=37, r=30, **kw)
            assert not bad
            parts.append(out)
            total += n
        finally:
            h.close()
    return refused, parts, total


@pytest.mark.parametrize("name,accepts", [("true", True), ("stale-first-250", True), ("stale-every-other", False), ("plus-7000", False)])
def test_ranks_refuse_together_or_tile(ctx, files, name, accepts):
    """Three ranks, each with a one-pass handle of its own, set_share and realign_sequential(batch_reads=37): all three
    refuse before anything is written, or the parts concatenated are byte for byte the single process's SAM -- and which
    of the two is expected()'s answer."""
    f = files
    assert (btc.expected(f.raw, f.bytes[name], WORLD, f.stream) != btc.REFUSE) == accepts
    refused, parts, total = _ranks(ctx, f, name, "sam_" + name)
    if refused:
        assert refused == list(range(WORLD)) and not parts and not accepts
        return
    assert accepts and total == 400 and len(parts) == WORLD
    assert b"".join(open(p, "rb").read() for p in parts) == open(f.whole, "rb").read()


def test_ranks_refuse_together_or_tile_full_bam_device_inflate(ctx, files):
    """The same with whole BAM records (out_format="bam", records="full") and the input inflated on the device, for the index
    that accepts and one that refuses: the parts' record streams one after the other are the single process's."""
    f = files
    kw = dict(out_format="bam", records="full", eof=False)
    ctx.set("device_inflate", True)
    try:
        whole = str(f.tmp / "whole_full.bam")
        open(whole, "wb").close()
        one =bam.NativeBam(f.bp, one_pass=True, share=False)
        n, bad, _ = one.realign_sequential(ctx, f.nf, REGIONS, whole, batch_reads=37, r=30, bai=whole + ".bai", **kw)
        assert n == 400 and not bad and one.inflate_info()[7] == 1 and one.inflate_info()[0] > 0
        one.close()
        refused, parts, total = _ranks(ctx, f, "true", "bam_true", **kw)
        assert not refused and total == 400 and len(parts) == WORLD
        stream = bam._bgzf_decompress(whole)
        assert len(stream) > 200_000 and b"".join(bam._bgzf_decompress(p) for p in parts) == stream
        refused, parts, total = _ranks(ctx, f, "plus-7000", "bam_plus7000", **kw)
        assert refused == list(range(WORLD)) and not parts
    finally:
        ctx.set("device_inflate", False)


def _sam_records(path):
    return [l for l in open(path) if not l.startswith("@")]


def _tool(args, nproc=0, port=0):
    cmd = [sys.executable]
    if nproc:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1", "--master-port", str(port)]
    return subprocess.run(cmd + ["-m", "npore_amd.realign"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)


def test_tool_three_ranks_with_a_stale_index(files, tmp_path):
    """`realign` under torch.distributed.run, three ranks on the one card, the index of every other record beside the BAM
    (at its parent, two ranks fell back and dealt themselves a third of ALL reads each, the third walked an empty stretch,
    and a third of the reads was missing from the merged output without an error): every rank says that it takes the
    indexed reader, and the records are those of one process run with no index, in order.  (BAM out: there the indexed
    reader deals contiguous shares, so the merged parts are in file order; its SAM parts of a resident file are dealt
    round-robin, and their order is arbitrary as the reference's is.)"""
    f = files
    bp = str(tmp_path / "s.bam")
    shutil.copy(f.bp, bp)
    one = _tool(["--bam", bp, "--ref", f.fa, "--out_prefix", str(tmp_path / "one"), "--out_format", "bam"])
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-3000:]
    def record_stream(path):                                     # (the header's text names the output file)
        s = btc.Stream(open(path, "rb").read())
        assert len(s.starts) == 400
        return s.data[s.first_record:]

    want = record_stream(str(tmp_path / "one.bam"))
    with open(bp + ".bai", "wb") as fh:
        fh.write(f.bytes["stale-every-other"])
    out = _tool(["--bam", bp, "--ref", f.fa, "--out_prefix", str(tmp_path / "three"), "--out_format", "bam"], nproc=3, port=29500 + os.getpid() % 100)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    said = [l for l in out.stdout.splitlines() if "taking the indexed reader" in l]
    assert len(said) == 3 and all(bp + ".bai" in l for l in said), out.stdout[-3000:]
    assert record_stream(str(tmp_path / "three.bam")) == want


def test_tool_with_an_index_that_declares_a_contig_empty(files, tmp_path):
    """One process, the index of records 0 - 299 (contig a only) beside the BAM: `realign` exits non-zero and names the
    index -- the default regions made from it would leave contig b's 100 reads out; with the index removed it writes all
    400 reads."""
    f = files
    bp = str(tmp_path / "s.bam")
    shutil.copy(f.bp, bp)
    with open(bp + ".bai", "wb") as fh:
        fh.write(f.bytes["stale-contig-a"])
    out = _tool(["--bam", bp, "--ref", f.fa, "--out_prefix", str(tmp_path / "stale")])
    assert out.returncode != 0, out.stdout[-2000:]
    errors = [l for l in out.stdout.splitlines() if l.startswith("ERROR")]
    assert len(errors) == 1 and bp + ".bai" in errors[0] and "stale" in errors[0], out.stdout[-2000:] + out.stderr[-2000:]
    os.remove(bp + ".bai")
    out = _tool(["--bam", bp, "--ref", f.fa, "--out_prefix", str(tmp_path / "fresh")])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert _sam_records(str(tmp_path / "fresh.sam")) == _sam_records(f.whole)
