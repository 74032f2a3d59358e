"""BAM out with Huffman-coded BGZF members, the device side (csrc/bam_deflate_kernels.hpp): the three kernels against the
host twin at small shapes, the file pipeline in every variant against npore_bam_write_file, the command line with one
process and with two ranks on the one card."""
import argparse
import os
import sys

import numpy as np
import pytest

from npore_amd import _lib, aln, bam, cfg
from conftest import GOLDEN, REPO
from test_bam_out import Hdr, check_index, decoded_lines, members
from test_bam_deflate import KINDS, content, host_member
from test_gpu_bam_out import realign_cli, record_stream, sam_records

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, "data")
P = 65280


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


def device_members(ctx, data, phase):
    """(members, head fragment, tail fragment, stream position behind the call) of npore_debug_deflate_device."""
    lib = _lib.load()
    n = len(data)
    cap = (n // P + 1) * (P + 31)
    src = np.frombuffer(data, np.uint8)
    out, sizes = np.zeros(cap, np.uint8), np.zeros(n // P + 1, np.uint32)
    head, tail = np.full(P, 0xEE, np.uint8), np.full(P, 0xEE, np.uint8)
    info = np.zeros(5, np.int64)
    rc = lib.npore_debug_deflate_device(ctx.handle, src.ctypes.data, n, phase, out.ctypes.data, cap, sizes.ctypes.data, len(sizes),
                                        head.ctypes.data, tail.ctypes.data, info.ctypes.data)
    assert rc == 0, _lib.last_error()
    nm, comp, hd, tl, pos = (int(x) for x in info)
    assert int(sizes[:nm].sum()) == comp
    mem, at = [], 0
    for k in range(nm):
        mem.append(out[at:at + int(sizes[k])].tobytes())
        at += int(sizes[k])
    return mem, head[:hd].tobytes(), tail[:tl].tobytes(), pos


def mixed_buffer(n):
    """n bytes: stretches of the CPU test's contents one after the other, so that the members of a buffer differ in kind
    (one value, two values, the Fibonacci histogram that needs the length limit, all 256 values -- stored --, real records)."""
    parts = []
    for k in range(n // P + 2):
        parts.append(content(KINDS[k % len(KINDS)], P))
    return b"".join(parts)[:n]


# ---- 1. the kernels against the host twin ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,phase", [(3 * P + 1000, 0), (3 * P + 1000, 1), (3 * P + 1000, P - 1), (3 * P + 1000, 5 * P + 777),
                                     (1000, 0), (1000, 1), (1000, P - 1000), (1000, P - 999), (P, 0), (P, 17), (5 * P, 0)])
def test_kernels_equal_host_twin(ctx, n, phase):
    data = mixed_buffer(n)
    mem, head, tail, pos = device_members(ctx, data, phase)
    first = (P - phase % P) % P
    if n < first:
        want_head, n_mem, want_tail = n, 0, 0
    else:
        want_head, n_mem = first, (n - first) // P
        want_tail = n - first - n_mem * P
    assert (len(head), len(mem), len(tail)) == (want_head, n_mem, want_tail)
    assert head == data[:want_head] and tail == data[n - want_tail:]
    assert pos == phase + n
    for k, m in enumerate(mem):
        payload = data[want_head + k * P:want_head + (k + 1) * P]
        assert m == host_member(payload), (k, len(m))


@pytest.mark.parametrize("kind", KINDS)
def test_kernels_every_content(ctx, kind):
    """Two members of one kind, at an odd phase: every place in the output has every alignment."""
    payload = content(kind, P)
    data = payload[-3:] + payload + payload + payload[:5]
    mem, head, tail, _ = device_members(ctx, data, P - 3)
    assert (head, tail) == (payload[-3:], payload[:5])
    want = host_member(payload)
    assert mem == [want, want]
    assert (len(want) == P + 31) == (kind == "uniform")


# ---- 2. the file pipeline ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads_10kb(tmp_path_factory):
    """200 reads of 10 kb on one contig (the benchmark's generator): about 3 MB of records, 46 members."""
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import bench_realign
    tmp = tmp_path_factory.mktemp("bam_deflate")
    bp, fa, clen = bench_realign.build_inputs(str(tmp), 200, 0, 10000, 31, procs=4)
    bam.write_bai(bp)
    return bp, fa, clen


def test_file_pipeline(ctx, tmp_path, reads_10kb):
    src, fa, clen = reads_10kb
    n = 60                                                  # the first 60 reads: about 14 members
    regions = [("ctg", 0, clen - 1)]
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=regions, max_reads=0)
    try:
        nb, nf = bam.NativeBam(src), bam.NativeFasta(fa)
        idx = nb.select(regions)[:n]
        assert len(idx) == n
        sam = tmp_path / "route.sam"
        st = nb.realign_file(ctx, nf, idx, str(sam), batch_reads=17, r=30)
        it = iter(sam_records(str(sam)))
        finals = ["" if s_ & 32 else next(it).split("\t")[5] for s_ in st]
        want = str(tmp_path / "want.bam")
        bam.create_bam_header(want, Hdr(nb.references, nb.lengths))
        nb.write_file(idx, finals, st, want, batch_reads=9, bai=want + ".bai", compress="huffman")
        want_bytes, want_bai = open(want, "rb").read(), open(want + ".bai", "rb").read()
        mem = members(want)
        assert sum(1 for m in mem if len(m[1]) == P) >= 8 and not all(m[2] for m in mem[:-1])

        def run(name, **kw):
            out = str(tmp_path / name)
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            stb = nb.realign_file(ctx, nf, idx, out, r=30, out_format="bam", bai=out + ".bai", compress="huffman", **kw)
            assert np.array_equal(stb, st), name
            assert open(out, "rb").read() == want_bytes, name
            assert open(out + ".bai", "rb").read() == want_bai, name
            return out

        dev = run("b5.bam", batch_reads=5)
        run("b17.bam", batch_reads=17)
        run("b1000.bam", batch_reads=1000)
        ctx.set("tb_budget_mb", 2)                          # several groups per batch: the kernels follow the last of them
        try:
            run("groups.bam", batch_reads=17)
        finally:
            ctx.set("tb_budget_mb", 0)
        for key in ("device_pack", "device_glue"):
            ctx.set(key, 0)
            run(f"no_{key}.bam", batch_reads=17)
        ctx.set("device_pack", 1)
        ctx.set("device_glue", 1)
        check_index(dev, dev + ".bai")
        one = bam.NativeBam(src, one_pass=True)
        out = str(tmp_path / "onepass.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        n1, bad, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=17, max_reads=n, r=30, out_format="bam", bai=out + ".bai",
                                            compress="huffman")
        assert n1 == n and [b for b, _ in bad] == np.nonzero(st)[0].tolist() and open(out, "rb").read() == want_bytes and open(out + ".bai", "rb").read() == want_bai
        # the stored mode beside it: the same payloads, and the mode holds for one run
        stored = str(tmp_path / "stored.bam")
        bam.create_bam_header(stored, Hdr(nb.references, nb.lengths))
        nb.realign_file(ctx, nf, idx, stored, batch_reads=17, r=30, out_format="bam", bai=stored + ".bai")
        assert record_stream(stored) == record_stream(want) and all(m[2] for m in members(stored)[:-1])
        one.close(); nb.close(); nf.close()
    finally:
        cfg.args = old


# ---- 3. the command line ------------------------------------------------------------------------------------------------------
def test_cli_golden(tmp_path):
    common = ["--bam", os.path.join(DATA, "reads.bam"), "--ref", os.path.join(DATA, "ref.fasta"), "--out_format", "bam", "--bam_compress", "huffman"]
    p1, p3 = str(tmp_path / "one"), str(tmp_path / "py")
    realign_cli(common + ["--out_prefix", p1], 300)
    realign_cli(common + ["--out_prefix", p3, "--python_io"], 300)
    refs = bam.read_fasta(os.path.join(DATA, "ref.fasta"))
    gold = sam_records(os.path.join(DATA, "npore_realigned.sam"))
    assert decoded_lines(p1 + ".bam", refs) == gold and len(gold) == 10
    assert record_stream(p1 + ".bam") == record_stream(p3 + ".bam")
    for p in (p1, p3):
        mem = members(p + ".bam")
        assert not mem[-2][2]                                   # the records' member is Huffman-coded
        check_index(p + ".bam", p + ".bam.bai")
    import subprocess
    out = subprocess.run([sys.executable, "-m", "npore_amd.realign", "--bam", os.path.join(DATA, "reads.bam"), "--ref",
                          os.path.join(DATA, "ref.fasta"), "--bam_compress", "huffman", "--out_prefix", str(tmp_path / "no")],
                         cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--bam_compress needs --out_format bam" in out.stdout


def test_cli_two_ranks(tmp_path, reads_10kb):
    bp, fa, _clen = reads_10kb
    common = ["--bam", bp, "--ref", fa, "--out_format", "bam", "--bam_compress", "huffman", "--batch_reads", "60"]
    b1, b2 = str(tmp_path / "one"), str(tmp_path / "two")
    realign_cli(common + ["--out_prefix", b1], 300)
    out = realign_cli(common + ["--out_prefix", b2], 600,
                      launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                "--master-port", str(29600 + os.getpid() % 100)])
    assert "no .bai index" not in out
    assert record_stream(b2 + ".bam") == record_stream(b1 + ".bam")
    for b in (b1, b2):
        mem = members(b + ".bam")
        assert sum(1 for m in mem if not m[2]) >= 40                # (200 reads of 10 kb: about 46 members, Huffman-coded)
        check_index(b + ".bam", b + ".bam.bai")
    assert not any(os.path.exists(f"{b2}.part{k}.bam{ext}") for k in range(2) for ext in ("", ".bai"))
