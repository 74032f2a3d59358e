"""BAM out with matches in the BGZF members, the device side (csrc/bam_deflate_kernels.hpp plan_match_kernel /
emit_match_kernel): the kernels against the host twin at small shapes and on every content, the file pipeline in every
variant against npore_bam_write_file, the command line with one process and with two ranks on the one card, and the one
size condition: on records with repeats the file is smaller than the Huffman mode's, member by member never larger."""
import argparse
import os
import struct
import sys

import numpy as np
import pytest

from npore_amd import _lib, aln, bam, cfg
from conftest import GOLDEN, REPO
from test_bam_out import Hdr, check_index, decoded_lines, members
from test_bam_deflate import KINDS, content, host_member
from test_bam_match import ALL, any_content, host_member_mode
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


def device_members(ctx, data, phase, mode=2):
    """(members, head fragment, tail fragment, stream position behind the call) of npore_debug_deflate_device_mode."""
    lib = _lib.load()
    n = len(data)
    cap = (n // P + 1) * (P + 31)
    src = np.frombuffer(data, np.uint8)
    out, sizes = np.zeros(cap, np.uint8), np.zeros(n // P + 1, np.uint32)
    head, tail = np.full(P, 0xEE, np.uint8), np.full(P, 0xEE, np.uint8)
    info = np.zeros(5, np.int64)
    rc = lib.npore_debug_deflate_device_mode(ctx.handle, src.ctypes.data, n, phase, out.ctypes.data, cap, sizes.ctypes.data, len(sizes),
                                             head.ctypes.data, tail.ctypes.data, info.ctypes.data, mode)
    assert rc == 0, _lib.last_error()
    nm, comp, hd, tl, pos = (int(x) for x in info)
    assert int(sizes[:nm].sum()) == comp
    mem, at = [], 0
    for k in range(nm):
        mem.append(out[at:at + int(sizes[k])].tobytes())
        at += int(sizes[k])
    return mem, head[:hd].tobytes(), tail[:tl].tobytes(), pos


def mixed_buffer(n):
    """n bytes: stretches of every content one after the other, so that neighbouring members differ in form (match blocks,
    Huffman blocks, stored ones)."""
    parts = []
    for k in range(n // P + 2):
        kind, new = ALL[(5 * k) % len(ALL)]
        parts.append(any_content(kind, new, P))
    return b"".join(parts)[:n]


_want = {}


def want_member(payload):
    if payload not in _want:
        _want[payload] = host_member_mode(payload, 2)
    return _want[payload]


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
        assert m == want_member(payload), (k, len(m))


@pytest.mark.parametrize("kind,new", ALL)
def test_kernels_every_content(ctx, kind, new):
    """Two members of one kind, at an odd phase: every place in the output has every alignment."""
    payload = any_content(kind, new, P)
    data = payload[-3:] + payload + payload + payload[:5]
    mem, head, tail, _ = device_members(ctx, data, P - 3)
    assert (head, tail) == (payload[-3:], payload[:5])
    want = want_member(payload)
    assert mem == [want, want]
    assert len(want) <= len(host_member(payload))
    if kind in ("uniform", "nomatch"):
        assert len(want) == P + 31


def test_huffman_mode_unchanged(ctx):
    """The old entry and mode 1 of the new one give the Huffman mode's members after a run with matches."""
    data = mixed_buffer(2 * P + 100)
    device_members(ctx, data, 50)
    lib = _lib.load()
    src, out, sizes = np.frombuffer(data, np.uint8), np.zeros(3 * (P + 31), np.uint8), np.zeros(3, np.uint32)
    head, tail, info = np.zeros(P, np.uint8), np.zeros(P, np.uint8), np.zeros(5, np.int64)
    assert lib.npore_debug_deflate_device(ctx.handle, src.ctypes.data, len(data), 50, out.ctypes.data, len(out), sizes.ctypes.data, 3,
                                          head.ctypes.data, tail.ctypes.data, info.ctypes.data) == 0, _lib.last_error()
    want = host_member(data[P - 50:2 * P - 50])
    assert info.tolist() == [1, len(want), P - 50, 150, 50 + len(data)] and out[:len(want)].tobytes() == want
    mem, head, tail, pos = device_members(ctx, data, 50, mode=1)
    assert mem == [want] and head == data[:P - 50] and tail == data[2 * P - 50:] and pos == 50 + len(data)


# ---- 2. the file pipeline ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads_10kb(tmp_path_factory):
    """200 reads of 10 kb on one contig (the benchmark's generator): about 3 MB of records, 46 members."""
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import bench_realign
    tmp = tmp_path_factory.mktemp("bam_match")
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
        want, want_h = str(tmp_path / "want.bam"), str(tmp_path / "want_h.bam")
        for path, mode in ((want, "match"), (want_h, "huffman")):
            bam.create_bam_header(path, Hdr(nb.references, nb.lengths))
            nb.write_file(idx, finals, st, path, batch_reads=9, bai=path + ".bai", compress=mode)
        want_bytes, want_bai = open(want, "rb").read(), open(want + ".bai", "rb").read()
        mem = members(want)
        assert sum(1 for m in mem if len(m[1]) == P) >= 8 and not all(m[2] for m in mem[:-1])
        assert len(want_bytes) < os.path.getsize(want_h)

        def run(name, mode="match", **kw):
            out = str(tmp_path / name)
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            stb = nb.realign_file(ctx, nf, idx, out, r=30, out_format="bam", bai=out + ".bai", compress=mode, **kw)
            assert np.array_equal(stb, st), name
            return out

        def same(out, path):
            assert open(out, "rb").read() == open(path, "rb").read(), out
            assert open(out + ".bai", "rb").read() == open(path + ".bai", "rb").read(), out

        dev = run("b5.bam", batch_reads=5)
        same(dev, want)
        same(run("b17.bam", batch_reads=17), want)
        same(run("b1000.bam", batch_reads=1000), want)
        ctx.set("tb_budget_mb", 2)                          # several groups per batch: the kernels follow the last of them
        try:
            same(run("groups.bam", batch_reads=17), want)
        finally:
            ctx.set("tb_budget_mb", 0)
        for key in ("device_pack", "device_glue"):
            ctx.set(key, 0)
            same(run(f"no_{key}.bam", batch_reads=17), want)
        ctx.set("device_pack", 1)
        ctx.set("device_glue", 1)
        check_index(dev, dev + ".bai")
        one = bam.NativeBam(src, one_pass=True)
        out = str(tmp_path / "onepass.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        n1, bad, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=17, max_reads=n, r=30, out_format="bam", bai=out + ".bai",
                                            compress="match")
        assert n1 == n and [b for b, _ in bad] == np.nonzero(st)[0].tolist()
        same(out, want)
        # a Huffman run and a stored run on the same context afterwards are what they were: the mode holds for one run
        same(run("huffman.bam", mode="huffman", batch_reads=17), want_h)
        stored = run("stored.bam", mode="none", batch_reads=17)
        assert record_stream(stored) == record_stream(want) == record_stream(want_h) and all(m[2] for m in members(stored)[:-1])
        one.close(); nb.close(); nf.close()
    finally:
        cfg.args = old


# ---- 3. the command line ------------------------------------------------------------------------------------------------------
def test_cli_golden(tmp_path):
    common = ["--bam", os.path.join(DATA, "reads.bam"), "--ref", os.path.join(DATA, "ref.fasta"), "--out_format", "bam", "--bam_compress", "match"]
    p1, p3 = str(tmp_path / "one"), str(tmp_path / "py")
    realign_cli(common + ["--out_prefix", p1], 300)
    realign_cli(common + ["--out_prefix", p3, "--python_io"], 300)
    refs = bam.read_fasta(os.path.join(DATA, "ref.fasta"))
    gold = sam_records(os.path.join(DATA, "npore_realigned.sam"))
    assert decoded_lines(p1 + ".bam", refs) == gold and len(gold) == 10
    assert record_stream(p1 + ".bam") == record_stream(p3 + ".bam")
    for p in (p1, p3):
        mem = members(p + ".bam")
        assert not mem[-2][2]                                   # the records' member is coded
        check_index(p + ".bam", p + ".bam.bai")
    import subprocess
    out = subprocess.run([sys.executable, "-m", "npore_amd.realign", "--bam", os.path.join(DATA, "reads.bam"), "--ref",
                          os.path.join(DATA, "ref.fasta"), "--bam_compress", "match", "--out_prefix", str(tmp_path / "no")],
                         cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--bam_compress needs --out_format bam" in out.stdout


def member_sizes(path):
    raw = open(path, "rb").read()
    return [struct.unpack_from("<H", raw, m[0] + 16)[0] + 1 for m in members(path)]


def test_cli_two_ranks_and_size(tmp_path, reads_10kb):
    """Two ranks give one process's record stream; and on the generator's 200 reads the file is strictly smaller than the
    Huffman mode's of the same run, every member at most its Huffman twin (rule 6; zlib at level 1 finds matches in the same
    pieces, the yardstick of the same claim)."""
    import zlib
    bp, fa, _clen = reads_10kb
    common = ["--bam", bp, "--ref", fa, "--out_format", "bam", "--batch_reads", "60"]
    b1, b2, bh = str(tmp_path / "one"), str(tmp_path / "two"), str(tmp_path / "huffman")
    realign_cli(common + ["--bam_compress", "match", "--out_prefix", b1], 300)
    realign_cli(common + ["--bam_compress", "huffman", "--out_prefix", bh], 300)
    out = realign_cli(common + ["--bam_compress", "match", "--out_prefix", b2], 600,
                      launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                "--master-port", str(29700 + os.getpid() % 100)])
    assert "no .bai index" not in out
    assert record_stream(b2 + ".bam") == record_stream(b1 + ".bam") == record_stream(bh + ".bam")
    for b in (b1, b2):
        mem = members(b + ".bam")
        assert sum(1 for m in mem if not m[2]) >= 40                # (200 reads of 10 kb: about 46 members, coded)
        check_index(b + ".bam", b + ".bam.bai")
    assert not any(os.path.exists(f"{b2}.part{k}.bam{ext}") for k in range(2) for ext in ("", ".bai"))
    ms, hs = member_sizes(b1 + ".bam"), member_sizes(bh + ".bam")
    assert len(ms) == len(hs) and all(a <= b for a, b in zip(ms, hs))
    assert os.path.getsize(b1 + ".bam") < os.path.getsize(bh + ".bam")
    pieces = [m[1] for m in members(bh + ".bam") if len(m[1]) == P]
    z1 = 0
    for piece in pieces:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z1 += len(c.compress(piece) + c.flush())
    print("match / huffman file bytes:", os.path.getsize(b1 + ".bam"), os.path.getsize(bh + ".bam"), "zlib -1 blocks:", z1)
    assert z1 < sum(hs)                                             # the yardstick finds matches in these pieces too
