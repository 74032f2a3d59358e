"""BGZF in on the device: inflate_blocks_kernel (csrc/inflate_kernels.hpp, the decoder of csrc/inflate_wave.hpp with one
wave per stream) against its host twin on the shared cases of inflate_device_cases.py, and the readers of
npore_bam_confusion / npore_bam_purity / npore_bam_realign_sequential with Context.set("device_inflate", 1) against the
same readers inflating on the host.  Exact equality throughout.  The readers also get files whose members are made by hand
(mixed.bam: every kind of block, members the device declines, empty members inside a window) and the same files with
one member damaged: what the decoder is written to refuse, passed through it like the corrupt corpus."""
import os
import struct
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from npore_amd import aln, bam, cfg, purity, realign
import inflate_device_cases as idc
from test_bam_out import Hdr, header_len, split_records

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, "data")


@pytest.fixture(scope="module")
def ctx():
    c = aln.Context(None, None, max_n=6, max_l=100, device=0)        # an annotation-only context will do for the decoder
    yield c
    c.close()


@pytest.mark.parametrize("launch", idc.launches() + idc.corrupt_launches() + idc.mutant_launches(), ids=lambda l: l.name)
def test_kernel_equals_host_twin(ctx, launch):
    """Status and bytes equal the twin's, stream by stream, and the whole output buffer -- guards, neighbours, what a
    refused stream left in its own range -- equals the twin's.  The corrupt corpus goes through in one launch like any
    other input (test_inflate_wave.py and scripts/asan_inflate_wave.sh have passed it through the twin on a CPU)."""
    want_status, want_out = idc.twin(launch)
    status, out = idc.device(ctx, launch)
    assert set(np.unique(status).tolist()) <= {0, 1}
    differ = np.nonzero(status != want_status)[0]
    assert differ.size == 0, [(int(k), launch.cases[k][0], int(status[k])) for k in differ[:5]]
    for k in range(len(launch.cases)):
        if status[k] == 1:
            assert launch.piece(out, k) == launch.piece(want_out, k), launch.cases[k][0]
    assert launch.guards_intact(out), "wrote outside a block"
    assert np.array_equal(out, want_out), int(np.nonzero(out != want_out)[0][0])


@pytest.mark.parametrize("guard", (0, idc.GUARD))
def test_kernel_takes_the_deflate_limit_members(ctx, guard):
    """The blocks this tree's coder writes at its limits (deflate_limit_cases.py: codes of 15 bits in both alphabets, tokens of
    48 bits, 65 280 bytes each, within the 65 536 of the entry): status 1 and the payload, as the host twin has it."""
    import deflate_limit_cases as dlc
    launch = dlc.inflate_launch(guard)
    want_status, want_out = idc.twin(launch)
    status, out = idc.device(ctx, launch)
    assert (status == 1).all() and np.array_equal(status, want_status)
    for k, case in enumerate(launch.cases):
        assert launch.piece(out, k) == case[3], case[0]
    assert launch.guards_intact(out) and np.array_equal(out, want_out)


def test_out_len_beyond_a_member_is_refused_unread(ctx):
    """the device entry refuses a table with 65 537 bytes of output as a whole, as the host twin's entry does: no launch"""
    launch = idc.oversize_launch()
    out, status = launch.fresh_out(), np.full(len(launch.cases), -7, np.int32)
    rc = idc._lib.load().npore_debug_inflate_device(ctx.handle, launch.inp.ctypes.data, launch.inp.size, launch.in_off.ctypes.data, launch.in_len.ctypes.data,
                                                   out.ctypes.data, out.size, launch.out_off.ctypes.data, launch.out_len.ctypes.data,
                                                   len(launch.cases), status.ctypes.data)
    assert rc != 0 and (status == -7).all() and (out == idc.FILL).all()


def nonempty_members(path):
    raw, p, n = open(path, "rb").read(), 0, 0
    while p < len(raw):
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        n += struct.unpack_from("<I", raw, p + bsize - 4)[0] > 0
        p += bsize
    return n


@pytest.fixture(scope="module")
def written_bams(tmp_path_factory):
    """{compress: path} of one record stream of a few dozen BGZF members, written by bam.BamRecordWriter as stored, Huffman
    and match-coded members (the last two: the project's own coding, so reading them back is a round trip), + its FASTA"""
    tmp = tmp_path_factory.mktemp("inflate_device")
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import bench_realign
    bp, fa, clen = bench_realign.build_inputs(str(tmp), 420, 0, 3000, 17, procs=2)
    stream = bam._bgzf_decompress(bp)
    src = bam.BamFile(bp)
    recs = [r for _, r in split_records(stream[header_len(stream):])]
    out = {}
    for compress in ("none", "huffman", "match"):
        path = str(tmp / f"{compress}.bam")
        bam.create_bam_header(path, Hdr(src.references, src.lengths))
        w = bam.BamRecordWriter(path, compress=compress)
        w.add(recs)
        w.close()
        assert nonempty_members(path) >= 24
        out[compress] = path
    return out, fa, [(n, 0, l) for n, l in zip(src.references, src.lengths)]


def _both_routes(path, fasta, ranges, window, monkeypatch):
    """(confusion, purity, inflate_info of each) of one file with device_inflate 0 and 1"""
    if window:
        monkeypatch.setenv("NPORE_BAM_WINDOW_BLOCKS", window)
    else:
        monkeypatch.delenv("NPORE_BAM_WINDOW_BLOCKS", raising=False)
    res = {}
    for mode in (0, 1):
        c = aln.Context(None, None, max_n=6, max_l=100, device=0)
        try:
            c.set("device_inflate", mode)
            h = bam.NativeBam(path, one_pass=True, share=False)
            try:
                cms = bam.confusion_from_bam(c, h, fasta, ranges)
                info_c = h.inflate_info()
            finally:
                h.close()
            h = bam.NativeBam(path, one_pass=True, share=False)
            try:
                pur = purity.purity_from_bam(c, h, ranges, per_position=True)
                info_p = h.inflate_info()
            finally:
                h.close()
        finally:
            c.close()
        res[mode] = (cms, pur, info_c, info_p)
    return res


def _check_routes(path, fasta, ranges, window, monkeypatch, declined=0, launches=None):
    """declined: the members the device leaves to the host decoder; launches: how many windows hold a non-empty member,
    where the file has empty members other than the last"""
    res = _both_routes(path, fasta, ranges, window, monkeypatch)
    (cms0, pur0, ic0, ip0), (cms1, pur1, ic1, ip1) = res[0], res[1]
    tally = lambda t: {k: v for k, v in t.items() if not k.endswith("_ns")}     # (the kernels' time is no count)
    assert all(np.array_equal(a, b) for a, b in zip(cms0[:4], cms1[:4])) and tally(cms0[4]) == tally(cms1[4])
    assert int(cms1[0].sum()) > 0
    assert np.array_equal(pur0[0], pur1[0]) and np.array_equal(pur0[1], pur1[1]) and np.array_equal(pur0[3], pur1[3])
    assert tally(pur0[2]) == tally(pur1[2])
    assert ic0 == (0,) * 8 and ip0 == (0,) * 8
    n_blocks = nonempty_members(path)
    for info in (ic1, ip1):
        assert info[0] == n_blocks - declined and info[1] == declined and info[2] == 0 and info[7] == 1, info
        want_launches = n_blocks if window == "1" else -(-(n_blocks + 1) // 2) if window == "2" else 1
        if launches is None:
            assert info[3] >= 1 and abs(info[3] - want_launches) <= 1, (info, want_launches)     # (the empty EOF member may share a window)
        else:
            assert info[3] == launches, (info, launches)
        assert info[4] > 0 and info[5] > 0 and info[6] == sum(struct.unpack("<I", m[-4:])[0] for m in _members_raw(path))


def _members_raw(path):
    raw, p = open(path, "rb").read(), 0
    while p < len(raw):
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        yield raw[p:p + bsize]
        p += bsize


@pytest.mark.parametrize("window", [None, "1", "2"])
def test_readers_on_golden_bam(window, monkeypatch):
    f = bam.BamFile(os.path.join(DATA, "reads.bam"))
    ranges = [(n, 0, l) for n, l in zip(f.references, f.lengths)]
    _check_routes(os.path.join(DATA, "reads.bam"), os.path.join(DATA, "ref.fasta"), ranges, window, monkeypatch)


@pytest.mark.parametrize("window", [None, "1", "2"])
@pytest.mark.parametrize("compress", ["none", "huffman", "match"])
def test_readers_on_written_bams(written_bams, compress, window, monkeypatch):
    paths, fasta, ranges = written_bams
    _check_routes(paths[compress], fasta, ranges, window, monkeypatch)


@pytest.fixture(scope="module")
def mixed_bam(written_bams, tmp_path_factory):
    """(path, members, fasta, ranges, number of records) of mixed.bam: every seventh record of the written BAMs' stream behind its header, in
    members chosen by hand (inflate_device_cases.mixed_members), + its .bai"""
    paths, fasta, ranges = written_bams
    stream = bam._bgzf_decompress(paths["none"])
    hl = header_len(stream)
    recs = [r for _, r in split_records(stream[hl:])[::7]]
    members = idc.mixed_members(stream[:hl] + b"".join(recs))
    path = str(tmp_path_factory.mktemp("mixed") / "mixed.bam")
    open(path, "wb").write(b"".join(idc.member_bytes(members)))
    bam.write_bai(path)
    return path, members, fasta, ranges, len(recs)


def _windows_with_data(members, window):
    per = int(window) if window else len(members)
    return sum(any(m[2] for m in members[a:a + per]) for a in range(0, len(members), per))


@pytest.mark.parametrize("window", [None, "1", "2"])
def test_readers_on_hand_made_members(mixed_bam, window, monkeypatch):
    """mixed.bam: zlib's level 9, Z_FIXED and level 0, three sync-flushed pieces, and every fifth member an empty dynamic
    block of the end-of-block code alone in front of a stored one, which the device declines (as many as the host twin
    declines of these payloads) and the host decoder takes; empty members in between, two in a row once.  Counts equal
    the host route's, and every member is accounted for."""
    path, members, fasta, ranges, _ = mixed_bam
    kinds = [m[0] for m in members]
    lone, nonempty = kinds.count(idc.LONE_KIND), sum(bool(m[2]) for m in members)
    size = os.path.getsize(path)
    print("mixed.bam: %d bytes, %d members, %d non-empty, %d lone end-of-block, the twin declines %d" % (size, len(members), nonempty, lone, idc.twin_declines(members)))
    assert nonempty >= 30 and lone >= 6 and all(kinds.count(k) >= 6 for k, _ in idc.MEMBER_KINDS) and size < 1 << 20
    assert any(a == b == "empty" for a, b in zip(kinds, kinds[1:-1])) and kinds[0] != "empty"
    _check_routes(path, fasta, ranges, window, monkeypatch, declined=idc.twin_declines(members), launches=_windows_with_data(members, window))


def _confusion(c, path, fasta, ranges):
    h = bam.NativeBam(path, one_pass=True, share=False)
    try:
        return bam.confusion_from_bam(c, h, fasta, ranges)[:4]
    finally:
        h.close()


@pytest.mark.parametrize("what", ["crc", "stored byte", "header bit"])
def test_readers_refuse_a_damaged_member(mixed_bam, what, tmp_path, monkeypatch):
    """mixed.bam with one later member damaged -- its CRC word, a byte of a stored block (the stream inflates, the CRC tells),
    a header bit of a dynamic block (zlib refuses the stream) --: the count fails with words about BGZF on either route,
    in one window and in windows of one block, and the next count of mixed.bam is right.  In one window the device's
    tallies say what happened to the member."""
    path, members, fasta, ranges, _ = mixed_bam
    at, parts = idc.damaged_files(members)[what]
    bad = str(tmp_path / "damaged.bam")
    open(bad, "wb").write(b"".join(parts))
    lone = idc.twin_declines(members)
    want = None
    for mode in (0, 1):
        c = aln.Context(None, None, max_n=6, max_l=100, device=0)
        try:
            c.set("device_inflate", mode)
            for window in (None, "1"):
                if window:
                    monkeypatch.setenv("NPORE_BAM_WINDOW_BLOCKS", window)
                else:
                    monkeypatch.delenv("NPORE_BAM_WINDOW_BLOCKS", raising=False)
                h = bam.NativeBam(bad, one_pass=True, share=False)
                try:
                    with pytest.raises(RuntimeError, match="BGZF"):
                        bam.confusion_from_bam(c, h, fasta, ranges)
                    info = h.inflate_info()
                finally:
                    h.close()
                if mode == 1 and window is None:
                    nonempty = sum(bool(m[2]) for m in members)
                    assert info[1] == lone + (what == "header bit") and info[2] == (what != "header bit") and info[0] == nonempty - lone - 1, info
                elif mode == 0:
                    assert info == (0,) * 8
                got = _confusion(c, path, fasta, ranges)
                want = got if want is None else want
                assert all(np.array_equal(a, b) for a, b in zip(got, want)) and int(got[0].sum()) > 0, (what, mode, window)
        finally:
            c.close()


def test_realign_sequential_on_hand_made_members(mixed_bam, tmp_path):
    """rank 1 of 2 on mixed.bam: the same SAM text with the members inflated on the host and on the device"""
    path, members, fasta, _, n_records = mixed_bam
    sub, nps, _, _ = aln.load_default_tables()
    c = aln.Context(sub, nps, device=0)
    nf = bam.NativeFasta(fasta)
    try:
        res = {}
        for mode in (0, 1):
            c.set("device_inflate", mode)
            h = bam.NativeBam(path, one_pass=True, share=False)
            try:
                begin = h.set_share(1, 2)[1]
                out = str(tmp_path / f"mixed_m{mode}.sam")
                n, bad, _ = h.realign_sequential(c, nf, [(r, 0, l) for r, l in zip(h.references, h.lengths)], out, batch_reads=16, r=30)
                info = h.inflate_info()
            finally:
                h.close()
            assert not bad and (info == (0,) * 8 if mode == 0 else info[7] == 1 and info[0] > 0 and info[1] > 0 and info[2] == 0), info
            res[mode] = (open(out, "rb").read(), n, begin)
        assert res[0] == res[1] and res[0][2] > 0 and 0 < res[0][1] < n_records and len(res[0][0]) > 0
    finally:
        nf.close()
        c.close()


def _sam_records(path):
    return [l for l in open(path) if not l.startswith("@")]


def test_realign_sequential_with_device_inflate(tmp_path, written_bams):
    """The realignment of the golden BAM reads the same records either way and writes the records of npore_realigned.sam,
    also as rank 0 and rank 1 of 2 on the golden .bai (the golden file's records lie in one block: rank 1's share is empty,
    either way); a share that really starts mid-file: rank 1 of 2 on the Huffman-coded BAM of a few dozen members."""
    sub, nps, _, _ = aln.load_default_tables()
    c = aln.Context(sub, nps, device=0)
    try:
        def run(path, fasta, mode, share, tag):
            c.set("device_inflate", mode)
            h = bam.NativeBam(path, one_pass=True, share=False)
            try:
                begin = h.set_share(share, 2)[1] if share is not None else 0
                regions = [(n, 0, l) for n, l in zip(h.references, h.lengths)]
                out = str(tmp_path / f"{tag}_m{mode}_s{share}.sam")
                n, bad, _ = h.realign_sequential(c, fasta, regions, out, batch_reads=4 if tag == "golden" else 64, r=30)
                info = h.inflate_info()
            finally:
                h.close()
            assert not bad
            if mode == 0:
                assert info == (0,) * 8, info
            else:
                assert info[7] == 1 and info[2] == 0 and (info[0] > 0 or n == 0), info
            return open(out, "rb").read(), n, begin

        nf = bam.NativeFasta(os.path.join(DATA, "ref.fasta"))
        try:
            outs = {(mode, share): run(os.path.join(DATA, "reads.bam"), nf, mode, share, "golden")[0] for mode in (0, 1) for share in (None, 0, 1)}
        finally:
            nf.close()
        for share in (None, 0, 1):
            assert outs[0, share] == outs[1, share], share
        assert outs[1, 0] + outs[1, 1] == outs[1, None]
        got = outs[1, None].decode().splitlines(keepends=True)
        want = {l.split("\t")[0]: l for l in _sam_records(os.path.join(DATA, "npore_realigned.sam"))}
        assert len(got) == len(want) == 10
        for line in got:
            assert line == want[line.split("\t")[0]]
        paths, fasta, _ = written_bams
        bam.write_bai(paths["huffman"])
        nf = bam.NativeFasta(fasta)
        try:
            (text0, n0, begin0), (text1, n1, begin1) = (run(paths["huffman"], nf, mode, 1, "written") for mode in (0, 1))
        finally:
            nf.close()
        assert begin0 == begin1 > 65536 and 0 < n0 == n1 < 420 and text0 == text1
    finally:
        c.close()


def test_realign_cli_recalc_cms_with_device_inflate(tmp_path, monkeypatch):
    """`realign --bam_inflate device --recalc_cms --cms_source bam --recalc_exit` writes the matrices of `--bam_inflate host`."""
    monkeypatch.chdir(tmp_path)
    old = cfg.args
    got = {}
    try:
        for mode in ("host", "device"):
            out = tmp_path / mode
            cfg.args = realign.argparser().parse_args(
                ["--bam", os.path.join(DATA, "reads.bam"), "--ref", os.path.join(DATA, "ref.fasta"), "--out_prefix", str(tmp_path / "o"),
                 "--recalc_cms", "--recalc_exit", "--cms_source", "bam", "--stats_dir", str(out), "--chunk_width", "97", "--bam_inflate", mode])
            with pytest.raises(SystemExit) as ex:
                realign.main()
            assert ex.value.code == 0
            got[mode] = [np.load(os.path.join(out, f"{k}_cm.npy")) for k in ("subs", "nps", "inss", "dels")]
    finally:
        cfg.args = old
    assert all(np.array_equal(a, b) for a, b in zip(got["host"], got["device"])) and got["device"][0].sum() > 4000
    assert realign.argparser().parse_args(["--bam", "x", "--ref", "y", "--out_prefix", "z"]).bam_inflate == "host"
