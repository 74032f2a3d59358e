"""BAM output (--out_format bam), host side: the record encoder npore_bam_format_bam, the stored-BGZF writer with its
framing and its .bai, the part merge -- against the statement of the format in npore_amd/csrc/bam_reader.hpp ("BAM out:
records and file, stated once") and its pure-Python twin bam.bam_record.  The decoder throughout is bam._bgzf_decompress
+ bam.BamFile (Python's zlib and struct), never the library's own inflate.  No GPU here: the final CIGARs are given.
"""
import argparse
import os
import struct
import zlib

import numpy as np
import pytest

from npore_amd import bam, cfg
from conftest import GOLDEN

DATA = os.path.join(GOLDEN, "data")
SEQ16 = "=ACMGRSVTWYHKDBN"
PAYLOAD = 65280
BIG = 1 << 29


# ---- test-side helpers (nothing below comes from the code under test) --------------------------------------------------
def spec_reg2bin(beg, end):
    """The bin of [beg, end): the smallest bin of the 6-level scheme (level l: bins of 2^(29 - 3l) bases, the first one
    numbered (8^l - 1) / 7) that holds the whole interval."""
    end -= 1
    for level in range(5, -1, -1):
        shift = 29 - 3 * level
        if beg >> shift == end >> shift:
            return (8 ** level - 1) // 7 + (beg >> shift)
    raise AssertionError


def hp_aux(hp):
    """(type letter, bytes) of the smallest integer type, htslib's order."""
    if hp >= 0:
        return ("C", struct.pack("<B", hp)) if hp < 256 else ("S", struct.pack("<H", hp)) if hp < 65536 else ("I", struct.pack("<I", hp))
    return ("c", struct.pack("<b", hp)) if hp >= -128 else ("s", struct.pack("<h", hp)) if hp >= -32768 else ("i", struct.pack("<i", hp))


def make_bam(path, references, records):
    """A BAM (deflated members) of records given as dicts: name, flag, ref_id, pos, mapq, cigar [(op, len)], seq, qual
    (bytes / None), hp (int / None, written in the type hp_aux picks)."""
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in references)
    out = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(references)))
    for n, l in references:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    code = {c: i for i, c in enumerate(SEQ16)}
    for r in records:
        name = r["name"].encode() + b"\0"
        nib = [code[c] for c in r["seq"]] + ([0] if len(r["seq"]) & 1 else [])
        packed = bytes(nib[k] << 4 | nib[k + 1] for k in range(0, len(nib), 2))
        qual = bytes([0xFF]) * len(r["seq"]) if r.get("qual") is None else bytes(r["qual"])
        cig = b"".join(struct.pack("<I", ln << 4 | op) for op, ln in r["cigar"])
        aux = b"XAA!"                                   # (a tag in front of HP, which the writer must not carry over)
        if r.get("hp") is not None:
            t, v = hp_aux(r["hp"])
            aux += b"HP" + t.encode() + v
        body = struct.pack("<iiBBHHHiiii", r["ref_id"], r["pos"], len(name), r.get("mapq", 60), 0, len(r["cigar"]), r["flag"],
                           len(r["seq"]), 5, 77, 9) + name + cig + packed + qual + aux
        out += struct.pack("<i", len(body)) + body
    with open(path, "wb") as fh:
        for p in range(0, len(out), 0xFF00):
            chunk = bytes(out[p:p + 0xFF00])
            comp = zlib.compressobj(6, zlib.DEFLATED, -15)
            data = comp.compress(chunk) + comp.flush()
            fh.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(data) + 25) + data +
                     struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def members(path):
    """[(file offset, payload, is a single stored block)] of a BGZF file; asserts the gzip framing, CRC-32 and ISIZE."""
    raw = open(path, "rb").read()
    out, p = [], 0
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04" and raw[p + 10:p + 16] == b"\x06\x00BC\x02\x00", p
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        deflate = raw[p + 18:p + bsize - 8]
        crc, isize = struct.unpack_from("<II", raw, p + bsize - 8)
        payload = zlib.decompress(deflate, -15)
        assert zlib.crc32(payload) == crc and len(payload) == isize, p
        stored = len(deflate) == isize + 5 and deflate[0] == 1 and struct.unpack_from("<HH", deflate, 1) == (isize, isize ^ 0xFFFF)
        out.append((p, payload, stored))
        p += bsize
    assert p == len(raw)
    return out


def split_records(stream):
    """[(offset, record bytes)] of a record stream (no header)."""
    out, p = [], 0
    while p < len(stream):
        bs, = struct.unpack_from("<i", stream, p)
        out.append((p, stream[p:p + 4 + bs]))
        p += 4 + bs
    assert p == len(stream)
    return out


def header_len(data):
    l_text, = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, p)
        p += 8 + l_name
    return p


def parse_bai(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", raw, 4)
    q, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", raw, q); q += 4
        bins = {}
        for _ in range(n_bin):
            b_id, n_chunk = struct.unpack_from("<Ii", raw, q); q += 8
            assert b_id not in bins and n_chunk > 0
            v = struct.unpack_from(f"<{2 * n_chunk}Q", raw, q); q += 16 * n_chunk
            bins[b_id] = list(zip(v[0::2], v[1::2]))
        n_intv, = struct.unpack_from("<i", raw, q); q += 4
        refs.append((bins, list(struct.unpack_from(f"<{n_intv}Q", raw, q)))); q += 8 * n_intv
    assert q == len(raw) or q + 8 == len(raw)
    return refs


def check_index(bam_path, bai_path):
    """Test 4's walker: every bin's chunks, sought in the inflated stream, hold exactly the records whose reg2bin is that
    bin (in file order); the linear index is what bam.write_bai computes for the same file."""
    mem = members(bam_path)
    start_of = {}                                           # member file offset -> offset of its payload in the stream
    u = 0
    for off, payload, _ in mem:
        start_of[off] = u
        u += len(payload)
    data = b"".join(m[1] for m in mem)

    def to_stream(v):
        assert (v >> 16) in start_of, hex(v)
        return start_of[v >> 16] + (v & 0xFFFF)

    h = header_len(data)
    n_ref = len(parse_bai(bai_path))
    want = [dict() for _ in range(n_ref)]
    for off, rec in split_records(data[h:]):
        rid, pos, l_rn, _mq, _bin, n_cig = struct.unpack_from("<iiBBHH", rec, 4)
        cig = struct.unpack_from(f"<{n_cig}I", rec, 36 + l_rn)
        reflen = sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8))
        want[rid].setdefault(spec_reg2bin(pos, pos + max(1, reflen)), []).append(h + off)
    got = parse_bai(bai_path)
    for rid, (bins, _lin) in enumerate(got):
        assert set(bins) == set(want[rid]), rid
        for b_id, chunks in bins.items():
            found = []
            for c0, c1 in chunks:
                p, e = to_stream(c0), to_stream(c1)
                assert p < e
                while p < e:
                    found.append(p)
                    p += 4 + struct.unpack_from("<i", data, p)[0]
                assert p == e                                # a chunk ends where a record ends
            assert found == want[rid][b_id], (rid, b_id)
    ref_bai = bai_path + ".lin"
    bam.write_bai(bam_path, ref_bai)
    lin = parse_bai(ref_bai)
    assert [l for _, l in got] == [l for _, l in lin]
    return got


class Hdr:
    def __init__(self, references, lengths):
        self.references, self.lengths = references, lengths


def write_native(nb, idx, finals, status, path, batch_reads, bai=True, eof=True):
    bam.create_bam_header(path, Hdr(nb.references, nb.lengths))
    return nb.write_file(idx, finals, status, path, batch_reads=batch_reads, bai=path + ".bai" if bai else None, eof=eof)


def decoded_lines(path, refs, finals_by_name=None):
    """SAM lines of a written BAM through the independent decoder: BamFile -> get_read_data -> sam_line with the CIGAR
    the record itself carries."""
    old = cfg.args
    b = bam.BamFile(path)
    cfg.args = argparse.Namespace(max_reads=0, regions=[(n, 0, l) for n, l in zip(b.references, b.lengths)])
    try:
        return [bam.sam_line(rd, rd[5]) for rd in bam.get_read_data(b, refs)]
    finally:
        cfg.args = old


# ---- 1. the host encoder against the golden data -----------------------------------------------------------------------
def golden_inputs():
    old = cfg.args
    bf = bam.BamFile(os.path.join(DATA, "reads.bam"))
    refs = bam.read_fasta(os.path.join(DATA, "ref.fasta"))
    cfg.args = argparse.Namespace(max_reads=0, regions=[(n, 0, l - 1) for n, l in zip(bf.references, bf.lengths)])
    try:
        rds = list(bam.get_read_data(bf, refs))
    finally:
        cfg.args = old
    gold = [l for l in open(os.path.join(DATA, "npore_realigned.sam")) if not l.startswith("@")]
    final_of = {l.split("\t")[0]: l.split("\t")[5] for l in gold}
    return bf, refs, rds, gold, [final_of[rd[0]] for rd in rds]


def test_host_encoder_golden(tmp_path):
    bf, refs, rds, gold, finals = golden_inputs()
    nb = bam.NativeBam(os.path.join(DATA, "reads.bam"), stream=False)
    idx = nb.select([(n, 0, l - 1) for n, l in zip(bf.references, bf.lengths)])
    assert len(idx) == len(rds) == len(gold) == 10
    got = nb.format_bam(idx, finals, np.zeros(10, np.int32))
    assert got == b"".join(bam.bam_record(rd, f, bf.references) for rd, f in zip(rds, finals))
    out = str(tmp_path / "g.bam")
    info = write_native(nb, idx, finals, np.zeros(10, np.int32), out, 4)
    assert info["records"] == 10 and info["indexed"] == 1
    assert decoded_lines(out, refs) == gold
    nb.close()


# ---- 2. synthetic records ----------------------------------------------------------------------------------------------
def synthetic_records():
    rng = np.random.default_rng(11)
    recs, finals = [], []
    positions = []
    for b in (1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26):
        positions += [b - 150, b - 100, b - 1, b, b + 7]
    hps = [None, 0, 2, 255, 256, -1, -129, 70000, -128, 65535, 65536, -32768, -32769]
    for k, pos in enumerate(sorted(positions)):
        lead, trail = (0, 3, 4, 1, 0, 7)[k % 6], (0, 2, 0, 5)[k % 4]
        reflen, body = 100, 90 + k % 5
        cig = ([(5, 6)] if k % 5 == 1 else []) + ([(4, lead)] if lead else []) + [(0, 50), (1, body - 90), (2, 10), (0, 40)] + \
              ([(4, trail)] if trail else []) + ([(5, 9)] if k % 7 == 2 else [])
        cig = [c for c in cig if c[1] > 0]
        seq = "".join(SEQ16[x] for x in rng.integers(1, 16, lead + body + trail))
        name = "n" if k == 3 else "L" * 254 if k == 4 else f"read{k}"
        recs.append(dict(name=name, flag=16 if k % 3 == 0 else 0, ref_id=0, pos=pos, mapq=k % 61, cigar=cig, seq=seq,
                         qual=None if k % 4 == 1 else bytes(rng.integers(0, 60, len(seq)).tolist()), hp=hps[k % len(hps)]))
        finals.append(f"{40 + k}M{body - 90 + 1}I{11}D{49 - k}M" if k % 2 else f"{reflen}M")
        recs[-1]["_lead"], recs[-1]["_trail"], recs[-1]["_reflen"] = lead, trail, reflen
    return recs, finals


def test_synthetic_records(tmp_path):
    recs, finals = synthetic_records()
    src = str(tmp_path / "syn.bam")
    make_bam(src, [("big", BIG)], recs)
    nb = bam.NativeBam(src, stream=False)
    idx = np.arange(len(recs), dtype=np.int64)
    status = np.zeros(len(recs), np.int32)
    status[6] = 32                                           # a refused read: left out
    kept = [k for k in range(len(recs)) if k != 6]
    got = nb.format_bam(idx, finals, status)
    # the Python statement, from the independent decoder's view of the input
    bf = bam.BamFile(src)
    old = cfg.args
    cfg.args = argparse.Namespace(max_reads=0, regions=[("big", 0, BIG)])
    try:
        rds = list(bam.get_read_data(bf, {"big": ""}))
    finally:
        cfg.args = old
    assert len(rds) == len(recs)
    assert got == b"".join(bam.bam_record(rds[k], finals[k], bf.references) for k in kept)
    # field by field, from the bytes
    out = split_records(got)
    assert len(out) == len(kept)
    seen_types = set()
    for (off, rec), k in zip(out, kept):
        r = recs[k]
        rid, pos, l_rn, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
        lead, trail = r["_lead"], r["_trail"]
        want_seq = r["seq"][lead:len(r["seq"]) - trail]
        assert (rid, pos, mapq, flag, nref, npos, tlen) == (0, r["pos"], r["mapq"], r["flag"], -1, -1, r["_reflen"])
        assert bin_ == spec_reg2bin(pos, pos + r["_reflen"]) and l_seq == len(want_seq)
        q = 36
        assert rec[q:q + l_rn] == r["name"].encode() + b"\0"
        q += l_rn
        words = struct.unpack_from(f"<{n_cig}I", rec, q)
        assert "".join(f"{w >> 4}{'MID'[w & 15]}" for w in words) == finals[k]
        q += 4 * n_cig
        nb_ = (l_seq + 1) // 2
        nibs = "".join(SEQ16[b >> 4] + SEQ16[b & 15] for b in rec[q:q + nb_])
        assert nibs[:l_seq] == want_seq and (l_seq % 2 == 0 or rec[q + nb_ - 1] & 15 == 0)
        q += nb_
        assert rec[q:q + l_seq] == (bytes([0xFF]) * l_seq if r["qual"] is None else bytes(r["qual"])[lead:lead + l_seq])
        q += l_seq
        t, v = hp_aux(0 if r["hp"] is None else r["hp"])
        assert rec[q:] == b"HP" + t.encode() + v
        seen_types.add(t)
    assert seen_types == set("CSIcsi")
    assert {len(recs[k]["name"]) for k in kept} >= {1, 254} and {recs[k]["_lead"] % 2 for k in kept if recs[k]["_lead"]} == {0, 1}
    # ... and as a file: the decoder reads back the same reads, the index holds
    path = str(tmp_path / "syn_out.bam")
    info = write_native(nb, idx, finals, status, path, 5)
    assert info["records"] == len(kept) and info["indexed"] == 1
    back = bam.BamFile(path)
    assert [r.query_name for r in back.records] == [recs[k]["name"] for k in kept]
    assert [r.hp for r in back.records] == [recs[k]["hp"] or 0 for k in kept]
    check_index(path, path + ".bai")
    # a final text that is no CIGAR is refused, not written
    with pytest.raises(RuntimeError):
        nb.format_bam(idx[:1], ["12"], status[:1])
    nb.close()


# ---- 3. / 4. framing and index -------------------------------------------------------------------------------------------
def long_read_bam(path, n=60, contigs=2):
    """Reads of 3 - 9 kb over `contigs` contigs, a few hundred KB of records: several members, hundreds of windows."""
    rng = np.random.default_rng(3)
    recs, finals = [], []
    for k in range(n):
        L = int(rng.integers(3000, 9000))
        lead = int(rng.integers(0, 4))
        seq = "".join("ACGT"[x] for x in rng.integers(0, 4, L + lead))
        recs.append(dict(name=f"long{k}", flag=0, ref_id=k * contigs // n, pos=(k % (n // contigs)) * 5000 + 17,
                         cigar=([(4, lead)] if lead else []) + [(0, L)], seq=seq, qual=bytes(rng.integers(0, 50, L + lead).tolist()),
                         hp=k % 3))
        finals.append(f"{L // 2}M3I3D{L - L // 2 - 3}M")
    make_bam(path, [(f"c{j}", 10_000_000) for j in range(contigs)], recs)
    return recs, finals


def test_framing(tmp_path):
    src = str(tmp_path / "long.bam")
    recs, finals = long_read_bam(src)
    nb = bam.NativeBam(src, stream=False)
    idx = np.arange(len(recs), dtype=np.int64)
    st = np.zeros(len(recs), np.int32)
    files = []
    for nbatch in (1, 3, 7):
        path = str(tmp_path / f"b{nbatch}.bam")
        write_native(nb, idx, finals, st, path, (len(recs) + nbatch - 1) // nbatch)
        files.append(open(path, "rb").read())
    assert files[0] == files[1] == files[2]
    path = str(tmp_path / "b1.bam")
    mem = members(path)                                       # (CRC-32 and ISIZE of every member checked there)
    data = b"".join(m[1] for m in mem)
    h = header_len(data)
    # the header in members of its own, then the record stream cut every 65 280 bytes, then the EOF member
    assert mem[-1][1] == b"" and open(path, "rb").read()[-28:] == bam.BGZF_EOF
    n_hdr = 0
    while sum(len(m[1]) for m in mem[:n_hdr]) < h:
        n_hdr += 1
    assert sum(len(m[1]) for m in mem[:n_hdr]) == h
    body = mem[n_hdr:-1]
    assert len(body) >= 4 and all(len(m[1]) == PAYLOAD for m in body[:-1]) and 0 < len(body[-1][1]) <= PAYLOAD
    assert all(m[2] and len(m[1]) <= 65536 for m in mem[:-1])
    want = nb.format_bam(idx, finals, st)
    assert data[h:] == want
    # the library's own readers take the file: resident and one-pass
    back = bam.NativeBam(path, stream=False)
    assert back.n_records == len(recs) and back.references == nb.references and back.lengths == nb.lengths
    regions = [(n, 0, l) for n, l in zip(back.references, back.lengths)]
    assert np.array_equal(back.select(regions), idx)
    assert back.format_bam(idx, finals, st) == want           # (a written record, realigned to the same CIGAR, is itself)
    back.close()
    streamed = bam.NativeBam(path, stream=True)
    assert streamed.streamed and streamed.n_records == len(recs) and np.array_equal(streamed.select(regions), idx)
    assert streamed.format_bam(idx, finals, st) == want
    streamed.close()
    nb.close()
    from model import bam_walk                                # the one-pass walker, built without HIP
    one = bam_walk.one_pass(path, [(0, 0, 10_000_000), (1, 0, 10_000_000)])
    offs = np.array([h + o for o, _ in split_records(data[h:])])
    assert np.array_equal(np.asarray(one), offs)


def test_index_and_shares(tmp_path, capfd):
    src = str(tmp_path / "long.bam")
    recs, finals = long_read_bam(src, n=90, contigs=3)
    nb = bam.NativeBam(src, stream=False)
    idx = np.arange(len(recs), dtype=np.int64)
    st = np.zeros(len(recs), np.int32)
    path = str(tmp_path / "ix.bam")
    info = write_native(nb, idx, finals, st, path, 11)
    assert info["indexed"] == 1
    got = check_index(path, path + ".bai")
    assert all(bins and lin for bins, lin in got)
    # the pure-Python writer makes the same file, and an index that passes the same walk
    py = str(tmp_path / "py.bam")
    bam.create_bam_header(py, Hdr(nb.references, nb.lengths))
    w = bam.BamRecordWriter(py, bai=py + ".bai")
    stream = [r for _, r in split_records(nb.format_bam(idx, finals, st))]
    for k in range(0, len(stream), 13):
        w.add(stream[k:k + 13])
    assert w.close()
    assert open(py, "rb").read() == open(path, "rb").read()
    check_index(py, py + ".bai")
    assert open(py + ".bai", "rb").read() == open(path + ".bai", "rb").read()
    # npore_bam_set_share takes the index: the stretches begin at record starts and tile the file
    data = bam._bgzf_decompress(path)
    h = header_len(data)
    starts = {h + o for o, _ in split_records(data[h:])}
    for world in (2, 3, 5):
        prev_end = None
        for rank in range(world):
            hnd = bam.NativeBam(path, one_pass=True, share=False)
            has, b0, e0, _ = hnd.set_share(rank, world)
            hnd.close()
            assert has == 1
            if rank == 0:
                assert b0 == 0
            else:
                assert b0 == prev_end and b0 in starts
            assert (e0 == -1) == (rank == world - 1)
            prev_end = e0
    # records out of order: the BAM alone, and one line saying so
    capfd.readouterr()
    rev = str(tmp_path / "rev.bam")
    info = write_native(nb, idx[::-1].copy(), finals[::-1], st, rev, 11)
    assert info["indexed"] == -1 and info["records"] == len(recs) and not os.path.exists(rev + ".bai")
    assert "no .bai index is written" in capfd.readouterr().out
    assert [r.query_name for r in bam.BamFile(rev).records] == [r["name"] for r in recs[::-1]]
    nb.close()


# ---- 5. the part merge under gloo, world 2 ---------------------------------------------------------------------------------
def _bam_parts_worker(rank, world_size, port, prefix, src, finals, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from npore_amd import bam as bam_mod, dist
    nb = bam_mod.NativeBam(src, stream=False, share=False)
    n = nb.n_records
    per = (n + world_size - 1) // world_size
    mine = np.arange(rank * per, min(n, (rank + 1) * per), dtype=np.int64)
    part = f"{prefix}.part{rank}.bam"
    open(part, "w").close()
    nb.write_file(mine, [finals[k] for k in mine], np.zeros(len(mine), np.int32), part, batch_reads=7, bai=part + ".bai", eof=False)
    nb.close()
    q.put((rank, dist.gather_bam_parts(prefix + ".bam", prefix, len(mine))))


def test_part_merge_gloo_world2(tmp_path):
    import torch.multiprocessing as mp
    src = str(tmp_path / "long.bam")
    recs, finals = long_read_bam(src, n=90, contigs=3)
    nb = bam.NativeBam(src, stream=False)
    single = str(tmp_path / "single.bam")
    write_native(nb, np.arange(len(recs), dtype=np.int64), finals, np.zeros(len(recs), np.int32), single, 1000)
    prefix = str(tmp_path / "o")
    bam.create_bam_header(prefix + ".bam", Hdr(nb.references, nb.lengths))
    nb.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    procs = [ctx.Process(target=_bam_parts_worker, args=(r, 2, port, prefix, src, finals, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res == [(0, 90), (1, 90)]
    assert bam._bgzf_decompress(prefix + ".bam") == bam._bgzf_decompress(single)
    assert open(prefix + ".bam", "rb").read()[-28:] == bam.BGZF_EOF
    members(prefix + ".bam")
    check_index(prefix + ".bam", prefix + ".bam.bai")
    assert not any(os.path.exists(f"{prefix}.part{k}.bam{ext}") for k in range(2) for ext in ("", ".bai"))
