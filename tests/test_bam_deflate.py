"""BAM out with Huffman-coded BGZF members (--bam_compress huffman), the host side: csrc/deflate_code.hpp's host twin
(npore_debug_deflate_member) against the Python statement (bam.deflate_member), both decoders, an independent
Huffman cost, the writer and its index with members of different sizes, the part merge.  No GPU.

Derived bounds (no measurement):
  * data bits: for a member whose optimal prefix code has depth <= 15 the coder's sum of count * length must EQUAL the
    cost of Huffman's algorithm on the 257-entry histogram (256 byte values, end-of-block once): the length limit does
    not act, and every optimal code has the same cost;
  * header: at most 17 bits of counts + 19 * 3 + 259 code lengths of at most 7 bits = 1887 bits, 236 bytes;
  * the stored fallback: the rule writes the stored block where the Huffman block takes >= n + 5 bytes.  With all 256
    byte values equally often (n >= 256) every code but one has 8 bits or more, so the data bits alone exceed 8 n and
    the member must be the stored one, n + 31 bytes.  A payload shorter than 256 bytes cannot hold 256 values: there the
    "uniform" content is n distinct values, Huffman may be the smaller, and the test asserts the rule itself (stored
    exactly where the Python statement's block is >= n + 5) and member <= n + 31.
"""
import heapq
import os
import struct
import zlib

import numpy as np
import pytest

from npore_amd import _lib, bam
from test_bam_out import (DATA, Hdr, PAYLOAD, check_index, golden_inputs, header_len, long_read_bam, members,
                          split_records)

SIZES = (1, 2, 63, 64, 65, 1019, 1020, 1021, 65279, 65280)
KINDS = ("one", "two", "fibonacci", "uniform", "golden")


def host_member(payload):
    lib = _lib.load()
    out = np.zeros(len(payload) + 64, np.uint8)
    src = np.frombuffer(payload, np.uint8) if payload else np.zeros(1, np.uint8)
    n = lib.npore_debug_deflate_member(src.ctypes.data, len(payload), out.ctypes.data, len(out))
    assert n > 0, _lib.last_error()
    return out[:n].tobytes()


def inflate(block, n, force):
    lib = _lib.load()
    src, out = np.frombuffer(block, np.uint8), np.zeros(max(n, 1), np.uint8)
    rc = lib.npore_debug_inflate(src.ctypes.data, len(block), out.ctypes.data, n, force)
    return rc, out[:n].tobytes()


_golden_stream = []


def golden_stream():
    """The golden BAM's own record stream (its reads with the golden final CIGARs), repeated to 65 280 bytes."""
    if not _golden_stream:
        bf, _refs, rds, _gold, finals = golden_inputs()
        one = b"".join(bam.bam_record(rd, f, bf.references) for rd, f in zip(rds, finals))
        _golden_stream.append((one * (PAYLOAD // len(one) + 1))[:PAYLOAD])
    return _golden_stream[0]


def content(kind, n):
    """n bytes, deterministic."""
    rng = np.random.default_rng(n)
    if kind == "one":
        return bytes([7]) * n
    if kind == "two":
        return bytes(rng.choice(np.array([3, 200], np.uint8), n))
    if kind == "fibonacci":
        # 22 symbols with counts 1, 1, 2, 3, 5 ...: end-of-block is the first of them, 21 byte values follow as far as n allows
        # (all of them need 46 366 bytes); what is left goes to the most frequent.  Without a limit the tree is a chain.
        fib = [1, 1]
        while len(fib) < 22:
            fib.append(fib[-1] + fib[-2])
        counts = []
        for f in fib[1:]:
            if sum(counts) + f > n:
                break
            counts.append(f)
        counts[-1] += n - sum(counts)
        out = np.repeat(np.arange(40, 40 + len(counts), dtype=np.uint8), counts)
        return bytes(rng.permutation(out))
    if kind == "uniform":
        return bytes((np.arange(n) % 256).astype(np.uint8)[rng.permutation(n)])
    return golden_stream()[:n]


def huffman_cost_and_depth(freq):
    """The yardstick: Huffman's algorithm with a heap; (sum of count * depth, depth of the tree)."""
    heap = [(f, 0) for f in freq if f]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def histogram(payload):
    freq = np.bincount(np.frombuffer(payload, np.uint8), minlength=257).tolist()
    freq[256] = 1
    return freq


def min_depth_of_optimum(freq):
    """The smallest depth any optimal code of the histogram can have is not what a heap reports (ties); so the depth test
    uses the Python statement's unlimited lengths instead: a code that IS optimal and whose depth is known."""
    lens = bam.huffman_lengths(freq, 300)
    return max(lens), sum(f * l for f, l in zip(freq, lens))


# ---- 1. the flag is new --------------------------------------------------------------------------------------------------
def test_flag_accepted():
    nb = bam.NativeBam(os.path.join(DATA, "reads.bam"), stream=False)
    nb.set_output("bam", compress="huffman")
    nb.set_output("bam", bai=None, eof=False, compress="huffman")
    with pytest.raises(ValueError):
        nb.set_output("sam", compress="huffman")
    with pytest.raises(ValueError):
        nb.set_output("bam", compress="lz")
    lib = _lib.load()
    assert lib.npore_bam_set_output(nb.handle, 0, None, 4) != 0          # NPORE_OUT_DEFLATE needs NPORE_OUT_BAM
    assert lib.npore_bam_set_output(nb.handle, 1, None, 8) != 0          # an unknown flag is still refused
    nb.set_output("sam")
    nb.close()


# ---- 2. / 3. member sizes and contents; size against the yardstick ----------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_member(kind, n):
    payload = content(kind, n)
    assert len(payload) == n
    h = host_member(payload)
    assert h == bam.deflate_member(payload)
    assert h[:4] == b"\x1f\x8b\x08\x04" and h[10:16] == b"\x06\x00BC\x02\x00"
    assert struct.unpack_from("<H", h, 16)[0] + 1 == len(h)
    assert struct.unpack("<II", h[-8:]) == (zlib.crc32(payload), n)
    block = h[18:-8]
    assert zlib.decompress(block, -15) == payload
    for force in (1, 2):                                               # this tree's decoder without a fallback; zlib
        assert inflate(block, n, force) == (1, payload), force
    assert len(h) <= n + 31
    py_block, header_bits, data_bits = bam.deflate_block(payload)
    stored = len(h) == n + 31 and block[:5] == struct.pack("<BHH", 1, n, n ^ 0xFFFF) and block[5:] == payload
    assert stored == (py_block is None) == ((header_bits + data_bits + 7) // 8 >= n + 5)
    if kind == "uniform" and n >= 256:
        assert stored and len(h) == n + 31
    if kind in ("one", "two") and n >= 63:
        assert not stored
    freq = histogram(payload)
    depth, cost = min_depth_of_optimum(freq)
    assert cost == huffman_cost_and_depth(freq)[0]                     # (the statement's unlimited code is optimal)
    if kind == "fibonacci" and n >= 65279:
        assert depth > 15                                              # the length limit must act: 22 Fibonacci counts and end-of-block
        assert max(bam.huffman_lengths(freq, 15)) == 15 and data_bits >= cost
    else:
        assert depth <= 15
        assert data_bits == cost
    assert header_bits <= 17 + 19 * 3 + 259 * 7
    if not stored:
        assert block[0] & 7 == 0b101                                   # one FINAL block of type 2
        assert len(block) == (header_bits + data_bits + 7) // 8


def test_lengths_never_exceed_the_limit():
    """Histograms that force the limit at both alphabets: Fibonacci counts (depth = symbols - 1 without it)."""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    for nsym, limit in ((24, 15), (19, 7), (12, 7)):
        lens = bam.huffman_lengths(fib[:nsym], limit)
        assert max(lens) == limit and min(lens) >= 1
        assert sum(2.0 ** -l for l in lens) == 1.0                     # a complete code: both decoders insist on it


# ---- 4. the writer ---------------------------------------------------------------------------------------------------------
def write_mode(nb, idx, finals, st, path, batch_reads, compress):
    bam.create_bam_header(path, Hdr(nb.references, nb.lengths))
    return nb.write_file(idx, finals, st, path, batch_reads=batch_reads, bai=path + ".bai", compress=compress)


def writer_inputs(which, tmp_path):
    if which == "golden":
        bf, _refs, rds, _gold, finals = golden_inputs()
        nb = bam.NativeBam(os.path.join(DATA, "reads.bam"), stream=False)
        idx = nb.select([(n, 0, l - 1) for n, l in zip(bf.references, bf.lengths)])
        return nb, idx, finals
    src = str(tmp_path / "long.bam")
    recs, finals = long_read_bam(src)
    return bam.NativeBam(src, stream=False), np.arange(len(recs), dtype=np.int64), finals


@pytest.mark.parametrize("which", ("golden", "long"))
def test_writer(which, tmp_path):
    nb, idx, finals = writer_inputs(which, tmp_path)
    st = np.zeros(len(idx), np.int32)
    stored = str(tmp_path / "stored.bam")
    write_mode(nb, idx, finals, st, stored, 7, "none")
    files = []
    for batch_reads in (1, 7, len(idx)):
        path = str(tmp_path / f"h{batch_reads}.bam")
        info = write_mode(nb, idx, finals, st, path, batch_reads, "huffman")
        assert info["records"] == len(idx) and info["indexed"] == 1 and info["file_bytes"] == os.path.getsize(path)
        files.append((open(path, "rb").read(), open(path + ".bai", "rb").read()))
    assert files[0] == files[1] == files[2]
    path = str(tmp_path / "h7.bam")
    mem = members(path)                                                # (framing, CRC-32 and ISIZE of every member)
    smem = members(stored)
    assert b"".join(m[1] for m in mem) == b"".join(m[1] for m in smem)
    assert [len(m[1]) for m in mem] == [len(m[1]) for m in smem]       # the cuts do not depend on the mode
    data = b"".join(m[1] for m in mem)
    h = header_len(data)
    n_hdr = 0
    while sum(len(m[1]) for m in mem[:n_hdr]) < h:
        n_hdr += 1
    body = mem[n_hdr:-1]
    assert body and all(len(m[1]) == PAYLOAD for m in body[:-1]) and 0 < len(body[-1][1]) <= PAYLOAD
    assert mem[-1][1] == b"" and files[1][0][-28:] == bam.BGZF_EOF
    assert os.path.getsize(path) < os.path.getsize(stored)
    raw = files[1][0]
    for off, payload, _ in body:                                       # every member is what the statement says, and our decoder takes it
        size = struct.unpack_from("<H", raw, off + 16)[0] + 1
        assert raw[off:off + size] == bam.deflate_member(payload)
        assert inflate(raw[off + 18:off + size - 8], len(payload), 1) == (1, payload)
    check_index(path, path + ".bai")
    # the library's own readers take the file: indexed and one-pass
    want = nb.format_bam(idx, finals, st)
    assert data[h:] == want
    back = bam.NativeBam(path, stream=False)
    regions = [(n, 0, l) for n, l in zip(back.references, back.lengths)]
    sel = back.select(regions)
    assert back.n_records == len(idx) and len(sel) == len(idx)
    assert back.format_bam(sel, finals, st) == want
    back.close()
    from model import bam_walk
    one = bam_walk.one_pass(path, [(k, 0, l) for k, l in enumerate(nb.lengths)])
    assert np.array_equal(np.asarray(one), np.array([h + o for o, _ in split_records(data[h:])]))
    # the Python writer makes the same file and index
    py = str(tmp_path / "py.bam")
    bam.create_bam_header(py, Hdr(nb.references, nb.lengths))
    w = bam.BamRecordWriter(py, bai=py + ".bai", compress="huffman")
    stream = [r for _, r in split_records(want)]
    for k in range(0, len(stream), 13):
        w.add(stream[k:k + 13])
    assert w.close()
    assert (open(py, "rb").read(), open(py + ".bai", "rb").read()) == files[1]
    # the stored mode is what it was: the stream in stored members, as the Python statement of that mode writes them
    assert open(stored, "rb").read() == (bam.bgzf_stored(data[:h]) + bam.bgzf_stored(data[h:]) + bam.BGZF_EOF)
    assert all(m[2] for m in smem[:-1])
    check_index(stored, stored + ".bai")
    nb.close()


# ---- 5. the part merge under gloo, world 2 ---------------------------------------------------------------------------------
def _deflate_parts_worker(rank, world_size, port, prefix, src, finals, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from npore_amd import bam as bam_mod, dist
    nb = bam_mod.NativeBam(src, stream=False, share=False)
    n = nb.n_records
    per = (n + world_size - 1) // world_size
    mine = np.arange(rank * per, min(n, (rank + 1) * per), dtype=np.int64)
    part = f"{prefix}.part{rank}.bam"
    open(part, "w").close()
    nb.write_file(mine, [finals[k] for k in mine], np.zeros(len(mine), np.int32), part, batch_reads=7, bai=part + ".bai", eof=False,
                  compress="huffman")
    nb.close()
    q.put((rank, dist.gather_bam_parts(prefix + ".bam", prefix, len(mine))))


def test_part_merge_gloo_world2(tmp_path):
    import torch.multiprocessing as mp
    src = str(tmp_path / "long.bam")
    recs, finals = long_read_bam(src, n=90, contigs=3)
    nb = bam.NativeBam(src, stream=False)
    single = str(tmp_path / "single.bam")
    write_mode(nb, np.arange(len(recs), dtype=np.int64), finals, np.zeros(len(recs), np.int32), single, 1000, "huffman")
    prefix = str(tmp_path / "o")
    bam.create_bam_header(prefix + ".bam", Hdr(nb.references, nb.lengths))
    nb.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000
    procs = [ctx.Process(target=_deflate_parts_worker, args=(r, 2, port, prefix, src, finals, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res == [(0, 90), (1, 90)]
    assert bam._bgzf_decompress(prefix + ".bam") == bam._bgzf_decompress(single)
    assert open(prefix + ".bam", "rb").read()[-28:] == bam.BGZF_EOF
    mem = members(prefix + ".bam")
    assert not all(m[2] for m in mem[:-1])                              # (Huffman members, not stored ones)
    check_index(prefix + ".bam", prefix + ".bam.bai")
    assert not any(os.path.exists(f"{prefix}.part{k}.bam{ext}") for k in range(2) for ext in ("", ".bai"))
