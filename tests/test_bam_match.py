"""BAM out with matches in the BGZF members (--bam_compress match), the host side: the rule of csrc/deflate_code.hpp
(MATCHES) in its host twin (npore_debug_deflate_member_mode) against the Python statement (bam.deflate_member(...,
matches=True)), both decoders, the per-member size guarantee, the token stream against a brute-force restatement of
the rule, the writer with its index, the part merge.  No GPU.

Contents beside test_bam_deflate's: each aims at one place where the rule can go wrong (see match_content).

Derived bounds (no measurement):
  * rule 6 makes len(match member) <= len(huffman member) <= n + 31 for EVERY payload, and a payload without a match
    (n distinct byte values; or all 256 values equally often, where both blocks exceed the stored one) gives the Huffman
    mode's member byte for byte;
  * a run of r >= 5 equal bytes is one literal and matches of distance 1 that cover min(r - 1, 258) bytes first; what is
    left of a run of 260, 261, 262 bytes (1, 2, 3 bytes) is shorter than a match and goes out as literals.
"""
import os
import struct
import zlib

import numpy as np
import pytest

from npore_amd import _lib, bam
from test_bam_out import Hdr, PAYLOAD, check_index, long_read_bam, members, split_records
from test_bam_deflate import KINDS, SIZES, content, host_member, inflate, write_mode, writer_inputs

MATCH_KINDS = ("period", "far", "runs", "tail", "collide", "onedist", "nomatch")
FAR = (32767, 32768, 32769)
RUNS = (3, 4, 5, 257, 258, 259, 260, 261, 262, 263)


def hash4(b):
    return ((struct.unpack("<I", bytes(b))[0] * 2654435761) & 0xFFFFFFFF) >> 17


_collision = []


def colliding_grams():
    """Two different 4-grams of equal hash, found by search (letters only, so that they stand out of the filler)."""
    if not _collision:
        seen = {}
        rng = np.random.default_rng(5)
        while not _collision:
            g = bytes(rng.integers(65, 91, 4).astype(np.uint8))
            h = hash4(g)
            if h in seen and seen[h] != g:
                _collision.append((seen[h], g))
            seen[h] = g
    return _collision[0]


def match_content(kind, n):
    """n bytes, deterministic."""
    rng = np.random.default_rng(1000 + n)
    if kind == "period":            # short periods and those around a window of 64 positions: candidates in the same window or the next
        periods = (1, 2, 3, 4, 5, 6, 7, 63, 64, 65)
        seg = max(1, -(-n // len(periods)))
        out = b"".join((bytes(rng.integers(0, 256, p).astype(np.uint8)) * (seg // p + 1))[:seg] for p in periods)
        return out[:n]
    if kind == "far":               # three marked 8-byte strings in zeros, each twice: 32 767, 32 768 and 32 769 bytes apart
        out = bytearray(n)
        for k, d in enumerate(FAR):
            mark = bytes(range(16 * k + 1, 16 * k + 9))
            for at in (100 * (k + 1), 100 * (k + 1) + d):
                if at + 8 <= n:
                    out[at:at + 8] = mark
        return bytes(out)
    if kind == "runs":              # runs of one byte value each, another value per run, a separator between them
        out, k = bytearray(), 0
        while len(out) < n:
            out += bytes([1 + k % 250]) * RUNS[k % len(RUNS)] + bytes([251 + k % 5])
            k += 1
        return bytes(out[:n])
    if kind == "tail":              # the last 8 bytes repeat 8 bytes at most 1 008 back: a match that ends exactly at n
        out = bytearray(rng.permutation(np.arange(n) % 256).astype(np.uint8).tobytes())
        if n >= 24:
            at = max(0, n - 1008)
            out[n - 8:] = out[at:at + 8]
        return bytes(out)
    if kind == "collide":           # G1 + text ... G2 (same hash as G1, other bytes) ... G1 + text: G2 hides the true repeat
        g1, g2 = colliding_grams()
        text = b"0123456789"
        filler = rng.permutation(np.arange(n) % 64 + 128).astype(np.uint8).tobytes()
        out = bytearray(filler)
        for at, s in ((8, g1 + text), (30, g2), (44, g1 + text)):
            if at + len(s) <= n:
                out[at:at + len(s)] = s
        return bytes(out)
    if kind == "onedist":           # a block of 64 distinct bytes, repeated: every match lies 64 back
        return (rng.permutation(64).astype(np.uint8).tobytes() * (n // 64 + 1))[:n]
    assert kind == "nomatch"
    return content("uniform", n)


ALL = [(k, False) for k in KINDS] + [(k, True) for k in MATCH_KINDS]


def any_content(kind, new, n):
    return match_content(kind, n) if new else content(kind, n)


def host_member_mode(payload, mode):
    lib = _lib.load()
    out = np.zeros(len(payload) + 64, np.uint8)
    src = np.frombuffer(payload, np.uint8) if payload else np.zeros(1, np.uint8)
    n = lib.npore_debug_deflate_member_mode(src.ctypes.data, len(payload), out.ctypes.data, len(out), mode)
    assert n > 0, _lib.last_error()
    return out[:n].tobytes()


def brute_tokens(p):
    """Rules 1 to 4 restated without a table: O(n^2)."""
    n = len(p)
    hs = [hash4(p[i:i + 4]) for i in range(n - 3)]
    tokens, i = [], 0
    while i < n:
        c = -1
        if i <= n - 4:
            for j in range(i - 1, -1, -1):
                if hs[j] == hs[i]:
                    c = j
                    break
        length = 0
        if c >= 0:
            while length < min(258, n - i) and p[c + length] == p[i + length]:
                length += 1
        if length >= 4 and i - c <= 32768:
            tokens.append((length, i - c))
            i += length
        else:
            tokens.append(p[i])
            i += 1
    return tokens


def replay(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


# ---- 1. the flag is new ----------------------------------------------------------------------------------------------------
def test_flag_accepted():
    from test_bam_out import DATA
    nb = bam.NativeBam(os.path.join(DATA, "reads.bam"), stream=False)
    nb.set_output("bam", compress="match")
    nb.set_output("bam", bai=None, eof=False, compress="match")
    with pytest.raises(ValueError):
        nb.set_output("sam", compress="match")
    with pytest.raises(ValueError):
        nb.set_output("bam", compress="lz")
    lib = _lib.load()
    assert lib.npore_bam_set_output(nb.handle, 1, None, 12) == 0         # NPORE_OUT_DEFLATE | NPORE_OUT_MATCH
    assert lib.npore_bam_set_output(nb.handle, 1, None, 13) == 0
    assert lib.npore_bam_set_output(nb.handle, 1, None, 8) != 0          # NPORE_OUT_MATCH needs NPORE_OUT_DEFLATE
    assert lib.npore_bam_set_output(nb.handle, 0, None, 12) != 0         # ... and NPORE_OUT_BAM
    assert lib.npore_bam_set_output(nb.handle, 1, None, 16) != 0
    nb.set_output("sam")
    nb.close()
    buf = np.zeros(100, np.uint8)
    for mode in (0, 3):
        assert lib.npore_debug_deflate_member_mode(buf.ctypes.data, 10, buf.ctypes.data + 20, 80, mode) < 0
    with pytest.raises(ValueError):
        bam.bgzf_members(b"abc", "lz")


# ---- 2. the statements agree, the members decode, rule 6 ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,new", ALL)
@pytest.mark.parametrize("n", SIZES + (3,))
def test_member(kind, new, n):
    payload = any_content(kind, new, n)
    assert len(payload) == n
    m = host_member_mode(payload, 2)
    assert m == bam.deflate_member(payload, matches=True)
    h = host_member(payload)
    assert h == host_member_mode(payload, 1) == bam.deflate_member(payload)     # the Huffman mode is what it was
    assert m[:4] == b"\x1f\x8b\x08\x04" and m[10:16] == b"\x06\x00BC\x02\x00"
    assert struct.unpack_from("<H", m, 16)[0] + 1 == len(m)
    assert struct.unpack("<II", m[-8:]) == (zlib.crc32(payload), n)
    block = m[18:-8]
    assert zlib.decompress(block, -15) == payload
    assert inflate(block, n, 1) == (1, payload)                         # this tree's decoder, without a fallback to zlib
    assert len(m) <= len(h) <= n + 31
    tokens = bam.match_tokens(payload)
    assert replay(tokens) == payload
    if not any(isinstance(t, tuple) for t in tokens) or kind == "nomatch":
        assert m == h
    if m != h:                                                          # the match block: smaller than both other forms
        py_block, header_bits, data_bits = bam.deflate_match_block(payload, tokens)
        assert block == py_block and len(block) == (header_bits + data_bits + 7) // 8
        assert block[0] & 7 == 0b101 and len(block) < n + 5
        assert header_bits <= 17 + 19 * 3 + 316 * 7


# ---- 3. the token stream obeys rules 2 to 4 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,new", ALL)
@pytest.mark.parametrize("n", (3, 4, 5, 64, 65, 129, 1021, 2000))
def test_tokens_brute_force(kind, new, n):
    payload = any_content(kind, new, n)
    assert bam.match_tokens(payload) == brute_tokens(payload)


def test_far():
    """Distances 32 767 and 32 768 are matches, 32 769 is none: its eight bytes go out as literals."""
    payload = match_content("far", PAYLOAD)
    tokens = bam.match_tokens(payload)
    dists = {t[1] for t in tokens if isinstance(t, tuple)}
    assert 32767 in dists and 32768 in dists and max(dists) == 32768
    third = bytes(range(33, 41))
    lit = [t for t in tokens if not isinstance(t, tuple)]
    assert all(lit.count(b) == 2 for b in third)                        # both copies of the third string, byte by byte
    assert all(lit.count(b) == 1 for b in bytes(range(1, 9)) + bytes(range(17, 25)))


def test_runs():
    payload = match_content("runs", 2200)
    tokens, at = bam.match_tokens(payload), 0
    per_run = []
    for k, r in enumerate(RUNS):                                        # the first cycle: every value is new, the only candidates lie in the run
        got, end = [], at + r + 1
        pos = 0
        for t in tokens:
            if at <= pos < end - 1:
                got.append(t)
            pos += t[0] if isinstance(t, tuple) else 1
        per_run.append(got)
        at = end
    v = [1 + k for k in range(len(RUNS))]
    assert per_run[0] == [v[0]] * 3 and per_run[1] == [v[1]] * 4
    assert per_run[2] == [v[2], (4, 1)]
    assert per_run[3] == [v[3], (256, 1)] and per_run[4] == [v[4], (257, 1)] and per_run[5] == [v[5], (258, 1)]
    assert per_run[6] == [v[6], (258, 1), v[6]] and per_run[7] == [v[7], (258, 1), v[7], v[7]]
    assert per_run[8] == [v[8], (258, 1)] + [v[8]] * 3
    assert per_run[9] == [v[9], (258, 1), (4, 1)]


def test_tail_and_collide():
    for n in (1020, PAYLOAD):
        payload = match_content("tail", n)
        last = bam.match_tokens(payload)[-1]
        assert isinstance(last, tuple) and last[0] >= 4                 # a match ends the payload, exactly at n
    g1, g2 = colliding_grams()
    assert g1 != g2 and hash4(g1) == hash4(g2)
    payload = match_content("collide", 129)
    tokens, pos = bam.match_tokens(payload), 0
    at = {}
    for t in tokens:
        at[pos] = t
        pos += t[0] if isinstance(t, tuple) else 1
    assert at[44] == g1[0]                                              # the nearer 4-gram of equal hash hides the repeat: a literal ...
    assert at[45] == (13, 36)                                           # ... and the repeat is found one byte on


def test_onedist_single_code():
    payload = match_content("onedist", PAYLOAD)
    tokens = bam.match_tokens(payload)
    assert {t[1] for t in tokens if isinstance(t, tuple)} == {64}
    m = host_member_mode(payload, 2)
    assert len(m) < len(host_member(payload))
    hdist = ((m[18] | m[19] << 8) >> 8 & 31) + 1
    assert hdist == 12                                                  # distance 64 is symbol 11; its code is the one 1-bit code


# ---- 4. the writer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("golden", "long"))
def test_writer(which, tmp_path):
    nb, idx, finals = writer_inputs(which, tmp_path)
    st = np.zeros(len(idx), np.int32)
    stored, huff = str(tmp_path / "stored.bam"), str(tmp_path / "huffman.bam")
    write_mode(nb, idx, finals, st, stored, 7, "none")
    write_mode(nb, idx, finals, st, huff, 7, "huffman")
    files = []
    for batch_reads in (1, 7, len(idx)):
        path = str(tmp_path / f"m{batch_reads}.bam")
        info = write_mode(nb, idx, finals, st, path, batch_reads, "match")
        assert info["records"] == len(idx) and info["indexed"] == 1 and info["file_bytes"] == os.path.getsize(path)
        files.append((open(path, "rb").read(), open(path + ".bai", "rb").read()))
    assert files[0] == files[1] == files[2]
    path = str(tmp_path / "m7.bam")
    mem, smem, hmem = members(path), members(stored), members(huff)
    assert [m[1] for m in mem] == [m[1] for m in smem] == [m[1] for m in hmem]      # the record stream and its cuts
    raw, hraw = files[1][0], open(huff, "rb").read()
    n_coded = 0
    for (off, payload, _), (hoff, _, _) in zip(mem[:-1], hmem[:-1]):
        size = struct.unpack_from("<H", raw, off + 16)[0] + 1
        hsize = struct.unpack_from("<H", hraw, hoff + 16)[0] + 1
        assert size <= hsize
        if raw[off + 18] & 7 == 0b101:                                  # (the header's members are stored in every mode)
            n_coded += 1
            assert raw[off:off + size] == bam.deflate_member(payload, matches=True)
            assert hraw[hoff:hoff + hsize] == bam.deflate_member(payload)
            assert inflate(raw[off + 18:off + size - 8], len(payload), 1) == (1, payload)
    assert n_coded >= 1 and os.path.getsize(path) < os.path.getsize(huff) < os.path.getsize(stored)
    check_index(path, path + ".bai")
    # the Python writer makes the same file and index
    data = b"".join(m[1] for m in mem)
    want = nb.format_bam(idx, finals, st)
    assert data.endswith(want)
    py = str(tmp_path / "py.bam")
    bam.create_bam_header(py, Hdr(nb.references, nb.lengths))
    w = bam.BamRecordWriter(py, bai=py + ".bai", compress="match")
    stream = [r for _, r in split_records(want)]
    for k in range(0, len(stream), 13):
        w.add(stream[k:k + 13])
    assert w.close()
    assert (open(py, "rb").read(), open(py + ".bai", "rb").read()) == files[1]
    # the other modes are what they were
    h = len(data) - len(want)
    assert open(stored, "rb").read() == bam.bgzf_stored(data[:h]) + bam.bgzf_stored(data[h:]) + bam.BGZF_EOF
    assert hraw == bam.bgzf_stored(data[:h]) + bam.bgzf_members(data[h:], "huffman") + bam.BGZF_EOF
    assert all(hraw[o:o + struct.unpack_from("<H", hraw, o + 16)[0] + 1] == host_member(p) for o, p, st_ in hmem[:-1] if not st_)
    nb.close()


# ---- 5. the part merge under gloo, world 2 ---------------------------------------------------------------------------------
def _match_parts_worker(rank, world_size, port, prefix, src, finals, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from npore_amd import bam as bam_mod, dist
    nb = bam_mod.NativeBam(src, stream=False, share=False)
    n = nb.n_records
    per = (n + world_size - 1) // world_size
    mine = np.arange(rank * per, min(n, (rank + 1) * per), dtype=np.int64)
    part = f"{prefix}.part{rank}.bam"
    open(part, "w").close()
    nb.write_file(mine, [finals[k] for k in mine], np.zeros(len(mine), np.int32), part, batch_reads=7, bai=part + ".bai", eof=False,
                  compress="match")
    nb.close()
    q.put((rank, dist.gather_bam_parts(prefix + ".bam", prefix, len(mine))))


def test_part_merge_gloo_world2(tmp_path):
    import torch.multiprocessing as mp
    src = str(tmp_path / "long.bam")
    recs, finals = long_read_bam(src, n=90, contigs=3)
    nb = bam.NativeBam(src, stream=False)
    single, huff = str(tmp_path / "single.bam"), str(tmp_path / "huffman.bam")
    everything = np.arange(len(recs), dtype=np.int64)
    write_mode(nb, everything, finals, np.zeros(len(recs), np.int32), single, 1000, "match")
    write_mode(nb, everything, finals, np.zeros(len(recs), np.int32), huff, 1000, "huffman")
    prefix = str(tmp_path / "o")
    bam.create_bam_header(prefix + ".bam", Hdr(nb.references, nb.lengths))
    nb.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + os.getpid() % 2000
    procs = [ctx.Process(target=_match_parts_worker, args=(r, 2, port, prefix, src, finals, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res == [(0, 90), (1, 90)]
    assert bam._bgzf_decompress(prefix + ".bam") == bam._bgzf_decompress(single)
    assert open(prefix + ".bam", "rb").read()[-28:] == bam.BGZF_EOF
    assert os.path.getsize(single) < os.path.getsize(huff)
    check_index(prefix + ".bam", prefix + ".bam.bai")
    assert not any(os.path.exists(f"{prefix}.part{k}.bam{ext}") for k in range(2) for ext in ("", ".bai"))
