"""The host twin of the wave-per-stream DEFLATE decoder (csrc/inflate_wave.hpp, npore_debug_inflate_wave_host) against
zlib.decompressobj(-15) on the shared cases of inflate_device_cases.py: the code the gfx950 kernel runs, with the loop over
the lanes written out.  No GPU."""
import os
import re

import numpy as np
import pytest

from npore_amd import _lib, bam
import inflate_device_cases as idc

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "npore_amd.h")
LONE = "lone end-of-block code, then stored"
NEW_NAMES = ("npore_debug_inflate_device", "npore_debug_inflate_wave_host", "npore_bam_inflate_info")


def host_decoder_takes(raw, n):
    """csrc/inflate.hpp alone (force = 1) on the stream"""
    src = np.frombuffer(raw + b"\0", np.uint8)
    out = np.zeros(n + 1, np.uint8)
    return _lib.load().npore_debug_inflate(src.ctypes.data, len(raw), out.ctypes.data, n, 1) == 1


@pytest.mark.parametrize("launch", idc.launches(), ids=lambda l: l.name)
def test_twin_equals_zlib(launch):
    """Status 1 means zlib's bytes, and that zlib accepts the stream with that size; a malformed twin of a stream gets
    status 0; every valid stream that csrc/inflate.hpp takes by itself, the twin takes too; guard bytes and the
    neighbours' bytes are as they were."""
    status, out = idc.twin(launch)
    assert launch.guards_intact(out), "wrote outside a block"
    for k, (name, raw, n, want) in enumerate(launch.cases):
        assert status[k] in (0, 1), (name, status[k])
        if want is None:
            assert status[k] == 0, name
            continue
        if status[k] == 1:
            assert launch.piece(out, k) == want, name
        else:
            assert not host_decoder_takes(raw, n), name + ": csrc/inflate.hpp takes it, the twin does not"


def test_twin_takes_nearly_everything():
    """what the twin declines goes to the host decoder in production: that must stay the exception"""
    launch = idc.launches()[0]
    status, _ = idc.twin(launch)
    valid = [k for k, c in enumerate(launch.cases) if c[3] is not None]
    assert sum(int(status[k]) for k in valid) >= 0.9 * len(valid)
    taken = {c[0] for k, c in enumerate(launch.cases) if status[k] == 1}
    for name in ("empty", "BGZF EOF payload", "1 bytes", "65535 bytes", "65536 bytes", "sync and full flush", "stored, by hand",
                 "fibonacci level=9 strategy=0", "reads.bam block 0"):
        assert name in taken, name
    for name, _, _, want in idc.hand_built_cases():                 # every hand-built valid stream but the one oddity
        assert want is None or name in taken or name == LONE, name


def test_hand_built_cases():
    """The hand-built streams are in the launch of everything under names of their own; each malformed one is refused by the
    twin, each valid one but the lone end-of-block code is taken (zlib's verdict on each: inflate_device_cases.py, at import)."""
    cases = idc.hand_built_cases()
    valid = [c for c in cases if c[3] is not None]
    print("hand-built cases: %d, valid %d, malformed %d" % (len(cases), len(valid), len(cases) - len(valid)))
    names = [c[0] for c in idc.valid_and_malformed_cases()]
    assert all(names.count(c[0]) == 1 for c in cases)
    assert all((c[3] is None) == c[0].startswith("bad: ") for c in cases) and LONE in {c[0] for c in valid}
    launch = idc.launches()[0]
    status, _ = idc.twin(launch)
    got = {c[0]: int(status[k]) for k, c in enumerate(launch.cases)}
    for name, raw, n, want in cases:
        assert got[name] == int(want is not None and name != LONE), name
    k = next(k for k, c in enumerate(launch.cases) if c[0] == LONE)
    assert not host_decoder_takes(*launch.cases[k][1:3])


def test_out_len_beyond_a_member_is_refused_unread():
    """65 537 bytes of output: the debug entries refuse the table as a whole and write nothing, neither a status nor a byte
    (the decoder's own refusal of such a stream, status 0, is what scripts/asan_inflate_wave.sh sees: it calls
    inflate_wave_host on the same launch with no entry in front)."""
    launch = idc.oversize_launch()
    out = launch.fresh_out()
    status = np.full(len(launch.cases), -7, np.int32)
    rc = _lib.load().npore_debug_inflate_wave_host(launch.inp.ctypes.data, launch.inp.size, launch.in_off.ctypes.data, launch.in_len.ctypes.data,
                                                   out.ctypes.data, out.size, launch.out_off.ctypes.data, launch.out_len.ctypes.data,
                                                   len(launch.cases), status.ctypes.data)
    assert rc != 0 and (status == -7).all() and (out == idc.FILL).all()


@pytest.mark.parametrize("launch", idc.mutant_launches(), ids=lambda l: l.name)
def test_twin_equals_zlib_on_single_bit_mutants(launch):
    """Every single-bit flip of the first 96 bytes of six small streams, each with the size zlib gives it: status 1 exactly
    where zlib accepts, with zlib's bytes -- but for a stream csrc/inflate.hpp declines too --, never a byte outside."""
    status, out = idc.twin(launch)
    assert launch.guards_intact(out), "wrote outside a block"
    accepted = sum(want is not None for _, _, _, want in launch.cases)
    print("mutants: %d, zlib accepts %d (%.3f)" % (len(launch.cases), accepted, accepted / len(launch.cases)))
    assert len(launch.cases) >= 3000 and 2 * accepted >= len(launch.cases)
    for k, (name, raw, n, want) in enumerate(launch.cases):
        assert status[k] in (0, 1), (name, status[k])
        if status[k] == 1:
            assert want is not None and launch.piece(out, k) == want, name
        elif want is not None:
            assert not host_decoder_takes(raw, n), name + ": csrc/inflate.hpp takes it, the twin does not"


@pytest.mark.parametrize("launch", idc.corrupt_launches(), ids=lambda l: l.name)
def test_twin_on_corrupt_streams(launch):
    """Never a byte outside the block, and whatever is accepted is what zlib gives for that size."""
    status, out = idc.twin(launch)
    assert launch.guards_intact(out), "wrote outside a block"
    n_fuzz = 0
    for k, (name, raw, n, want) in enumerate(launch.cases):
        if want is idc.FUZZ:
            n_fuzz += 1
            assert status[k] in (0, 1)
            if status[k] == 1:
                assert idc.zlib_inflate(raw, n) == launch.piece(out, k), name
        else:                                                       # the good neighbour, back to back with a corrupt one
            assert status[k] == 1 and launch.piece(out, k) == want, (k, name)
    assert n_fuzz == 200


def test_host_reader_on_hand_made_members(tmp_path):
    """The golden BAM's stream in some thirty small members of every kind (inflate_device_cases.mixed_members: the readers'
    own decoder declines the lone end-of-block ones, zlib takes them): the resident reader gives the stream back; with one
    member's CRC, stored bytes or dynamic header damaged the open call fails with words about BGZF, and the next one works."""
    stream = bam._bgzf_decompress(os.path.join(idc.GOLDEN, "data", "reads.bam"))
    members = idc.mixed_members(stream, 300, 800)
    kinds = [m[0] for m in members]
    assert sum(bool(m[2]) for m in members) >= 24 and all(kinds.count(k) >= 3 for k, _ in idc.MEMBER_KINDS) and kinds.count(idc.LONE_KIND) >= 4
    assert any(a == b == "empty" for a, b in zip(kinds, kinds[1:-1]))
    assert idc.twin_declines(members) == kinds.count(idc.LONE_KIND)
    lib = _lib.load()

    def opened(name, parts):
        path = str(tmp_path / name)
        open(path, "wb").write(b"".join(parts))
        return path, lib.npore_bam_open_mode(os.fsencode(path), 2, 1, None)

    def check_good():
        path, h = opened("mixed.bam", idc.member_bytes(members))
        assert h, _lib.last_error()
        raw = str(tmp_path / "mixed.raw")
        try:
            assert lib.npore_bam_n_records(h) == 10 and lib.npore_bam_dump_inflated(h, os.fsencode(raw)) == 0
        finally:
            lib.npore_bam_close(h)
        assert stream in open(raw, "rb").read()

    check_good()
    for what, (i, parts) in idc.damaged_files(members).items():
        _, h = opened("damaged.bam", parts)
        assert not h and "BGZF" in _lib.last_error(), (what, i, _lib.last_error())
        check_good()


def test_header_and_signatures_agree_on_the_new_names():
    text = open(HEADER).read()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
