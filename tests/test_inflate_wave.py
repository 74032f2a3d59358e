"""The host twin of the wave-per-stream DEFLATE decoder (csrc/inflate_wave.hpp, npore_debug_inflate_wave_host) against
zlib.decompressobj(-15) on the shared cases of inflate_device_cases.py: the code the gfx950 kernel runs, with the loop over
the lanes written out.  No GPU."""
import os
import re

import numpy as np
import pytest

from npore_amd import _lib
import inflate_device_cases as idc

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "npore_amd.h")
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


def test_header_and_signatures_agree_on_the_new_names():
    text = open(HEADER).read()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
