"""ctypes wrapper for tests/model/libbam_walk.so (test infrastructure: the product's BAM reader, csrc/bam_reader.hpp,
compiled with plain g++ -- no ROCm include path, no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build(force=False):
    so = os.path.join(_HERE, "libbam_walk.so")
    csrc = os.path.join(_HERE, "..", "..", "npore_amd", "csrc")
    deps = [os.path.join(_HERE, "bam_walk.cpp")] + [
        os.path.join(csrc, f) for f in ("bam_reader.hpp", "hostio.hpp", "inflate.hpp", "crc32.hpp", "glue.hpp", "std_stream.hpp")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", so, deps[0], "-lz", "-lpthread"])
    return so


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(build())
        regions = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.bam_walk_select.argtypes = [C.c_char_p] + regions + [C.c_int64, C.c_void_p, C.c_int64]
        lib.bam_walk_select.restype = C.c_int64
        lib.bam_walk_one_pass.argtypes = [C.c_char_p] + regions + [C.c_int64, C.c_int, C.c_int, C.c_char_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.bam_walk_one_pass.restype = C.c_int64
        lib.bam_walk_last_error.restype = C.c_char_p
        lib.bam_walk_shares.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.bam_walk_shares.restype = C.c_int
        lib.bam_walk_refs_with_reads.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
        lib.bam_walk_refs_with_reads.restype = C.c_int
        _LIB = lib
    return _LIB


class WalkError(RuntimeError):
    pass


def _call(fn, path, regions, *args):
    """regions: [(ref_id, start, stop)]; returns the int64 offsets the call keeps"""
    lib = load()
    rid = np.array([r for r, _, _ in regions], np.int32)
    beg = np.array([s for _, s, _ in regions], np.int64)
    end = np.array([e for _, _, e in regions], np.int64)
    head = (os.fsencode(path), len(regions), rid.ctypes.data, beg.ctypes.data, end.ctypes.data)
    n = fn(*head, *args, None, 0)
    if n < 0:
        raise WalkError(f"{n}: {lib.bam_walk_last_error().decode()}")
    out = np.zeros(max(int(n), 1), np.int64)
    assert fn(*head, *args, out.ctypes.data, len(out)) == n
    return out[:n]


def select(path, regions, max_reads=0):
    """offsets in the inflated stream of the records npore_bam_select keeps on a resident handle"""
    return _call(load().bam_walk_select, path, regions, int(max_reads))


def shares(path, bai, world):
    """what bam_set_share decides for every rank of `world`: (rc[world], [(begin, end)] per rank -- offsets into the
    inflated stream, -1: the end of the file)"""
    lib = load()
    rc, span = np.zeros(world, np.int32), np.zeros(2 * world, np.int64)
    r = lib.bam_walk_shares(os.fsencode(path), os.fsencode(bai) if bai else None, int(world), rc.ctypes.data, span.ctypes.data)
    if r < 0:
        raise WalkError(f"{r}: {lib.bam_walk_last_error().decode()}")
    return rc.tolist(), [(int(span[2 * k]), int(span[2 * k + 1])) for k in range(world)]


def refs_with_reads(path):
    """the contigs that a one-pass handle on `path` says have reads"""
    lib = load()
    has = np.zeros(4096, np.uint8)
    n = lib.bam_walk_refs_with_reads(os.fsencode(path), has.ctypes.data, len(has))
    if n < 0:
        raise WalkError(f"{n}: {lib.bam_walk_last_error().decode()}")
    return {k for k in range(n) if has[k]}


def one_pass(path, regions, max_reads=0, rank=0, world=1, bai=None, batch_reads=7):
    """... of the records the one-pass walker keeps (window size: NPORE_BAM_WINDOW_BLOCKS)"""
    return _call(load().bam_walk_one_pass, path, regions, int(max_reads), int(rank), int(world),
                 os.fsencode(bai) if bai else None, int(batch_reads))
