#!/usr/bin/env python
"""The device DEFLATE decoder alone (csrc/inflate_kernels.hpp inflate_blocks_kernel, one wave per BGZF block) on the blocks of
the file scripts/bench_realign.py generates (per-base qualities: literal-heavy): GB/s of inflated bytes per launch of 256,
1 024, 4 096 and 8 192 blocks.  The time is the wall of npore_debug_inflate_device minus the same call on ZERO-length
streams of the same buffers (the copies up and down and the launch), so it is the kernel's, to the copies' jitter;
npore_bam_inflate_info[4] of a file run (bench_recount.py --inflate device) has the kernel's time by events.
Prints one JSON line.  The host decoder on one core, for comparison: scripts/microbench/inflate_bench.cpp."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))


def blocks_of(path):
    raw, p, out = open(path, "rb").read(), 0, []
    while p < len(raw):
        xlen = struct.unpack_from("<H", raw, p + 10)[0]
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        isize = struct.unpack_from("<I", raw, p + bsize - 4)[0]
        if isize:
            out.append((raw[p + 12 + xlen:p + bsize - 8], isize))
        p += bsize
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=40000)
    ap.add_argument("--ref-len", type=int, default=10000)
    ap.add_argument("--sizes", default="256,1024,4096,8192")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--procs", type=int, default=max(1, min(16, len(os.sched_getaffinity(0)))))
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    import bench_realign
    from npore_amd import _lib, aln
    tmp_ctx = tempfile.TemporaryDirectory(dir=a.tmp) if not a.tmp or not os.path.exists(os.path.join(a.tmp, "reads.bam")) else None
    tmp = tmp_ctx.name if tmp_ctx else a.tmp
    bp, _, _ = bench_realign.build_inputs(tmp, a.reads, 0, a.ref_len, a.seed, procs=a.procs)
    blocks = blocks_of(bp)
    lib = _lib.load()
    ctx = aln.Context(None, None, max_n=6, max_l=100, device=0)
    res = {"bench": "inflate_device", "bam_mb": round(os.path.getsize(bp) / 1e6, 1), "blocks_in_file": len(blocks), "launches": []}
    for n in (int(x) for x in a.sizes.split(",")):
        use = [blocks[k % len(blocks)] for k in range(n)]
        in_len = np.array([len(b[0]) for b in use], np.int64)
        out_len = np.array([b[1] for b in use], np.int64)
        in_off = np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.int64)
        out_off = np.concatenate(([0], np.cumsum(out_len)[:-1])).astype(np.int64)
        inp = np.frombuffer(b"".join(b[0] for b in use), np.uint8)
        out = np.zeros(int(out_len.sum()), np.uint8)
        status = np.zeros(n, np.int32)
        zero = np.zeros(n, np.int64)

        def call(il, ol):
            t0 = time.perf_counter()
            rc = lib.npore_debug_inflate_device(ctx.handle, inp.ctypes.data, inp.size, in_off.ctypes.data, il.ctypes.data, out.ctypes.data,
                                                out.size, out_off.ctypes.data, ol.ctypes.data, n, status.ctypes.data)
            assert rc == 0, _lib.last_error()
            return time.perf_counter() - t0

        call(in_len, out_len)                                         # warm-up: the buffers' first touch
        assert status.all(), "a block was declined"
        full = [call(in_len, out_len) for _ in range(a.repeats)]
        empty = [call(zero, zero) for _ in range(a.repeats)]
        kernel_s = max(1e-9, statistics.median(full) - statistics.median(empty))
        res["launches"].append({"blocks": n, "inflated_mb": round(out.size / 1e6, 1), "compressed_mb": round(inp.size / 1e6, 1),
                                "call_s": [round(x, 4) for x in full], "copies_s": [round(x, 4) for x in empty],
                                "kernel_s": round(kernel_s, 4), "inflated_gb_per_s": round(out.size / 1e9 / kernel_s, 3)})
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if tmp_ctx:
        tmp_ctx.cleanup()


if __name__ == "__main__":
    main()
