#!/usr/bin/env python
"""Size of a --bam_compress huffman and a --bam_compress match file beside zlib on the same pieces: realigns a synthetic
ONT-like BAM (the generator of bench_realign.py) to BAM in the three modes, then deflates every 65 280-byte piece of the record stream with zlib at levels 1
and 6 on the host.  Prints one JSON line."""
import argparse
import json
import os
import struct
import sys
import tempfile
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from npore_amd import aln, bam, cfg     # noqa: E402
import bench_realign                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    sub, nps, _, _ = aln.load_default_tables()
    with tempfile.TemporaryDirectory() as tmp:
        bp, fa, clen = bench_realign.build_inputs(tmp, a.reads, 0, 10000, a.seed)
        regions = bench_realign.regions_of(clen)
        cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=regions, max_reads=0)
        ctx = aln.Context(sub, nps)
        sizes = {}
        for mode in ("none", "huffman", "match"):
            nb, nf = bam.NativeBam(bp, one_pass=True), bam.NativeFasta(fa)
            out = os.path.join(tmp, mode + ".bam")
            bam.create_bam_header(out, nb)
            nb.realign_sequential(ctx, nf, regions, out, batch_reads=1000, out_format="bam", bai=out + ".bai", compress=mode)
            sizes[mode] = os.path.getsize(out)
            nb.close(); nf.close()
        ctx.close()
        data = inflate_file(os.path.join(tmp, "huffman.bam"))
        assert data == inflate_file(os.path.join(tmp, "none.bam")) == inflate_file(os.path.join(tmp, "match.bam"))
        l_text, = struct.unpack_from("<i", data, 4)
        stream = data[bench_header_len(data, l_text):]
        z = {}
        for level in (1, 6):
            total = 0
            for p in range(0, len(stream), 0xFF00):
                c = zlib.compressobj(level, zlib.DEFLATED, -15)
                total += len(c.compress(stream[p:p + 0xFF00]) + c.flush()) + 26
            z[level] = total
        print(json.dumps({"what": "record stream of %d synthetic 10 kb reads, uniform qualities, cut every 65 280 bytes" % a.reads,
                          "stream_bytes": len(stream), "file_bytes_stored": sizes["none"], "file_bytes_huffman": sizes["huffman"],
                          "file_bytes_match": sizes["match"], "match_over_stored": round(sizes["match"] / sizes["none"], 4),
                          "members_bytes_zlib1": z[1], "members_bytes_zlib6": z[6],
                          "huffman_over_stored": round(sizes["huffman"] / sizes["none"], 4),
                          "zlib1_over_stored": round(z[1] / sizes["none"], 4), "zlib6_over_stored": round(z[6] / sizes["none"], 4)}))


def inflate_file(path):
    """The inflated bytes of a BGZF file, member by member along BSIZE (linear in the file's size)."""
    raw, out, p = open(path, "rb").read(), [], 0
    while p < len(raw):
        xlen, = struct.unpack_from("<H", raw, p + 10)
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        out.append(zlib.decompress(raw[p + 12 + xlen:p + bsize - 8], -15))
        p += bsize
    print("inflated", path, file=sys.stderr, flush=True)
    return b"".join(out)


def bench_header_len(data, l_text):
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, p)
        p += 8 + l_name
    return p


if __name__ == "__main__":
    main()
