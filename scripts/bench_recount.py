#!/usr/bin/env python3
"""Throughput of the recount of the confusion matrices (`realign --recalc_cms`), device route against text route.

The input is the synthetic ONT-like BAM of scripts/bench_realign.py (reads of `--ref-len` bases laid end to end, CIGARs of
=, X, I and D, qualities one uniform draw per base over phred 0 ... 93, so the default quality bound of 13 drops about one
base in seven).  One JSON line:
  device_reads_per_s     bam.confusion_from_bam file to file: open, one pass over the BGZF file, the planes and the counting
                         kernels on the GPU, the matrices back (second of two runs; the first is reported as *_first);
  kernel_ms_per_batch    the counting kernels alone, by HIP events, per batch of `--batch` reads (default 4 000);
  text_reads_per_s       the text route on `--text-reads` reads of the same generator (the first reads of the file, written
                         as a file of their own, cut into ranges of the same --chunk-width): this repository's Python pileup
                         writer (tests/model/cms_model.py) on `--procs` processes, then bam.calc_confusion_matrices
                         (npore_confusion_counts on all cores).  A different, much smaller file and a stand-in for samtools:
                         the two reads/s figures are NOT comparable.
`samtools` is not installed where this is measured, so the text route cannot be timed with the real `samtools mpileup`
in front of it; the Python writer stands in for it and is far slower than samtools would be -- the text figure is a
lower bound of what that route can do, not a measurement of samtools.

    python scripts/bench_recount.py [--reads 16000] [--ref-len 10000] [--batch 4000] [--text-reads 160] [--out profiles/recount_line.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np


def _text_job(job):
    """Worker: the pileup lines of some of the ranges of the small file, from the reads that overlap them (the reads lie end to end)."""
    path, fa, ranges, ref_len, min_bq, flags = job
    from model import cms_model
    from npore_amd import bam
    f = bam.BamFile(path)
    refs = bam.read_fasta(fa)
    k0, k1 = min(s for _, s, _ in ranges) // ref_len, (max(e for _, _, e in ranges) + ref_len - 1) // ref_len
    lines, tallies = cms_model.write_pileups(f.records[k0:k1], f.references, refs, ranges, 6, 100, min_bq, flags)
    return ranges, lines, int(tallies["entries_counted"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16000)
    ap.add_argument("--ref-len", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=4000)
    ap.add_argument("--chunk-width", type=int, default=100000)
    ap.add_argument("--text-reads", type=int, default=160)
    ap.add_argument("--procs", type=int, default=max(1, min(16, len(os.sched_getaffinity(0)))))
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--inflate", choices=("host", "device"), default="host",
                    help="where the one-pass reader inflates the BAM's BGZF blocks (Context.set device_inflate)")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    import bench_realign
    from npore_amd import aln, bam, cfg
    from npore_amd.bed import get_ranges
    tmp_ctx = tempfile.TemporaryDirectory(dir=a.tmp) if not a.tmp or not os.path.exists(os.path.join(a.tmp, "reads.bam")) else None
    tmp = tmp_ctx.name if tmp_ctx else a.tmp
    t0 = time.perf_counter()
    bp, fa, clen = bench_realign.build_inputs(tmp, a.reads, 0, a.ref_len, a.seed, procs=a.procs)
    gen_s = time.perf_counter() - t0
    ranges = get_ranges(bench_realign.regions_of(clen), a.chunk_width)
    res = {"bench": "recount", "reads": a.reads, "ref_len": a.ref_len, "batch": a.batch, "chunk_width": a.chunk_width, "ranges": len(ranges),
           "bam_mb": round(os.path.getsize(bp) / 1e6, 1), "generate_s": round(gen_s, 1), "cpus": a.procs}
    ctx = aln.Context(None, None, max_n=6, max_l=100, device=0)
    ctx.set("cms_batch_reads", a.batch)
    ctx.set("device_inflate", a.inflate == "device")
    res["inflate"] = a.inflate
    for tag in ("_first", ""):
        t0 = time.perf_counter()
        subs, nps, inss, dels, t = bam.confusion_from_bam(ctx, bp, fa, ranges)
        wall = time.perf_counter() - t0
        res["device_wall_s" + tag] = round(wall, 3)
        res["device_reads_per_s" + tag] = round(t["records"] / wall, 1)
    res.update(records=t["records"], entries_counted=t["entries_counted"], entries_lowq=t["entries_lowq"],
               adjacent_indels=t["adjacent_indels"], batches=t["batches"],
               kernel_ms_per_batch=round(t["kernel_ns"] / 1e6 / max(1, t["batches"]), 3),
               kernel_ms_total=round(t["kernel_ns"] / 1e6, 3))
    # ---- the text route on the first reads of the same generator
    n_text = min(a.text_reads, a.reads)
    small = os.path.join(tmp, "small")
    os.makedirs(small, exist_ok=True)
    sbp, sfa, sclen = bench_realign.build_inputs(small, n_text, 0, a.ref_len, a.seed, procs=a.procs)
    import multiprocessing as mp
    # the same kind of ranges as the device route's (--chunk-width), dealt to the processes in contiguous groups
    sranges = get_ranges(bench_realign.regions_of(sclen), a.chunk_width)
    per = (len(sranges) + a.procs - 1) // a.procs
    jobs = [(sbp, sfa, sranges[k:k + per], a.ref_len, 13, 0x704) for k in range(0, len(sranges), per)]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(a.procs) as pool:
        parts = pool.map(_text_job, jobs)
    write_s = time.perf_counter() - t0
    refs = bam.read_fasta(sfa)
    cfg.args = argparse.Namespace(max_n=6, max_l=100)
    t0 = time.perf_counter()
    total = None
    for rgs, lines, _ in parts:
        for rg, ln in zip(rgs, lines):
            r = bam.calc_confusion_matrices(rg, pileups=ln, refs=refs)
            total = r if total is None else tuple(x + y for x, y in zip(total, r))
    count_s = time.perf_counter() - t0
    small_dev = bam.confusion_from_bam(ctx, sbp, sfa, [rg for rgs, _, _ in parts for rg in rgs])
    ctx.close()
    res.update(text_reads=n_text, text_write_s=round(write_s, 3), text_count_s=round(count_s, 3),
               text_reads_per_s=round(n_text / (write_s + count_s), 2),
               text_equals_device=bool(all(np.array_equal(x, y) for x, y in zip(total, small_dev[:4]))),
               text_route="python pileup writer on %d processes + npore_confusion_counts; samtools is not installed" % a.procs)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if tmp_ctx:
        tmp_ctx.cleanup()


if __name__ == "__main__":
    main()
