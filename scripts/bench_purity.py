#!/usr/bin/env python3
"""Throughput of the Gini purity of pileups from BAM records (`python -m npore_amd.purity`), beside the recount of the
confusion matrices on the same file.

The input is the generator and the file of scripts/bench_recount.py (the synthetic ONT-like BAM of scripts/bench_realign.py:
`--reads` reads of `--ref-len` bases laid end to end).  purity.purity_from_bam and bam.confusion_from_bam -- existing code
on the same reader and staging -- run alternating, `--repeats` times each, after one warm-up run of each.  One JSON line:
  purity_reads_per_s      purity_from_bam file to file (open, one pass over the BGZF file, the kernels, the histograms
                          back), median of the repeats; purity_wall_s: every repeat;
  purity_kernel_ms_per_batch  the purity kernels alone (records kernel and the windows' ends), by HIP events, per batch;
  purity_host_ms_per_batch    what is left of the wall time per batch: the host's inflation, gate and staging;
  confusion_*             the same figures of confusion_from_bam;
  kernels_exceed_host     the finding to look for: true if the kernels' time per batch is above the host's.

    python scripts/bench_purity.py [--reads 8000] [--ref-len 10000] [--batch 4000] [--repeats 3] [--out profiles/purity_line.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8000)
    ap.add_argument("--ref-len", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=4000)
    ap.add_argument("--chunk-width", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=int, default=0, help="purity_window (0: the default)")
    ap.add_argument("--procs", type=int, default=max(1, min(16, len(os.sched_getaffinity(0)))))
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--inflate", choices=("host", "device"), default="host",
                    help="where the one-pass reader inflates the BAM's BGZF blocks (Context.set device_inflate)")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    import bench_realign
    from npore_amd import aln, bam, purity
    from npore_amd.bed import get_ranges
    tmp_ctx = tempfile.TemporaryDirectory(dir=a.tmp) if not a.tmp or not os.path.exists(os.path.join(a.tmp, "reads.bam")) else None
    tmp = tmp_ctx.name if tmp_ctx else a.tmp
    bp, fa, clen = bench_realign.build_inputs(tmp, a.reads, 0, a.ref_len, a.seed, procs=a.procs)
    regions = bench_realign.regions_of(clen)
    cms_ranges = get_ranges(regions, a.chunk_width)
    res = {"bench": "purity", "reads": a.reads, "ref_len": a.ref_len, "batch": a.batch, "bam_mb": round(os.path.getsize(bp) / 1e6, 1),
           "positions": purity.merged_positions(regions, {c: e for c, _, e in regions}), "cpus": a.procs}
    ctx = aln.Context(None, None, max_n=6, max_l=100, device=0)
    ctx.set("cms_batch_reads", a.batch)
    ctx.set("device_inflate", a.inflate == "device")
    res["inflate"] = a.inflate
    if a.window:
        ctx.set("purity_window", a.window)
    runs = {"purity": [], "confusion": []}
    tall = {}
    for rep in range(a.repeats + 1):                      # (the first of each is the warm-up: allocations, the FASTA's upload)
        for name in ("purity", "confusion"):
            t0 = time.perf_counter()
            if name == "purity":
                t = purity.purity_from_bam(ctx, bp, regions)[2]
            else:
                t = bam.confusion_from_bam(ctx, bp, fa, cms_ranges)[4]
            wall = time.perf_counter() - t0
            if rep:
                runs[name].append(wall)
            tall[name] = t
    ctx.close()
    for name in ("purity", "confusion"):
        t, wall = tall[name], statistics.median(runs[name])
        kernel_ms = t["kernel_ns"] / 1e6
        res[name + "_wall_s"] = [round(w, 4) for w in runs[name]]
        res[name + "_reads_per_s"] = round(t["records"] / wall, 1)
        res[name + "_batches"] = t["batches"]
        res[name + "_kernel_ms_total"] = round(kernel_ms, 3)
        res[name + "_kernel_ms_per_batch"] = round(kernel_ms / max(1, t["batches"]), 3)
        res[name + "_host_ms_per_batch"] = round((wall * 1e3 - kernel_ms) / max(1, t["batches"]), 3)
    t = tall["purity"]
    res.update(records=t["records"], entries_counted=t["entries_counted"], star_entries=t["star_entries"], entries_lowq=t["entries_lowq"],
               insertions_counted=t["insertions_counted"], insertions_hashed=t["insertions_hashed"], positions_covered=t["positions_covered"],
               windows=t["windows"], kernels_exceed_host=bool(res["purity_kernel_ms_per_batch"] > res["purity_host_ms_per_batch"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if tmp_ctx:
        tmp_ctx.cleanup()


if __name__ == "__main__":
    main()
