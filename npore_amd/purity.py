"""Gini purity of pileups (reference src/purity.py) straight from BAM records, counted on the GPU -- no pileup text, no
samtools.  The rule: csrc/purity_rec.hpp; the kernels: csrc/purity_kernels.hpp; the driver: npore_bam_purity.

    python -m npore_amd.purity --bams A [B ...] [--region ctg[:beg[-end]]] --out PREFIX

writes PREFIX{idx}.npy per BAM -- the array of (bases score, insertions score) per covered position that the reference
caches (src/purity.py:199), so its --plot_only can plot it -- and PREFIX_hist.json: per BAM the two 100-bin histograms
and the tallies, and for each pair of BAMs (2j, 2j+1) against the pair before it the summed counts and their ratios
(src/purity.py:100-124).  Plots stay out of scope.

Where this route differs from `samtools mpileup` on purpose: no depth cap (-d); no handling of overlapping mates; a `*`
entry takes the quality of the read base consumed last before its deletion; an entry with a letter outside ACGT (N
among them) is dropped instead of ending the column; inserted strings longer than 14 letters are compared by a 56-bit
hash (two different ones that collide at one position are merged); an insertion with no base entry to sit on (behind a
deletion, or leading the read) is not counted."""
import argparse
import json
import os
import re
import sys

import numpy as np

PURITY_TALLIES = ("records", "records_flagged", "records_refskip", "records_malformed", "insertions_without_entry",
                  "entries_ambiguous", "entries_lowq", "entries_counted", "star_entries", "insertions_counted",
                  "insertions_hashed", "positions_covered", "positions_too_deep", "windows", "batches", "kernel_ns")
N_BINS = 100


def scores_from_rows(rows):
    """float64 [covered positions, 2] from the integer rows (n, S_b, t, S_i): the two scores.  The exact sums of squares
    over n * n in one division -- the reference adds (c / n) ** 2 term by term, which differs in the last bits."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    rows = rows[(rows[:, 0] > 0) & (rows[:, 1] >= 0)]
    n2 = (rows[:, 0] * rows[:, 0]).astype(np.float64)
    return np.stack([rows[:, 1] / n2, rows[:, 3] / n2], axis=1)


def bin_of(S, n):
    """the integer-exact bin of S / n^2 (csrc/purity_rec.hpp pur_bin): the reference's int(x * 100 - 0.00001)"""
    num = 10 ** 7 * int(S) - int(n) * int(n)
    return 0 if num < 0 else num // (10 ** 5 * int(n) * int(n))


def purity_from_bam(ctx, bam, ranges, min_bq=13, exclude_flags=0x704, per_position=False):
    """The two 100-bin histograms of the pileups' Gini purity (bases, insertions) over the positions of `ranges`, counted
    from the BAM records on the GPU (npore_bam_purity).
    ctx: an aln.Context (an annotation-only one will do); bam: a path or a bam.NativeBam; ranges: [(contig, start, stop)],
    0-based and half-open -- clipped to their contigs and merged: a position is scored once.  A path is read in ONE PASS
    where the file is coordinate-sorted, else through the record index.
    Returns (base_hist, ins_hist, tallies) -- int64 [100] each and a dict of PURITY_TALLIES -- and with per_position also
    the integer rows int64 [P, 4] of (n, S_b, t, S_i) per merged position (contigs in header order; zeros where nothing
    is counted) and the scores float64 [covered positions, 2] computed from them on the host."""
    from . import _lib
    from .bam import NativeBam, OnePassUnsupported
    lib = _lib.load()

    def run(b):
        ids = {n: i for i, n in enumerate(b.references)}
        rid = np.array([ids.get(c, -1) for c, _, _ in ranges], np.int32)
        beg = np.array([s for _, s, _ in ranges], np.int64)
        end = np.array([e for _, _, e in ranges], np.int64)
        base_hist, ins_hist, tallies = np.zeros(N_BINS, np.int64), np.zeros(N_BINS, np.int64), np.zeros(16, np.int64)
        rows = None
        if per_position:
            rows = np.zeros((merged_positions(ranges, dict(zip(b.references, b.lengths)), b.references), 4), np.int64)
        rc = lib.npore_bam_purity(ctx.handle, b.handle, len(ranges), rid.ctypes.data, beg.ctypes.data, end.ctypes.data, int(min_bq),
                                  int(exclude_flags), base_hist.ctypes.data, ins_hist.ctypes.data,
                                  rows.ctypes.data if per_position else None, len(rows) if per_position else 0, tallies.ctypes.data)
        if rc == -5 and b.one_pass:
            raise OnePassUnsupported(_lib.last_error())
        if rc:
            raise RuntimeError(f"libnpore_amd: {rc} {_lib.last_error()}")
        out = (base_hist, ins_hist, dict(zip(PURITY_TALLIES, tallies.tolist())))
        return out + (rows, scores_from_rows(rows)) if per_position else out

    if isinstance(bam, NativeBam):
        return run(bam)
    if NativeBam.is_bgzf(bam) and os.environ.get("NPORE_BAM_ONE_PASS", "1") != "0":
        b = NativeBam(bam, one_pass=True)
        try:
            return run(b)
        except OnePassUnsupported:
            pass                             # (not coordinate-sorted: nothing was added, the indexed reader counts)
        finally:
            b.close()
    b = NativeBam(bam, share=False)
    try:
        return run(b)
    finally:
        b.close()


def merged_positions(ranges, lengths, order=None):
    """P: the positions of the ranges clipped to their contigs (lengths: {contig: length}) and merged"""
    total = 0
    for c in (order if order is not None else sorted({c for c, _, _ in ranges})):
        iv = sorted((max(0, s), min(e, lengths[c])) for cc, s, e in ranges if cc == c and c in lengths)
        iv = [(s, e) for s, e in iv if s < e]
        end = None
        for s, e in iv:
            if end is None or s > end:
                total += e - s
                end = e
            elif e > end:
                total += e - end
                end = e
    return total


def parse_region(region, references, lengths):
    """`--region` the way samtools reads it -- ctg, ctg:beg or ctg:beg-end, 1-based and inclusive, commas allowed in the
    numbers; a contig's name may itself hold colons -- as ranges [(contig, start, stop)], 0-based and half-open.
    None: every contig, whole."""
    size = dict(zip(references, lengths))
    if region is None:
        return [(c, 0, n) for c, n in zip(references, lengths)]
    if region in size:
        return [(region, 0, size[region])]
    m = re.fullmatch(r"(.+):([0-9,]+)(?:-([0-9,]*))?", region)
    if not m or m.group(1) not in size:
        raise ValueError(f"region '{region}': no such contig in the BAM header")
    ctg = m.group(1)
    beg = int(m.group(2).replace(",", ""))
    end = int(m.group(3).replace(",", "")) if m.group(3) else size[ctg]
    if beg < 1 or end < beg:
        raise ValueError(f"region '{region}': need 1 <= beg <= end")
    return [(ctg, beg - 1, min(end, size[ctg]))]


def pair_summary(hists):
    """src/purity.py:100-124: for every odd BAM index the counts of its histograms plus the BAM's before it; for each such
    pair after the first the ratio rows against the pair before (0 where either count is 0).
    hists: [(base_hist, ins_hist)] per BAM."""
    out, prev = [], None
    for j in range(len(hists) // 2):
        base = [int(a) + int(b) for a, b in zip(hists[2 * j][0], hists[2 * j + 1][0])]
        ins = [int(a) + int(b) for a, b in zip(hists[2 * j][1], hists[2 * j + 1][1])]
        entry = {"bams": [2 * j, 2 * j + 1], "base_counts": base, "ins_counts": ins}
        if prev is not None:
            entry["base_ratio"] = [x / y if x and y else 0 for x, y in zip(base, prev[0])]
            entry["ins_ratio"] = [x / y if x and y else 0 for x, y in zip(ins, prev[1])]
        out.append(entry)
        prev = (base, ins)
    return out


def argparser():
    p = argparse.ArgumentParser(prog="python -m npore_amd.purity", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--bams", nargs="+", required=True,
                   help="BAMs whose pileups' Gini purity is computed; pairs (2j, 2j+1) are summed and compared with the pair "
                        "before (the reference: baseline hap1, baseline hap2, realigned hap1, realigned hap2)")
    p.add_argument("--region", type=str, help="ctg[:beg[-end]], 1-based and inclusive like samtools; default: everything")
    p.add_argument("--out", default="out", help="output prefix")
    p.add_argument("--min_bq", type=int, default=13, help="entries of lower base quality are dropped (mpileup -Q)")
    p.add_argument("--exclude_flags", type=lambda x: int(x, 0), default=0x704, help="records with one of these flag bits are left out")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--bam_inflate", choices=("host", "device"), default="host",
                   help="one-pass reader: the BAMs' BGZF blocks are inflated on the CPU threads, or on the GPU, one wave per block; "
                        "the histograms are the same")
    p.add_argument("--max_score_positions", type=int, default=50_000_000,
                   help="PREFIX{idx}.npy (the per-position scores) is written only for regions of at most this many positions")
    return p


def main(argv=None):
    from . import aln
    from .bam import NativeBam
    args = argparser().parse_args(argv)
    ctx = aln.Context(None, None, max_n=6, max_l=100, device=args.device)
    ctx.set("device_inflate", args.bam_inflate == "device")
    if args.bam_inflate == "device" and os.environ.get("NPORE_BAM_ONE_PASS", "1") == "0":
        print("    (--bam_inflate device has no effect: the indexed reader inflates on the host)")
    report, hists = {"bams": []}, []
    try:
        for idx, path in enumerate(args.bams):
            h = NativeBam(path, share=False)
            try:
                ranges = parse_region(args.region, h.references, h.lengths)
                n_pos = merged_positions(ranges, dict(zip(h.references, h.lengths)), h.references)
            finally:
                h.close()
            want_scores = n_pos <= args.max_score_positions
            print(f"> computing purity for {path}")
            res = purity_from_bam(ctx, path, ranges, args.min_bq, args.exclude_flags, per_position=want_scores)
            if want_scores:
                np.save(f"{args.out}{idx}", res[4])
            else:
                print(f"    {args.out}{idx}.npy skipped: {n_pos} positions, more than --max_score_positions {args.max_score_positions}")
            hists.append((res[0], res[1]))
            report["bams"].append({"path": path, "base_hist": res[0].tolist(), "ins_hist": res[1].tolist(), "tallies": res[2]})
    finally:
        ctx.close()
    report["pairs"] = pair_summary(hists)
    with open(f"{args.out}_hist.json", "w") as fh:
        json.dump(report, fh)
    return 0


if __name__ == "__main__":
    sys.exit(main())
