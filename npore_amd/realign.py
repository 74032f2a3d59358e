#!/usr/bin/env python3
"""realign.py -- BAM in, SAM (or, --out_format bam, indexed BAM) out, same flags as reference src/realign.py:15-71.

    python -m npore_amd.realign --bam reads.bam --ref ref.fasta --out_prefix out \\
                                [--stats_dir DIR] [--contig ...] [--max_reads N] ...

The per-read DP runs on an MI355X through libnpore_amd.so; reads are handed to
it in batches instead of one align() call per pool worker
(src/realign.py:110-114).  Several GPUs: launch one process per GPU with
`python -m torch.distributed.run --nproc-per-node N -m npore_amd.realign ...`;
rank k realigns reads k, k+N, ... into its own part file and rank 0 appends
the parts to the SAM (record order is arbitrary in the reference too).
--recalc_cms recounts the confusion matrices with `samtools mpileup` like the reference (bam.get_confusion_matrices), or with
--cms_source bam straight from the BAM records on the GPU (bam.confusion_from_bam); --plot is out of scope.
"""
import argparse
import os
import sys
from time import perf_counter

import numpy as np

from . import aln, bam as bam_mod, cfg, dist as dist_mod


def argparser():
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--bam", required=True, help="Input BAM to be realigned.")
    parser.add_argument("--ref", required=True, help="Input reference FASTA.")
    parser.add_argument("--out_prefix", required=True, help="Output SAM file prefix.")
    parser.add_argument("--contig", type=str, help="Single contig to realign (with --contig_beg/--contig_end).")
    parser.add_argument("--contig_beg", type=int, help="Start of realigned region.")
    parser.add_argument("--contig_end", type=int, help="End of realigned region.")
    parser.add_argument("--contigs", type=str, help="Comma-separated contigs to realign.")
    parser.add_argument("--max_reads", type=int, default=0, help="Limit on realigned reads (0 = all).")
    parser.add_argument("--bed", type=str, help="BED file of regions to realign.")
    parser.add_argument("--max_n", type=int, default=6, help="Maximum n-polymer period considered.")
    parser.add_argument("--max_l", type=int, default=100, help="Maximum n-polymer repeat count considered.")
    parser.add_argument("--chunk_width", type=int, default=100000, help="(confusion-matrix recalculation only)")
    parser.add_argument("--stats_dir", default=None,
                        help="Directory with subs/nps/inss/dels _cm.npy (default: the shipped guppy5_stats; with --recalc_cms the "
                             "recounted matrices are written here, default ./stats as in the reference).")
    parser.add_argument("--plot", action="store_true", help="(not supported in this build)")
    parser.add_argument("--recalc_cms", action="store_true",
                        help="Recount the confusion matrices from the BAM instead of loading them (--cms_source: `samtools mpileup`, or the records themselves).")
    parser.add_argument("--recalc_exit", action="store_true", help="Exit after --recalc_cms.")
    parser.add_argument("--cms_source", choices=("mpileup", "bam"), default="mpileup",
                        help="--recalc_cms: `mpileup` reads the text of `samtools mpileup` like the reference; `bam` counts straight "
                             "from the BAM records on the GPU, without samtools.  `bam` is position-true (a position nobody covers "
                             "adds nothing, where the text route shifts), has no depth cap (mpileup -d) and no handling of "
                             "overlapping mates, and leaves out INDELs that follow another INDEL.")
    parser.add_argument("--cms_min_bq", type=int, default=13, help="--cms_source bam: bases below this quality are not counted (mpileup -Q).")
    parser.add_argument("--cms_exclude_flags", type=int, default=0x704,
                        help="--cms_source bam: records with one of these flag bits are left out (mpileup's UNMAP, SECONDARY, QCFAIL, DUP).")
    # additions
    parser.add_argument("--batch_reads", type=int, default=4000, help="Reads per GPU batch (4 000 reads of 10 kb fill the GPU once at the default band, Context.round_chunks; file to file 6 000 - 8 000 measured 5 - 7 %% faster at twice the device memory: 49 GB of traceback words per batch in flight, three in flight).")
    parser.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")), help="HIP device.")
    parser.add_argument("--out_format", choices=("sam", "bam"), default="sam",
                        help="`sam`: the text, OUT_PREFIX.sam.  `bam`: OUT_PREFIX.bam, the same records in binary (built on the GPU in "
                             "the default pipeline) in uncompressed BGZF members, with OUT_PREFIX.bam.bai when they go out in "
                             "coordinate order -- what `samtools view -u` and `samtools index` would make of the SAM.")
    parser.add_argument("--bam_compress", choices=("none", "huffman", "match"), default="none",
                        help="--out_format bam: `none`, stored BGZF members; `huffman`, every member one dynamic-Huffman DEFLATE block "
                             "of literals (no match search); `match`, of literals and length/distance pairs (a hash of four bytes, a "
                             "greedy parse) wherever that is smaller.  Both are coded on the GPU in the default pipeline.  The records, "
                             "the cuts and the index's meaning are the same.")
    parser.add_argument("--records", choices=("reference", "full"), default="reference",
                        help="--out_format bam: `reference`, each record is the reference's SAM line in binary (clips cut off, mate "
                             "fields cleared, HP the only tag); `full`, the input record with only what the realignment changes "
                             "replaced: clipped bases, mate fields and tags stay (NM MD cs de dv dropped), NM recounted on the GPU.")
    parser.add_argument("--md", action="store_true",
                        help="--records full: write the MD tag behind the recounted NM, built on the GPU from the final CIGAR and the "
                             "bases NM is counted on (`samtools calmd`'s text, but an IUPAC letter other than N counts as a mismatch "
                             "and prints as N, as it does in NM).  Without it the records carry no MD: the input's is stale.")
    parser.add_argument("--cs", choices=("short", "long"), default=None,
                        help="--records full: write minimap2's cs tag behind NM (and MD), built on the GPU from the final CIGAR and "
                             "the bases NM is counted on: `short`, `:<n>` for matches, `long`, `=<LETTERS>`.  As in NM, an IUPAC "
                             "letter other than N counts as a mismatch (minimap2 leaves ambiguous bases out).  Without it the "
                             "records carry no cs: the input's is stale.")
    parser.add_argument("--de", action="store_true",
                        help="--records full: write minimap2's de tag (gap-compressed per-base divergence, a float) behind cs, "
                             "counted on the GPU in the same walk.  Without it the records carry no de: the input's is stale.")
    parser.add_argument("--eqx", action="store_true",
                        help="--records full: write the final CIGAR with `=` and `X` in the place of `M`, as `minimap2 --eqx` does, "
                             "split on the GPU from the final CIGAR and the bases NM is counted on: X where NM counts a mismatch "
                             "(an IUPAC letter other than N included), = elsewhere; NM, MD, cs and de do not change.  More than "
                             "65 535 operations, which this form reaches sooner, go to the CG tag.  Without it the CIGAR has M.")
    parser.add_argument("--oc", action="store_true",
                        help="--records full: write the input's CIGAR as the OC:Z tag on every read whose alignment the run changed, "
                             "as GATK's IndelRealigner does -- every word as it stood, clips included; decided and written on the "
                             "GPU.  A read is unchanged when its input CIGAR, with = and X read as M, words of length 0 dropped and "
                             "neighbouring words of one kind merged, is its final CIGAR.  An OC the input carried is dropped, so an "
                             "unchanged read has none.  The position never changes: no OP is written.  Without it no OC is "
                             "written and an input's OC stays as it came.")
    parser.add_argument("--pass_through", action="store_true",
                        help="--records full: write the records the realigner does not take -- secondary (0x100), supplementary "
                             "(0x800) and placed but unmapped (0x4) ones -- as they came, every tag included, in their place among "
                             "the realigned records, so that the output holds the records of the input; they count towards "
                             "--max_reads.  Still left out: unplaced records (no reference), and reads whose CIGAR and sequence "
                             "disagree (reported, as without the flag).  Without it such records are dropped, as the reference does.")
    parser.add_argument("--bam_inflate", choices=("host", "device"), default="host",
                        help="One-pass reader: where the input BAM's BGZF blocks are inflated: `host`, on the CPU threads; `device`, "
                             "on the GPU, one wave per block (also for --recalc_cms --cms_source bam).  The output is the same.  "
                             "During the realignment the inflate kernel takes turns with the fill kernel.")
    parser.add_argument("--python_io", action="store_true",
                        help="Use the pure-Python BAM reader / SAM writer (the restatement the native one is tested against).")
    return parser


def main():
    if cfg.args.plot:
        print("\nERROR: --plot is not available in npore_amd (matplotlib reports are out of scope).")
        sys.exit(1)
    native = not cfg.args.python_io
    # what the run writes, said once (bam.OutputSpec): a rank's part has its own index sidecar (part-relative offsets, merged by
    # dist.gather_bam_parts), and the EOF member ends the whole file, not a part
    rank, world, _ = dist_mod.world()
    fmt = getattr(cfg.args, "out_format", "sam")
    as_bam = fmt == "bam"
    final_sam = f"{cfg.args.out_prefix}.{fmt}"
    out_sam = final_sam if world == 1 else f"{cfg.args.out_prefix}.part{rank}.{fmt}"
    try:
        spec = bam_mod.OutputSpec.from_args(cfg.args, bai=out_sam + ".bai" if as_bam else None, eof=world == 1)
    except bam_mod.OutputSpecError as e:
        print(f"\nERROR: {e.cli}")
        sys.exit(1)
    if spec.records == "full" and not native:
        print("\nERROR: --records full is written by the library's file pipeline: not with --python_io.")
        sys.exit(1)
    # one process per GPU: the host stages of a rank use its share of the node's cores, and the BAM is inflated
    # once per node (local rank 0; the other ranks map its copy, bam.NativeBam)
    threads = dist_mod.host_threads_per_rank() if int(os.environ.get("LOCAL_WORLD_SIZE", "1")) > 1 else 0
    print("> reading reference")
    ref_seqs = bam_mod.NativeFasta(cfg.args.ref) if native else bam_mod.read_fasta(cfg.args.ref)
    print("> selecting BAM regions")
    # One process, the native reader, batches written by the library: ONE PASS over the BAM (bam.NativeBam.realign_sequential:
    # no record index, every block inflated once, ingest overlapped with the GPU) -- the way the reference itself reads,
    # a generator over bam.fetch() (src/bam.pyx:18-47).  Several ranks, or regions / a file order that rule it out: the
    # indexed reader.
    # Several ranks on one file: each walks a contiguous stretch of the record stream in one pass, cut at record starts taken
    # from the .bai linear index (bam.NativeBam.set_share) -- the counterpart of the reference feeding all its workers from
    # one sequential read (src/bam.pyx:18-47, src/realign.py:110-114); without a .bai, or with --max_reads (the ranks cannot
    # know how many reads the others keep), the indexed reader.  The index is another file and may be stale or somebody
    # else's, so set_share locates and checks ALL the cuts on every rank (member starts, record starts: csrc/bam_reader.hpp
    # bam_set_share) -- the choice depends on the two files, the flags and the number of ranks, never on the rank: every
    # rank makes the same one.  (A rank that fell back on its own would take a share of ALL reads while the others walk
    # their stretches: reads twice, reads missing, no error.)
    # The .bai also says which contigs have reads, and the default regions leave out the others: the one-pass walk checks
    # that claim against the records it meets, and a record on such a contig ends the run (bam.StaleIndex).
    one_pass = (native and cfg.args.batch_reads > 0 and not getattr(cfg.args, "bed", None)
                and os.environ.get("NPORE_BAM_ONE_PASS", "1") != "0" and bam_mod.NativeBam.is_bgzf(cfg.args.bam)
                and (world == 1 or (not cfg.args.max_reads and bam_mod.NativeBam.bai_path(cfg.args.bam) is not None)))
    bam = bam_mod.NativeBam(cfg.args.bam, threads=threads, one_pass=one_pass) if native else bam_mod.BamFile(cfg.args.bam)
    if one_pass and world > 1:
        try:
            bam.set_share(rank, world)
        except bam_mod.OnePassUnsupported as e:
            print(f"    ({e}: taking the indexed reader)")
            bam.close()
            one_pass = False
            bam = bam_mod.NativeBam(cfg.args.bam, threads=threads)
    if getattr(cfg.args, "bam_inflate", "host") == "device" and not one_pass:
        print("    (--bam_inflate device has no effect: " + ("--python_io" if not native else "the indexed reader") + " inflates on the host)")
    bam_mod.get_bam_regions(bam, ref_seqs)

    if cfg.args.recalc_cms:              # src/realign.py:92-95 + src/bam.pyx:166-200
        # (the pileup counter slices the contigs: the native reader only serves lengths, so take the sequences too)
        cfg.args.refs = bam_mod.NativeFastaSeqs(cfg.args.ref) if native else ref_seqs
        subs, nps, inss, dels = bam_mod.get_confusion_matrices()
        print("> calculating score matrices")
        cfg.args.sub_scores, cfg.args.np_scores, cfg.args.ins_scores, cfg.args.del_scores = \
            aln.calc_score_matrices(subs, nps, inss, dels)
    else:
        print("> calculating score matrices")
        cfg.args.sub_scores, cfg.args.np_scores, cfg.args.ins_scores, cfg.args.del_scores = \
            aln.load_default_tables(cfg.args.stats_dir)

    if world > 1 and not native:
        print("\nERROR: --python_io runs on one GPU only.")
        sys.exit(1)
    if as_bam and native and cfg.args.batch_reads <= 0:
        print("\nERROR: --out_format bam is written by the library's file pipeline: --batch_reads must be positive.")
        sys.exit(1)
    print(f"> creating output {fmt.upper()}")
    if rank == 0:
        (bam_mod.create_bam_header if as_bam else bam_mod.create_header)(final_sam, bam)
    if world > 1:
        open(out_sam, "w").close()
    gather = dist_mod.gather_bam_parts if as_bam else dist_mod.gather_parts

    print("> extracting read data from BAM")
    start = perf_counter()
    n_dev = max(aln.device_count(), 1)
    ctx = aln.Context(cfg.args.sub_scores, cfg.args.np_scores, device=cfg.args.device % n_dev)
    ctx.set("device_inflate", getattr(cfg.args, "bam_inflate", "host") == "device")
    n = 0
    done = False
    if native and one_pass:
        print("> computing individual read realignments")
        header_bytes = os.path.getsize(out_sam)
        try:
            n, bad, _ = bam.realign_sequential(ctx, ref_seqs, cfg.args.regions, out_sam, batch_reads=cfg.args.batch_reads,
                                               max_reads=cfg.args.max_reads, threads=threads, output=spec)
            for k, st in bad:
                print(f"\nERROR: read #{k} of the selected reads: " +
                      ("CIGAR does not match sequence lengths; skipped." if st & 32 else f"inconsistent traceback (status {st})"))
            done = True
        except bam_mod.StaleIndex as e:
            # the regions came from the index's word on which contigs have reads: no reader can mend that here
            print(f"\nERROR: {e}.")
            sys.exit(1)
        except bam_mod.OnePassUnsupported as e:
            if world > 1 and "regions" not in str(e) and "region per contig" not in str(e):
                # found in the DATA of one rank's stretch (a file that is not sorted): the other ranks may not have seen it,
                # and a rank that changed readers on its own would deal the reads differently from the rest
                print(f"\nERROR: {e}.")
                sys.exit(1)
            print(f"    ({e}: taking the indexed reader)")
            with open(out_sam, "r+b") as fh:
                fh.truncate(header_bytes)
            bam.close()
            bam = bam_mod.NativeBam(cfg.args.bam, threads=threads)
    if done:
        bam.close()
        ref_seqs.close()
        if world > 1:
            n = gather(final_sam, cfg.args.out_prefix, n)
    elif native:
        idx = bam.select(cfg.args.regions, cfg.args.max_reads, pass_mask=spec.pass_mask)
        # reads are independent: dealt by index, no data-path collective.  A resident BAM is dealt round-robin; a
        # STREAMED one in contiguous shares, so that a rank only ever inflates the blocks that hold its own reads
        # (BAM output: contiguous shares always -- the parts in rank order are then in file order, sorted and indexable)
        if (bam.streamed or as_bam) and world > 1:
            per = (len(idx) + world - 1) // world
            idx = idx[rank * per:(rank + 1) * per]
        else:
            idx = idx[rank::world]
        print("> computing individual read realignments")
        n += bam_mod.realign_native(ctx, bam, ref_seqs, idx, out_sam, batch_reads=cfg.args.batch_reads, threads=threads, output=spec)
        bam.close()
        ref_seqs.close()
        if world > 1:
            n = gather(final_sam, cfg.args.out_prefix, n)
    else:
        read_data = bam_mod.get_read_data(bam, ref_seqs)
        print("> computing individual read realignments")
        batch = []
        writer = bam_mod.BamRecordWriter(out_sam, bai=spec.bai, compress=spec.compress) if as_bam else None
        py_kw = dict(bam_writer=writer, references=bam.references) if as_bam else {}
        for rd in read_data:
            batch.append(rd)
            if len(batch) >= cfg.args.batch_reads:
                n += bam_mod.realign_reads(ctx, batch, out_sam, **py_kw)
                batch = []
        n += bam_mod.realign_reads(ctx, batch, out_sam, **py_kw)
        if writer is not None:
            writer.close()
    ctx.close()
    print(f"    {n} reads, runtime: {perf_counter() - start:.2f}s")


if __name__ == "__main__":
    cfg.args = argparser().parse_args()
    try:
        main()
    except KeyboardInterrupt:
        print("\nERROR: Program terminated.")
        sys.exit(1)
