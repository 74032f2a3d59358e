"""The recount of the confusion matrices from BAM records on the GPU (npore_bam_confusion: csrc/confusion_kernels.hpp, the
planes from np_info_wave_kernel on the device) against the same expectation as tests/test_confusion_rec.py: a Python
pileup writer of the rule through the G7-pinned character loop.  Exact integer equality throughout."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from model import cms_model as m
from npore_amd import aln, bam, cfg, realign

pytestmark = pytest.mark.gpu


def _device(path, ranges, max_n, max_l, ref_path, handle=None, batch_reads=None, **kw):
    ctx = aln.Context(None, None, max_n=max_n, max_l=max_l, device=0)      # an annotation-only context will do
    try:
        if batch_reads:
            ctx.set("cms_batch_reads", batch_reads)
        return bam.confusion_from_bam(ctx, handle or path, ref_path, ranges, **kw)
    finally:
        ctx.close()


def _write_fasta(path, refs):
    with open(path, "w") as fh:
        for n, s in refs.items():
            fh.write(f">{n}\n")
            for k in range(0, len(s), 60):
                fh.write(s[k:k + 60] + "\n")
    return path


def _check(path, ref_path, references, refs, ranges, max_n, max_l, **kw):
    want, tallies = m.expected(path, refs, ranges, max_n, max_l, **kw)
    got = _device(path, ranges, max_n, max_l, ref_path, **kw)
    assert m.same(got, want), [(int(a.sum()), int(b.sum())) for a, b in zip(got[:4], want)]
    assert m.tallies_agree(got[4], tallies), (got[4], dict(tallies))
    return got


@pytest.mark.parametrize("chunk_width", [100000, 97])
def test_device_on_golden_reads(chunk_width):
    d = os.path.join(GOLDEN, "data")
    refs = bam.read_fasta(os.path.join(d, "ref.fasta"))
    f = bam.BamFile(os.path.join(d, "reads.bam"))
    references = list(zip(f.references, f.lengths))
    got = _check(os.path.join(d, "reads.bam"), os.path.join(d, "ref.fasta"), references, refs,
                 m.whole_contig_ranges(references, chunk_width), 6, 100)
    assert got[4]["adjacent_indels"] == 13 and got[4]["records"] == 10


@pytest.mark.parametrize("max_l,chunk_width", [(100, 100000), (100, 30), (5, 100000)])
def test_device_on_engineered_contig(tmp_path, max_l, chunk_width):
    references, refs, records = m.engineered_records()
    path, fa = str(tmp_path / "eng.bam"), _write_fasta(str(tmp_path / "eng.fasta"), refs)
    bam.write_bam(path, references, records)
    _check(path, fa, references, refs, m.whole_contig_ranges(references, chunk_width), 6, max_l)
    n = references[0][1]
    _check(path, fa, references, refs, [("eng", 40, n + 50), ("eng", 0, 60), ("eng", 10, 20), ("eng", n, n + 5)], 6, max_l)


@pytest.mark.parametrize("seed,max_l,chunk_width", m.RANDOM_CASES)
def test_device_on_random_bams(tmp_path, seed, max_l, chunk_width):
    path = str(tmp_path / "r.bam")
    references, refs = m.make_random_bam(path, seed, max_l=max_l)
    fa = _write_fasta(str(tmp_path / "r.fasta"), refs)
    _check(path, fa, references, refs, m.whole_contig_ranges(references, chunk_width), 6, max_l)
    _check(path, fa, references, refs, m.whole_contig_ranges(references, chunk_width), 4, max_l, min_bq=0, exclude_flags=0x904)


def test_device_readers_and_batching_agree(tmp_path):
    """the one-pass and the indexed reader, one batch and many small ones: the same counts, the same tallies"""
    path = str(tmp_path / "r.bam")
    references, refs = m.make_random_bam(path, 7, n_reads=90)
    fa = _write_fasta(str(tmp_path / "r.fasta"), refs)
    ranges = m.whole_contig_ranges(references, 53)
    want, _ = m.expected(path, refs, ranges, 6, 100)
    runs = {}
    for name, one_pass, batch in (("one-pass", True, None), ("indexed", False, None), ("one-pass, batches of 3", True, 3),
                                  ("indexed, batches of 1", False, 1)):
        h = bam.NativeBam(path, one_pass=one_pass, share=False)
        try:
            runs[name] = _device(path, ranges, 6, 100, fa, handle=h, batch_reads=batch)
        finally:
            h.close()
    for name, got in runs.items():
        assert m.same(got, want), name
        assert all(got[4][k] == runs["one-pass"][4][k] for k in m.TALLY_NAMES), name
    assert runs["one-pass"][4]["batches"] == 1 and runs["one-pass, batches of 3"][4]["batches"] > 10
    # a file that is not sorted by reference: the one-pass walk is refused, a path falls back to the index
    f = bam.BamFile(path)
    recs = [{"name": r.query_name, "flag": r.flag, "ref_id": r.ref_id, "pos": r.reference_start, "cigar": r.cigar, "seq": r.seq,
             "qual": None if r.qual[:1] == b"\xff" else r.qual} for r in f.records]
    unsorted = str(tmp_path / "u.bam")
    bam.write_bam(unsorted, references, recs[::-1])
    want_u, _ = m.expected(unsorted, refs, ranges, 6, 100)
    assert m.same(_device(unsorted, ranges, 6, 100, fa), want_u)


def test_device_equals_text_route_without_adjacent_indels(tmp_path):
    """min_bq = 0 and the realigner's flags on a BAM without adjacent INDELs: the counts of the text route fed by the
    repository's fixture writer (tests/golden/make_golden_cms.py pileup_lines), annotation from the device there too."""
    import argparse
    sys.path.insert(0, GOLDEN)
    from make_golden_cms import pileup_lines
    references, refs, records = m.engineered_records()
    keep = []
    for r in records:
        vis = [op for op, n in r["cigar"] if n > 0 and op not in (4, 5)]
        adjacent = any(op in (1, 2) and (k == 0 or vis[k - 1] in (1, 2)) for k, op in enumerate(vis))
        if not adjacent and set(r["seq"]) <= set("ACGTN"):
            keep.append(r)
    assert len(keep) > 30
    path, fa = str(tmp_path / "e.bam"), _write_fasta(str(tmp_path / "e.fasta"), refs)
    bam.write_bam(path, references, keep)
    sam = str(tmp_path / "e.sam")
    with open(sam, "w") as fh:
        for r in keep:
            cg = "".join(f"{n}{'MIDNSHP=X'[op]}" for op, n in r["cigar"])
            fh.write(f"{r['name']}\t{r['flag']}\teng\t{r['pos'] + 1}\t60\t{cg}\t*\t0\t0\t{r['seq']}\t*\n")
    ctg = refs["eng"]
    lines = pileup_lines(sam, len(ctg))
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100)
    try:
        for chunk_width in (100000, 41):
            ranges = m.whole_contig_ranges(references, chunk_width)
            want = None
            for c, st, en in ranges:
                res = bam.calc_confusion_matrices((c, st, en), pileups=lines[st:en], refs=refs)
                want = res if want is None else tuple(a + b for a, b in zip(want, res))
            got = _device(path, ranges, 6, 100, fa, min_bq=0, exclude_flags=0x904)
            assert m.same(got, want) and got[4]["adjacent_indels"] == 0 and int(want[0].sum()) > 1000
    finally:
        cfg.args = old


def test_realign_cli_recalc_cms_from_bam(tmp_path, monkeypatch):
    """`realign --recalc_cms --recalc_exit --cms_source bam`: the four matrices land in --stats_dir, equal to the API's on
    the same ranges, without samtools and with nothing written into the package's data directory."""
    from npore_amd.bed import get_ranges
    shipped = os.path.join(os.path.dirname(os.path.abspath(bam.__file__)), "data", "guppy5_stats")
    digest = lambda: [hashlib.sha256(open(os.path.join(shipped, f), "rb").read()).hexdigest() for f in sorted(os.listdir(shipped))]
    before = digest()
    monkeypatch.setenv("PATH", str(tmp_path))            # (no samtools anywhere)
    monkeypatch.chdir(tmp_path)
    d = os.path.join(GOLDEN, "data")
    old = cfg.args
    try:
        for extra, min_bq in ((["--chunk_width", "97"], 13), (["--chunk_width", "20000", "--cms_min_bq", "0", "--cms_exclude_flags", "2308"], 0)):
            out = tmp_path / f"st{min_bq}"
            cfg.args = realign.argparser().parse_args(
                ["--bam", os.path.join(d, "reads.bam"), "--ref", os.path.join(d, "ref.fasta"), "--out_prefix", str(tmp_path / "o"),
                 "--recalc_cms", "--recalc_exit", "--cms_source", "bam", "--stats_dir", str(out)] + extra)
            with pytest.raises(SystemExit) as ex:
                realign.main()
            assert ex.value.code == 0
            got = [np.load(os.path.join(out, f"{k}_cm.npy")) for k in ("subs", "nps", "inss", "dels")]
            ranges = get_ranges(cfg.args.regions, cfg.args.chunk_width)
            want = _device(os.path.join(d, "reads.bam"), ranges, 6, 100, os.path.join(d, "ref.fasta"), min_bq=min_bq,
                           exclude_flags=cfg.args.cms_exclude_flags)
            assert m.same(got, want) and got[0].sum() > 4000
            assert got[1].shape == (6, 101, 101) and all(g.dtype == np.int64 for g in got)
            assert not [f for f in os.listdir(out) if f.endswith(".tmp.npy")]
    finally:
        cfg.args = old
    assert digest() == before
    assert realign.argparser().parse_args(["--bam", "x", "--ref", "y", "--out_prefix", "z"]).cms_source == "mpileup"
