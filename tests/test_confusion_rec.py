"""The recount of the confusion matrices from BAM records, on the CPU: the counting rule of csrc/confusion_rec.hpp built by
g++ (tests/model/confusion_rec.cpp) against the G7-pinned character loop fed by a Python pileup writer that implements
the same rule (tests/model/cms_model.py), the n-polymer annotation from the oracle.  Exact integer equality throughout."""
import collections
import os

import pytest

from conftest import GOLDEN
from model import cms_model as m
from npore_amd import bam


def _check(path, references, refs, ranges, max_n, max_l, **kw):
    want, tallies = m.expected(path, refs, ranges, max_n, max_l, **kw)
    got = m.twin_count(path, [n for n, _ in references], refs, ranges, max_n, max_l, **kw)
    assert m.same(got, want), [(int(a.sum()), int(b.sum())) for a, b in zip(got[:4], want)]
    assert m.tallies_agree(got[4], tallies), (got[4], dict(tallies))
    assert int(want[0].sum()) == tallies["entries_counted"]
    return tallies


@pytest.mark.parametrize("chunk_width", [100000, 97])
def test_twin_on_golden_reads(chunk_width):
    """tests/golden/data/reads.bam on ref.fasta: its 10 reads hold 13 adjacent INDEL pairs, none of which is counted."""
    d = os.path.join(GOLDEN, "data")
    refs = bam.read_fasta(os.path.join(d, "ref.fasta"))
    f = bam.BamFile(os.path.join(d, "reads.bam"))
    references = list(zip(f.references, f.lengths))
    t = _check(os.path.join(d, "reads.bam"), references, refs, m.whole_contig_ranges(references, chunk_width), 6, 100)
    assert t["adjacent_indels"] == 13 and t["records"] == 10 and t["entries_counted"] > 4000
    # the realigner's filter, no quality bound: what the text route's fixture writer sees
    _check(os.path.join(d, "reads.bam"), references, refs, m.whole_contig_ranges(references, chunk_width), 6, 100, min_bq=0,
           exclude_flags=0x904)


@pytest.mark.parametrize("max_l,chunk_width", [(100, 100000), (100, 30), (5, 100000)])
def test_twin_on_engineered_contig(tmp_path, max_l, chunk_width):
    """the engineered contig of tests/golden/make_golden_cms.py, its lines turned into records (bam.write_bam)"""
    references, refs, records = m.engineered_records()
    path = str(tmp_path / "eng.bam")
    bam.write_bam(path, references, records)
    t = _check(path, references, refs, m.whole_contig_ranges(references, chunk_width), 6, max_l)
    for k in ("copy_deletion", "copy_insertion", "noncopy_indel_at_start", "indel_k_ge_max_l", "insertion_unit_clipped", "lowq_with_marker",
              "adjacent_indels", "entries_ambiguous", "records_flagged"):
        assert t[k] > 0, (k, dict(t))
    # overlapping ranges count their positions once each; a range that leaves the contig is clipped; ranges in any order
    n = references[0][1]
    _check(path, references, refs, [("eng", 40, n + 50), ("eng", 0, 60), ("eng", 10, 20), ("eng", n, n + 5)], 6, max_l)


def test_twin_on_random_bams(tmp_path):
    """Seeded random BAMs: clips, both strands, excluded and supplementary reads, qualities on both sides of the bound and
    missing, IUPAC letters, reads on a contig's first and last base, several contigs, chunk widths that cut polymers,
    max_l in {5, 100}.  The writer's tallies show that every branch of the counting loop was reached: a generator that
    misses one would hide it.  (`insertion_unit_clipped`: an insertion whose unit contig[a+1 : a+1+n] is cut by the contig's
    end for a period that divides it.  The loop compares only at a polymer start, which has three whole repeats inside the
    contig, so the clipped compare itself cannot run on a true annotation; the guard is exercised, the count is unchanged.)"""
    total = collections.Counter()
    for seed, max_l, chunk_width in m.RANDOM_CASES:
        path = str(tmp_path / f"r{seed}_{max_l}_{chunk_width}.bam")
        references, refs = m.make_random_bam(path, seed, max_l=max_l)
        t = _check(path, references, refs, m.whole_contig_ranges(references, chunk_width), 6, max_l)
        total.update(t)
        assert t["records_flagged"] > 0 and t["records_refskip"] == 1 and t["adjacent_indels"] > 0 and t["entries_lowq"] > 0
        assert t["entries_ambiguous"] > 0
        f = bam.BamFile(path)
        clen = dict(references)
        ends = [(r.reference_start, r.reference_start + sum(n for op, n in r.cigar if op in (0, 2, 3, 7, 8)) == clen[f.references[r.ref_id]])
                for r in f.records]
        assert any(p == 0 for p, _ in ends) and any(e for _, e in ends)
        assert any(r.flag & 0x800 and not r.flag & 0x704 for r in f.records) and any(r.flag & 16 for r in f.records)
        assert any(op == 4 for r in f.records for op, _ in r.cigar) and any(op == 5 for r in f.records for op, _ in r.cigar)
        assert any(r.qual[:1] == b"\xff" for r in f.records)
    for k in m.BRANCHES:
        assert total[k] > 0, (k, dict(total))
    per_case = {}
    for seed, max_l, chunk_width in m.RANDOM_CASES[:3]:
        path = str(tmp_path / f"r{seed}_{max_l}_{chunk_width}.bam")
        references, refs = m.make_random_bam(path, seed, max_l=max_l)
        _, per_case[(max_l, chunk_width)] = m.expected(path, refs, m.whole_contig_ranges(references, chunk_width), 6, max_l)
    for k in m.BRANCHES:                                   # ... and each within the three cases of one seed
        assert sum(t[k] for t in per_case.values()) > 0, k
