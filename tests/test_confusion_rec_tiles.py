"""The recount of the confusion matrices from BAM records on records whose CIGARs span several tiles of 256 operations --
the path every real ONT read takes through the kernel -- and on a hand-made annotation that reaches the clip of the
insertion compare.  Host twin (CPU) here; tests/test_gpu_confusion_rec_tiles.py runs the same inputs on the device."""
import numpy as np
import pytest

from model import cms_model as m
from npore_amd import bam


def check_long_facts(facts):
    """the generator made what it promises"""
    c0, c1, c2 = facts
    assert len(c0) > 512 and len(c1) > 512 and len(c2) > 768
    assert c0[255][0] in m.M_OPS and c0[256][0] == 1                       # a match on a tile's last slot, its marker in the next tile
    assert c0[510][0] in m.M_OPS and c0[511][0] == 2 and c0[512][0] == 1   # an adjacent pair across a border
    assert any(op in m.M_OPS and n > 256 for op, n in c0) and any(op in m.M_OPS and n > 256 for op, n in c2)
    assert c1[0][0] == 4 and c1[256][0] in m.M_OPS and c1[257][0] == 2     # with a leading clip: a D marker behind the first border's match
    assert c2[767][0] in m.M_OPS and c2[768][0] == 1


@pytest.mark.parametrize("max_l,chunk_width", [(100, 100000), (100, 257), (5, 1000)])
def test_twin_on_records_of_several_tiles(tmp_path, max_l, chunk_width):
    references, refs, records, facts = m.long_cigar_records()
    check_long_facts(facts)
    path = str(tmp_path / "long.bam")
    bam.write_bam(path, references, records)
    ranges = m.whole_contig_ranges(references, chunk_width)
    want, t = m.expected(path, refs, ranges, 6, max_l)
    got = m.twin_count(path, [n for n, _ in references], refs, ranges, 6, max_l)
    assert m.same(got, want) and m.tallies_agree(got[4], t), (got[4], dict(t))
    assert t["records"] == 3 and t["adjacent_indels"] >= 1 and t["entries_lowq"] > 0 and t["entries_counted"] > 3000
    assert t["copy_deletion"] + t["copy_insertion"] > 0


def test_twin_clipped_insertion_compare(tmp_path, monkeypatch):
    """An insertion whose copy test is clipped by the contig's end.  On a true annotation the compare runs only at a polymer
    start, which has three whole repeats inside the contig, so the clip cannot be reached; here the annotation is hand-made:
    a start of period 2 (and 1) on the contig's LAST base.  The clipped unit never compares equal, in the character loop
    (Python slice semantics) as in confusion_rec.hpp."""
    ctg = m.engineered_contig()
    n = len(ctg)

    def hook(seq, info):
        info = np.array(info)
        if seq.endswith(ctg[-4:]):                   # the slice reaches the contig's end: starts on its last base
            info[len(seq) - 1, 0, 0], info[len(seq) - 1, 1, 0] = 3, 0
            info[len(seq) - 1, 0, 1], info[len(seq) - 1, 1, 1] = 4, 0
        return info

    monkeypatch.setattr(m, "INFO_HOOK", hook)
    last = ctg[-1]
    records = [{"name": f"c{k}", "flag": 0, "ref_id": 0, "pos": n - 20, "cigar": [(0, 19), (1, len(ins)), (0, 1)],
                "seq": ctg[n - 20:n - 1] + ins + last, "qual": None} for k, ins in enumerate((last * 2, last, last * 4, "CG"))]
    path = str(tmp_path / "clip.bam")
    bam.write_bam(path, [("eng", n)], records)
    for ranges in ([("eng", 0, n)], [("eng", 0, n - 5), ("eng", n - 5, n)]):
        want, t = m.expected(path, {"eng": ctg}, ranges, 6, 100)
        got = m.twin_count(path, ["eng"], {"eng": ctg}, ranges, 6, 100)
        assert m.same(got, want) and m.tallies_agree(got[4], t)
        # the period-2 start was met with insertions of 2 and 4 bases (the clipped compare ran and failed: the diagonal),
        # the period-1 start with a true copy of one base and of two, four
        assert want[1][1, 4, 4] == 4 and want[1][0, 3, 4] == 1 and want[1][0, 3, 5] == 1 and want[1][0, 3, 7] == 1
