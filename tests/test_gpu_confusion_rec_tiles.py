"""npore_bam_confusion on records whose CIGARs span several tiles of 256 operations (tests/test_confusion_rec_tiles.py has the
same inputs on the host twin): the carry of the reference / query cursors across tiles, markers and adjacent pairs that
straddle a tile border, a match longer than a tile.  Exact integer equality with the pileup writer's expectation."""
import pytest

from model import cms_model as m
from npore_amd import bam
from test_confusion_rec_tiles import check_long_facts
from test_gpu_confusion_rec import _device, _write_fasta

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("max_l,chunk_width", [(100, 100000), (100, 257), (5, 1000)])
def test_device_on_records_of_several_tiles(tmp_path, max_l, chunk_width):
    references, refs, records, facts = m.long_cigar_records()
    check_long_facts(facts)
    path, fa = str(tmp_path / "long.bam"), _write_fasta(str(tmp_path / "long.fasta"), refs)
    bam.write_bam(path, references, records)
    ranges = m.whole_contig_ranges(references, chunk_width)
    want, t = m.expected(path, refs, ranges, 6, max_l)
    for batch in (None, 1):
        got = _device(path, ranges, 6, max_l, fa, batch_reads=batch)
        assert m.same(got, want) and m.tallies_agree(got[4], t), (got[4], dict(t))
    assert t["records"] == 3 and t["adjacent_indels"] >= 1 and t["entries_counted"] > 3000


def test_device_on_a_second_draw_of_long_records(tmp_path):
    references, refs, records, _ = m.long_cigar_records(seed=12)
    path, fa = str(tmp_path / "long.bam"), _write_fasta(str(tmp_path / "long.fasta"), refs)
    bam.write_bam(path, references, records)
    ranges = m.whole_contig_ranges(references, 1500)
    want, t = m.expected(path, refs, ranges, 6, 100, min_bq=0)
    got = _device(path, ranges, 6, 100, fa, min_bq=0)
    assert m.same(got, want) and m.tallies_agree(got[4], t)
