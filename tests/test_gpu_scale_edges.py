"""The purity, region and plane kernels on inputs larger than their size thresholds (tests/scale_edge_cases.py states each
threshold next to the constant it comes from; tests/test_scale_edge_cases.py shows on the CPU that the inputs cross them):

  * purity_scan_top_kernel's carry between its rounds of 256 blocks: windows of 518, 256 and 293 blocks;
  * region_scan_kernel with 1, 2, 5 and 7 counts per thread and empty tail threads;
  * np_info_wave_kernel<ANNOT_PLANES>: slices of more than one segment of 16 384 positions, read by the region kernels and
    by the recount from BAM records.

The expectations are those of tests/test_gpu_purity.py, tests/test_bed.py and tests/test_gpu_confusion_rec.py: the Python
pileup writers of tests/model and the literal loop over the oracle's get_np_info.  Integers are compared exactly."""
import functools

import numpy as np
import pytest

import oracle
import scale_edge_cases as sc
from model import cms_model as m
from model import purity_model as pm
from npore_amd import aln, bam
from test_bed import literal_np_regions
from test_gpu_confusion_rec import _device as recount_device, _write_fasta
from test_gpu_purity import _device as purity_device, _same as purity_same

pytestmark = pytest.mark.gpu


# ---- 1. purity beyond 256 and 512 scan blocks ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """the BAM of big_purity_case() and, per range set of big_ranges(), the model's expectation: computed once"""
    references, records = sc.big_purity_case()
    path = str(tmp_path_factory.mktemp("big") / "big.bam")
    bam.write_bam(path, references, records)
    whole, gap = sc.big_ranges()
    return path, whole, pm.expected(path, whole), gap, pm.expected(path, gap)


def test_purity_one_window_of_518_blocks(big):
    """the default window holds the whole contig: three rounds of purity_scan_top_kernel, the last block partial"""
    path, whole, want, _, _ = big
    got = purity_device(path, whole)
    purity_same(got, want)
    assert got[2]["windows"] == 1 and got[2]["insertions_counted"] == 60 and got[2]["insertions_hashed"] == 12


def test_purity_dense_positions_across_the_carry(big):
    """ranges with a gap of 2 000 positions: the dense index is not the contig position where the second round begins"""
    path, _, _, gap, want = big
    got = purity_device(path, gap)
    purity_same(got, want)
    assert got[2]["windows"] == 1 and got[3].shape[0] == sc.BIG_LEN - sc.GAP_CUT


def test_purity_windows_of_exactly_256_blocks(big):
    """purity_window = 262 144: one full round per window and no more; the third window has 6 blocks"""
    path, whole, want, _, _ = big
    got = purity_device(path, whole, window=sc.PUR_CARRY_FROM)
    purity_same(got, want)
    assert got[2]["windows"] == 3


def test_purity_window_of_293_blocks_then_225(big):
    """purity_window = 300 000: the second window is shorter than the first, whose block sums are still in the buffer"""
    path, whole, want, _, _ = big
    got = purity_device(path, whole, window=300_000)
    purity_same(got, want)
    assert got[2]["windows"] == 2


def test_purity_event_buffer_grows_in_the_long_window(big):
    """cms_batch_reads = 7: nine batches into one window of 518 blocks, the event buffer grown in between"""
    path, whole, want, _, _ = big
    got = purity_device(path, whole, batch_reads=7)
    purity_same(got, want)
    assert got[2]["windows"] == 1 and got[2]["batches"] >= 9


# ---- 2. region scan with more than one count per thread --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _region_slices(n_slices):
    return sc.region_slices(n_slices)[0]


def _check_regions(slices, max_n, max_l):
    ctx = aln.Context(None, None, max_n=max_n, max_l=max_l, device=0)      # an annotation-only context
    try:
        got = ctx.np_regions(slices)
    finally:
        ctx.close()
    assert len(got) == max_n and all(len(g) == len(slices) for g in got)
    total = 0
    for k, seq in enumerate(slices):
        want = literal_np_regions(np.asarray(oracle.get_np_info(seq, max_n=max_n, max_l=max_l)), 0, max_n) if len(seq) else [[]] * max_n
        for n in range(max_n):
            pos, reps = got[n][k]
            assert [(int(p), int(p) + (n + 1) * int(r)) for p, r in zip(pos, reps)] == want[n], (k, n, len(seq))
            total += len(pos)
    return total


@pytest.mark.parametrize("n_slices,max_n,max_l", sc.REGION_CONTEXTS)
def test_np_regions_with_many_slices(n_slices, max_n, max_l):
    """170, 171 and 1 100 slices: 1, 2 and 7 counts per thread of region_scan_kernel at max_n = 6 (5 and 2 at max_n = 4 and 1),
    runs of empty slices over whole threads, the total behind the last count"""
    total = _check_regions(_region_slices(n_slices), max_n, max_l)
    assert total > (400 if n_slices < 1100 else 2000 if max_n == 1 else 4000)


# ---- 3. byte planes across segment borders ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _border_slices():
    return sc.border_slices()


@pytest.mark.parametrize("max_n,max_l", sc.SEGMENT_CONTEXTS)
def test_np_regions_of_slices_longer_than_a_segment(max_n, max_l):
    """slices of 16 383, 16 384, 16 385, 40 000 and 70 000 positions in one call: every start bit of the byte planes, those
    on and next to the segment borders among them"""
    assert _check_regions(_border_slices(), max_n, max_l) > 1000


@pytest.fixture(scope="module")
def border(tmp_path_factory):
    references, refs, records, _ = sc.border_case()
    d = tmp_path_factory.mktemp("border")
    path, fa = str(d / "border.bam"), _write_fasta(str(d / "border.fasta"), refs)
    bam.write_bam(path, references, records)
    return path, fa, references, refs


@pytest.mark.parametrize("max_n", [6, 4])
def test_recount_on_a_contig_of_three_segments(border, max_n):
    """confusion_records_kernel reads the planes of a contig of 40 000 positions: as one range (three segments, two warm-ups),
    in chunks of 20 000 (each range crosses a border) and of 16 384 (the ranges end where the segments do)"""
    path, fa, references, refs = border
    for ranges in sc.border_range_sets(references):
        want, tallies = m.expected(path, refs, ranges, max_n, 100)
        got = recount_device(path, ranges, max_n, 100, fa)
        assert m.same(got, want), [(int(a.sum()), int(b.sum())) for a, b in zip(got[:4], want)]
        assert m.tallies_agree(got[4], tallies), (got[4], dict(tallies))
        assert tallies["copy_deletion"] > 10 and tallies["copy_insertion"] > 10
