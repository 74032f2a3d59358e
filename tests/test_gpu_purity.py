"""Gini purity of pileups from BAM records on the GPU (npore_bam_purity: csrc/purity_kernels.hpp) against the same
expectation as tests/test_purity.py: a Python pileup writer of the rule through the model of the reference's function
and its float binning.  Integers -- the per-position rows, both histograms, the tallies -- are compared exactly."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from model import cms_model
from model import purity_model as pm
from npore_amd import aln, bam, purity

pytestmark = pytest.mark.gpu


def _device(path, ranges, handle=None, batch_reads=None, window=None, **kw):
    ctx = aln.Context(None, None, max_n=6, max_l=100, device=0)      # an annotation-only context will do
    try:
        if batch_reads:
            ctx.set("cms_batch_reads", batch_reads)
        if window:
            ctx.set("purity_window", window)
        return purity.purity_from_bam(ctx, handle or path, ranges, per_position=True, **kw)
    finally:
        ctx.close()


def _same(got, want):
    rows, hb, hi, scores, tallies = want
    assert np.array_equal(got[3], rows), np.nonzero((got[3] != rows).any(axis=1))[0][:10]
    assert np.array_equal(got[0], hb) and np.array_equal(got[1], hi)
    assert pm.tallies_agree(got[2], tallies), (got[2], dict(tallies))
    # about ten roundings of values <= 1 at 2^-52 each, with a factor of four over
    assert got[4].shape == scores.shape and (len(scores) == 0 or np.abs(got[4] - scores).max() <= 1e-14)


def _check(path, ranges, min_bq=13, exclude_flags=0x704, **kw):
    want = pm.expected(path, ranges, min_bq, exclude_flags)
    got = _device(path, ranges, min_bq=min_bq, exclude_flags=exclude_flags, **kw)
    _same(got, want)
    return got


def test_device_on_golden_reads():
    path = os.path.join(GOLDEN, "data", "reads.bam")
    f = bam.BamFile(path)
    got = _check(path, [(n, 0, l) for n, l in zip(f.references, f.lengths)])
    assert got[2]["records"] == 10 and got[2]["star_entries"] > 0 and got[2]["insertions_counted"] > 0 and got[2]["windows"] >= 1
    mid = f.lengths[0] // 2
    region = purity.parse_region(f"{f.references[0]}:{mid - 200}-{mid + 300}", f.references, f.lengths)
    assert region == [(f.references[0], mid - 201, mid + 300)]
    _check(path, region)


def test_device_on_engineered_records(tmp_path):
    references, refs, records = cms_model.engineered_records()
    path = str(tmp_path / "eng.bam")
    bam.write_bam(path, references, records)
    for ranges in pm.range_sets(references):
        _check(path, ranges)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_device_on_random_bams(tmp_path, seed):
    path = str(tmp_path / "r.bam")
    references, _ = cms_model.make_random_bam(path, seed)
    sets = pm.range_sets(references)
    _check(path, sets[0])
    _check(path, sets[0], min_bq=0, exclude_flags=0x904)
    _check(path, sets[2])
    _check(path, sets[3], min_bq=0, exclude_flags=0x904)


def test_device_on_long_cigars(tmp_path):
    """more than 256 and more than 512 operations: the tile carry"""
    references, refs, records, facts = cms_model.long_cigar_records()
    assert max(map(len, facts)) > 512 and min(map(len, facts)) > 256
    path = str(tmp_path / "long.bam")
    bam.write_bam(path, references, records)
    got = _check(path, [("long", 0, references[0][1])])
    assert got[2]["insertions_without_entry"] >= 1
    _check(path, [("long", 0, references[0][1])], window=64)
    _check(path, [("long", 100, 700), ("long", 2000, 2100)], window=64)


def test_device_windows_of_64_equal_the_default(tmp_path):
    """purity_window = 64: a record spanning three windows, an insertion on a window's last position, a deletion across a
    window border, a deletion that covers a whole window -- through both readers"""
    references, records = pm.window_records()
    spans = [(r["pos"], r["pos"] + sum(n for op, n in r["cigar"] if op in (0, 2))) for r in records]
    assert any(e // 64 - s // 64 >= 2 for s, e in spans)
    assert any(len(r["cigar"]) > 1 and r["pos"] + r["cigar"][0][1] - 1 == 63 and r["cigar"][1][0] == 1 for r in records)
    assert any(len(r["cigar"]) > 1 and r["cigar"][1] == (2, 5) and r["pos"] + r["cigar"][0][1] == 126 for r in records)
    path = str(tmp_path / "w.bam")
    bam.write_bam(path, references, records)
    ranges = [("win", 0, 400)]
    want = pm.expected(path, ranges)
    base = _device(path, ranges)
    _same(base, want)
    assert base[2]["windows"] == 1
    for one_pass in (True, False):
        for batch in (None, 2):
            h = bam.NativeBam(path, one_pass=one_pass, share=False)
            try:
                got = _device(path, ranges, handle=h, window=64, batch_reads=batch)
            finally:
                h.close()
            _same(got, want)
            assert got[2]["windows"] == 7, got[2]
    # ranges with a gap: the windows are cut in the DENSE positions
    ranges = [("win", 30, 70), ("win", 100, 140), ("win", 60, 66), ("win", 180, 400)]
    want = pm.expected(path, ranges)
    for window in (None, 64):
        _same(_device(path, ranges, window=window), want)


def test_device_readers_and_batching_agree(tmp_path):
    """the one-pass and the indexed reader, one batch and many small ones, an unsorted file: the same integers"""
    path = str(tmp_path / "r.bam")
    references, _ = cms_model.make_random_bam(path, 7, n_reads=90)
    ranges = pm.range_sets(references)[2]
    want = pm.expected(path, ranges)
    runs = {}
    for name, one_pass, batch, window in (("one-pass", True, None, None), ("indexed", False, None, None), ("one-pass, batches of 3", True, 3, None),
                                          ("indexed, batches of 1", False, 1, None), ("one-pass, windows of 64", True, 3, 64),
                                          ("indexed, windows of 100", False, None, 100)):
        h = bam.NativeBam(path, one_pass=one_pass, share=False)
        try:
            runs[name] = _device(path, ranges, handle=h, batch_reads=batch, window=window)
        finally:
            h.close()
    for name, got in runs.items():
        _same(got, want)
    assert runs["one-pass"][2]["batches"] <= 3 and runs["one-pass, batches of 3"][2]["batches"] > 10      # (one per contig)
    # a file that is not coordinate-sorted: the one-pass walk is refused, a path falls back to the index
    f = bam.BamFile(path)
    recs = [{"name": r.query_name, "flag": r.flag, "ref_id": r.ref_id, "pos": r.reference_start, "cigar": r.cigar, "seq": r.seq,
             "qual": None if r.qual[:1] == b"\xff" else r.qual} for r in f.records]
    unsorted = str(tmp_path / "u.bam")
    bam.write_bam(unsorted, references, recs[::-1])
    h = bam.NativeBam(unsorted, one_pass=True, share=False)
    try:
        with pytest.raises(bam.OnePassUnsupported):
            _device(unsorted, ranges, handle=h)
    finally:
        h.close()
    _same(_device(unsorted, ranges), pm.expected(unsorted, ranges))
    _same(_device(unsorted, ranges, window=64), pm.expected(unsorted, ranges))
    # sorted by reference, but not by position within it
    by_ref = sorted(recs, key=lambda r: (r["ref_id"], -r["pos"]))
    half = str(tmp_path / "h.bam")
    bam.write_bam(half, references, by_ref)
    _same(_device(half, ranges), pm.expected(half, ranges))


@pytest.mark.parametrize("n_reads", [70, 300])
def test_device_many_insertions_at_one_position(tmp_path, n_reads):
    """three distinct strings, two of length 20 that differ in their last letter: buckets larger than a wave"""
    references, records = pm.deep_insertion_records(n_reads)
    path = str(tmp_path / "d.bam")
    bam.write_bam(path, references, records)
    got = _check(path, [("deep", 0, 120)])
    n, sb, t, si = got[3][49]
    assert t == n_reads > 64 and n == n_reads + n_reads // 5 and got[2]["insertions_hashed"] == 2 * n_reads // 5
    assert si == (n - t) ** 2 + 5 * (n_reads // 5) ** 2
    _check(path, [("deep", 0, 120)], batch_reads=7, window=64)


def test_purity_command_line(tmp_path):
    references, _ = cms_model.make_random_bam(str(tmp_path / "a.bam"), 4)
    cms_model.make_random_bam(str(tmp_path / "b.bam"), 5)
    paths = [str(tmp_path / "a.bam"), str(tmp_path / "b.bam")]
    region = f"{references[0][0]}:21-{references[0][1] - 20}"
    assert purity.main(["--bams"] + paths + ["--region", region, "--out", str(tmp_path / "p")]) == 0
    rep = json.load(open(tmp_path / "p_hist.json"))
    hists = []
    for idx, path in enumerate(paths):
        rows, hb, hi, scores, tallies = pm.expected(path, [(references[0][0], 20, references[0][1] - 20)])
        got = np.load(tmp_path / f"p{idx}.npy")
        assert got.dtype == np.float64 and got.shape == scores.shape and len(scores) > 100 and np.abs(got - scores).max() <= 1e-14
        assert rep["bams"][idx]["base_hist"] == hb.tolist() and rep["bams"][idx]["ins_hist"] == hi.tolist()
        assert pm.tallies_agree(rep["bams"][idx]["tallies"], tallies)
        hists.append((hb, hi))
    assert rep["pairs"] == json.loads(json.dumps(purity.pair_summary(hists)))
    assert rep["pairs"][0]["base_counts"] == (hists[0][0] + hists[1][0]).tolist()
    # more positions than --max_score_positions: the scores are skipped, the histograms are not
    assert purity.main(["--bams", paths[0], "--out", str(tmp_path / "q"), "--max_score_positions", "10"]) == 0
    assert not os.path.exists(tmp_path / "q0.npy") and os.path.exists(tmp_path / "q_hist.json")
