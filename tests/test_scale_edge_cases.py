"""The inputs of tests/scale_edge_cases.py on the CPU: that each of them crosses the threshold it is built for, and that the
two statements of every expectation the GPU tests use -- the Python writers of tests/model and the g++ twins of the
kernels' host rules -- agree on them.  No GPU."""
import hashlib

import numpy as np
import pytest

import oracle
import scale_edge_cases as sc
from model import cms_model as m
from model import purity_model as pm
from npore_amd import bam
from test_bed import literal_np_regions


# ---- 1. purity: windows of more than 256 and 512 scan blocks ---------------------------------------------------------------
@pytest.fixture(scope="module")
def big(tmp_path_factory):
    references, records = sc.big_purity_case()
    path = str(tmp_path_factory.mktemp("big") / "big.bam")
    bam.write_bam(path, references, records)
    return path, references, records


def test_big_purity_anchors_lie_on_both_sides_of_every_scan_border(big):
    path, references, records = big
    n_blocks = -(-sc.BIG_LEN // sc.PUR_SCAN_PER_BLOCK)
    assert n_blocks == 518 and -(-n_blocks // sc.PUR_TOP_ROUND) == 3 and sc.BIG_LEN % sc.PUR_SCAN_PER_BLOCK != 0
    assert sc.PUR_CARRY_FROM == 262_144 and sc.PURITY_WINDOW_DEFAULT // sc.PUR_SCAN_PER_BLOCK == 4096
    assert tuple(a // sc.PUR_SCAN_PER_BLOCK for a in sc.ANCHORS) == sc.ANCHOR_BLOCKS
    assert sc.ANCHOR_BLOCKS[-1] == n_blocks - 1
    for b in (sc.PUR_CARRY_FROM, 2 * sc.PUR_CARRY_FROM):                 # the last position of a round and the first of the next
        assert b - 1 in sc.ANCHORS and b in sc.ANCHORS
    assert len(records) == 5 * len(sc.ANCHORS) == 60
    ends = sorted((r["pos"] + r["cigar"][0][1] - 1, r["cigar"][1]) for r in records)
    assert [e for e, _ in ends] == sorted(list(sc.ANCHORS) * 5)
    assert all(len(r["cigar"]) == 3 and r["cigar"][1][0] == 1 and r["cigar"][2][0] == 0 for r in records)
    assert sorted(len(s) for s in sc.INSERTS) == [1, 1, 1, 2, 17]


def test_big_purity_model_equals_twin(big):
    path, references, records = big
    for ranges in sc.big_ranges():
        rows, hb, hi, scores, tallies = pm.expected(path, ranges)
        t_rows, t_hb, t_hi, t_tallies = pm.twin(path, [sc.BIG_NAME], ranges, len(rows))
        assert np.array_equal(t_rows, rows), np.nonzero((t_rows != rows).any(axis=1))[0][:10]
        assert np.array_equal(t_hb, hb) and np.array_equal(t_hi, hi)
        assert pm.tallies_agree(t_tallies, tallies), (t_tallies, dict(tallies))
        whole = len(ranges) == 1
        assert len(rows) == (sc.BIG_LEN if whole else sc.BIG_LEN - sc.GAP_CUT)
        inside = [a for a in sc.ANCHORS if whole or not 1000 <= a < 1000 + sc.GAP_CUT]
        assert len(inside) == (12 if whole else 10)
        assert tallies["insertions_counted"] == 5 * len(inside) and tallies["insertions_hashed"] == len(inside)
        for a in inside:
            at = a if whole or a < 1000 else a - sc.GAP_CUT
            n, sb, t, si = rows[at]
            assert t == 5 and n >= 5 and si == (n - 5) ** 2 + 11, (a, rows[at])
        if not whole:                                                    # the dense blocks are other blocks, on both sides of the first carry
            blocks = [(a if a < 1000 else a - sc.GAP_CUT) // sc.PUR_SCAN_PER_BLOCK for a in inside]
            assert blocks == [0, 254, 254, 254, 255, 255, 510, 510, 510, 515]


# ---- 2. region scan: more than one count per thread ------------------------------------------------------------------------
def test_region_slices_reach_every_per():
    assert [sc.scan_per(k, 6) for k in sc.REGION_SLICE_COUNTS] == [1, 2, 7]
    assert [sc.scan_per(k, mn) for k, mn, _ in sc.REGION_CONTEXTS] == [1, 2, 7, 5, 2]
    assert 6 * 170 <= sc.REGION_SCAN_THREADS < 6 * 171
    for k in sc.REGION_SLICE_COUNTS:
        slices, kinds = sc.region_slices(k)
        assert len(slices) == len(kinds) == k
        lens = [len(s) for s in slices]
        assert set(sc.STRIDE_LENGTHS) <= {n for n, kd in zip(lens, kinds) if kd == "rich"} and max(lens) == 1025
        assert all(len(s) == 0 for s, kd in zip(slices, kinds) if kd == "empty")
        assert kinds[:10] == ["empty"] * 10 and kinds[-14:-4] == ["empty"] * 10 and kinds[-4:] == ["plain"] * 3 + ["rich"]
        assert sum(lens) <= 330_000
        assert all(s.dtype == np.uint8 and (len(s) == 0 or (1 <= s.min() and s.max() <= 4)) for s in slices)


def test_region_slices_of_the_largest_case_under_the_literal_loop():
    k = 1100
    slices, kinds = sc.region_slices(k)
    assert 250_000 <= sum(map(len, slices)) <= 330_000
    counts = np.zeros((6, k), np.int64)
    for j, s in enumerate(slices):
        if len(s):
            want = literal_np_regions(np.asarray(oracle.get_np_info(s, max_n=6, max_l=100)), 0, 6)
            counts[:, j] = [len(w) for w in want]
    assert counts.sum() > 5000 and counts[:, -1].sum() > 0 and (counts.sum(axis=1) > 0).all()
    plain = counts[:, [j for j, kd in enumerate(kinds) if kd == "plain"]].sum(axis=0)
    rich = counts[:, [j for j, kd in enumerate(kinds) if kd == "rich" and len(slices[j]) >= 40]].sum(axis=0)
    assert plain.mean() < rich.mean() / 3
    # what the threads of region_scan_kernel see: whole threads of zeros behind threads that have counted, borders inside a
    # run of zeros, and empty threads at the end
    per = sc.scan_per(k, 6)
    flat = counts.reshape(-1)
    used = -(-len(flat) // per)
    assert used < sc.REGION_SCAN_THREADS and used * per > len(flat)          # the last thread that has counts has fewer than per
    sums = [int(flat[t * per:(t + 1) * per].sum()) for t in range(used)]
    zero_threads = [t for t in range(1, used) if sums[t] == 0 and sum(sums[:t]) > 0]
    assert len(zero_threads) >= 6 and sums[used - 1] > 0


# ---- 3. byte planes across segment borders ---------------------------------------------------------------------------------
def test_segment_generator_draws_are_unchanged():
    """the draws of tests/test_gpu_parity.py::test_get_np_info_segments_of_long_sequences, as they were when the generator
    stood inside that test"""
    rng = np.random.default_rng(12)
    h = hashlib.sha256()
    for _ in range(4):
        for kind in (0, 1):
            s = sc.segment_sequence(rng, kind, 70_000)
            assert s.dtype == np.uint8 and len(s) == 70_000
            h.update(s.tobytes())
    assert h.hexdigest() == "01520d6a81abfbc64d178b9b2ee1851b4cd1171372021b10c8fec8935dadbe09"


def test_border_slices_hold_what_they_plant():
    B = sc.NP_INFO_SEG
    slices = sc.border_slices()
    lens = [len(s) for s in slices]
    assert sorted(lens)[3:] == [B - 1, B, B + 1, 40_000, 70_000] and sorted(lens)[2] < B // 4
    off = np.concatenate([[0], np.cumsum(lens)])
    assert all(off[j] % 64 != 0 for j, n in enumerate(lens) if n >= B - 1)          # no long slice starts on a window of the buffer
    assert sum(lens) < 170_000
    assert [sc.np_info_warm(mn, ml) for mn, ml in sc.SEGMENT_CONTEXTS] == [2176, 2752, 256, 64]
    big, mid = slices[lens.index(70_000)], slices[lens.index(40_000)]
    # the homopolymer is longer than every warm-up, and the wave of the second segment starts inside it at the default shape
    assert (big[B - 2500:B + 500] == 3).all() and 3000 > max(sc.np_info_warm(mn, ml) for mn, ml in sc.SEGMENT_CONTEXTS)
    assert B - 2500 < B - sc.np_info_warm(6, 100)
    for s in (big, mid):
        assert (s[2 * B - 40:2 * B + 60] == 0).all()
    for s, b in ((big, 3 * B), (mid, B)):
        for max_n, max_l in ((6, 100), (6, 127)):
            info = np.asarray(oracle.get_np_info(s, max_n=max_n, max_l=max_l))
            assert info[b, 0, 5] == 30 and info[b, 1, 5] == 0                     # a start bit exactly on the border
            assert not ((info[b - 6:b, 0, 5] != 0) & (info[b - 6:b, 1, 5] == 0)).any()
    # the short array across 4 B: position 4 B is no start, but it would be one for a wave that began there without warm-up
    for max_n, max_l in sc.SEGMENT_CONTEXTS:
        _no_start_but_for_the_warm_up(big, 4 * B, max_n, max_l)
    # every segment border that is not inside an N stretch lies in a polymer
    for s in slices:
        info = np.asarray(oracle.get_np_info(s, max_n=6, max_l=100))
        for b in range(B, len(s), B):
            assert s[b] == 0 or (info[b - 3:b + 3, 0] != 0).any(), (len(s), b)


def _no_start_but_for_the_warm_up(s, b, max_n, max_l):
    info = np.asarray(oracle.get_np_info(s, max_n=max_n, max_l=max_l))
    assert info[b, 0, 1] != 0 and info[b, 1, 1] != 0, info[b]
    suffix = np.asarray(oracle.get_np_info(s[b:], max_n=max_n, max_l=max_l))
    assert suffix[0, 0, 1] == 4 and suffix[0, 1, 1] == 0, suffix[0]


@pytest.fixture(scope="module")
def border(tmp_path_factory):
    references, refs, records, forced = sc.border_case()
    path = str(tmp_path_factory.mktemp("border") / "border.bam")
    bam.write_bam(path, references, records)
    return path, references, refs, records, forced


def test_border_reads_carry_indels_at_the_starts_next_to_the_borders(border):
    path, references, refs, records, forced = border
    assert references == [(sc.BORDER_NAME, sc.BORDER_LEN)] and all(b < sc.BORDER_LEN for b in sc.BORDERS)
    assert len(records) == 80
    near = [r for r in records if any(abs(r["pos"] - b) <= 150 for b in sc.BORDERS)]
    assert len(near) >= 40
    assert len(forced) == 4 and sc.NP_INFO_SEG in forced and all(min(abs(p - b) for b in sc.BORDERS) < 140 for p in forced)
    at = {p: 0 for p in forced}
    for r in records:
        ref = r["pos"]
        for k, (op, n) in enumerate(r["cigar"]):
            if op in (1, 2) and ref in at and k > 0 and r["cigar"][k - 1][0] in m.M_OPS:
                at[ref] += 1
            ref += n if op in (0, 2, 7, 8) else 0
    assert all(v >= 5 for v in at.values()), at
    # the short array across the second border, and reads whose entry in front of it is counted with its annotation
    from npore_amd.cig import bases_to_int
    for max_n in (6, 4):
        _no_start_but_for_the_warm_up(np.asarray(bases_to_int(refs[sc.BORDER_NAME]), np.uint8), sc.BORDERS[1], max_n, 100)
    b = sc.BORDERS[1]
    across = 0
    for r in records:
        ref = r["pos"]
        for op, n in r["cigar"]:
            across += op in m.M_OPS and ref <= b - 1 < ref + n and not r["flag"] & 0x704
            ref += n if op in (0, 2, 7, 8) else 0
    assert across >= 5, across


@pytest.mark.parametrize("max_n", [6, 4])
def test_border_recount_model_equals_twin(border, max_n):
    path, references, refs, records, forced = border
    sets = sc.border_range_sets(references)
    assert [len(s) for s in sets] == [1, 2, 3] and sets[2][0] == (sc.BORDER_NAME, 0, sc.NP_INFO_SEG)
    totals = []
    for ranges in sets:
        want, tallies = m.expected(path, refs, ranges, max_n, 100)
        got = m.twin_count(path, [sc.BORDER_NAME], refs, ranges, max_n, 100)
        assert m.same(got, want), [(int(a.sum()), int(b.sum())) for a, b in zip(got[:4], want)]
        assert m.tallies_agree(got[4], tallies), (got[4], dict(tallies))
        assert tallies["copy_deletion"] > 10 and tallies["copy_insertion"] > 10 and tallies["records_flagged"] > 0 and tallies["entries_lowq"] > 0
        totals.append(int(want[0].sum()))
    assert totals[0] == totals[1] == totals[2] > 5000
    # counted copy-number changes at polymer starts behind the first border
    (subs, nps, inss, dels), _ = m.expected(path, refs, [(sc.BORDER_NAME, sc.NP_INFO_SEG, sc.BORDER_LEN)], max_n, 100)
    off_diagonal = int(nps.sum() - sum(np.trace(nps[n]) for n in range(max_n)))
    assert off_diagonal >= 10, off_diagonal
