"""Gini purity of pileups from BAM records on the CPU: the Python model of the reference's function against the
reference's own floats (tests/golden/purity.json); the g++ twin of csrc/purity_rec.hpp against an independent statement of
the rule (records -> mpileup-syntax columns -> model); the integer bin rule against the float expression; the key of the
inserted strings; region parsing.  Integers are compared exactly everywhere."""
import itertools
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from model import cms_model
from model import purity_model as pm
from npore_amd import bam, purity


def test_model_equals_the_reference_floats():
    fx = json.load(open(os.path.join(GOLDEN, "purity.json")))["columns"]
    assert len(fx) >= 190
    seen = set()
    for e in fx:
        got = pm.compute_purity(e["column"].upper())
        if e["scores"] is None:
            assert got is None
            continue
        assert got is not None and list(got) == e["scores"], e["column"]          # the same floats, bit for bit
        for tok in ("^", "$", "*", "+", "-"):
            if tok in e["column"]:
                seen.add(tok)
        if re.search(r"[+-]\d\d", e["column"]):
            seen.add("multi-digit")
        if e["column"] != e["column"].upper():
            seen.add("lower")
        n, sb, t, si = pm.column_integers(e["column"].upper())
        # the integers of the column give the same bins as the floats
        assert purity.bin_of(sb, n) == pm.float_bin(got[0]) and purity.bin_of(si, n) == pm.float_bin(got[1]), e["column"]
    assert seen == {"^", "$", "*", "+", "-", "multi-digit", "lower"}


def _check_twin(path, ranges, min_bq=13, exclude_flags=0x704):
    f = bam.BamFile(path)
    rows, hb, hi, scores, tallies = pm.expected_of(f.records, f.references, f.lengths, ranges, min_bq, exclude_flags)
    t_rows, t_hb, t_hi, t_tallies = pm.twin(path, f.references, ranges, len(rows), min_bq, exclude_flags)
    assert np.array_equal(t_rows, rows), np.nonzero((t_rows != rows).any(axis=1))[0][:10]
    assert np.array_equal(t_hb, hb) and np.array_equal(t_hi, hi)       # float-binned (writer) == integer-binned (twin)
    assert pm.tallies_agree(t_tallies, tallies), (t_tallies, dict(tallies))
    assert len(scores) == t_tallies["positions_covered"]
    return t_rows, t_tallies


def test_twin_on_golden_reads():
    path = os.path.join(GOLDEN, "data", "reads.bam")
    f = bam.BamFile(path)
    for ranges in pm.range_sets(list(zip(f.references, f.lengths))):
        rows, tallies = _check_twin(path, ranges)
    assert tallies["entries_counted"] > 0
    rows, tallies = _check_twin(path, [(n, 0, l) for n, l in zip(f.references, f.lengths)])
    assert tallies["star_entries"] > 0 and tallies["insertions_counted"] > 0 and tallies["records"] == 10


def test_twin_on_engineered_records(tmp_path):
    references, refs, records = cms_model.engineered_records()
    path = str(tmp_path / "eng.bam")
    bam.write_bam(path, references, records)
    for ranges in pm.range_sets(references):
        _check_twin(path, ranges)
    rows, tallies = _check_twin(path, [("eng", 0, references[0][1])])
    assert tallies["insertions_without_entry"] == 2 and tallies["insertions_hashed"] >= 2 and tallies["entries_ambiguous"] == 4
    assert tallies["entries_lowq"] >= 1 and tallies["records_flagged"] == 1      # 0x400 by the flags; 0x800 is not in 0x704


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_on_random_bams(tmp_path, seed):
    path = str(tmp_path / "r.bam")
    references, _ = cms_model.make_random_bam(path, seed)
    for ranges in pm.range_sets(references):
        for min_bq, flags in ((13, 0x704), (0, 0x904)):
            _check_twin(path, ranges, min_bq, flags)


def test_twin_on_window_and_deep_records(tmp_path):
    for name, (references, records) in (("w", pm.window_records()), ("d70", pm.deep_insertion_records(70)),
                                        ("d300", pm.deep_insertion_records(300))):
        path = str(tmp_path / f"{name}.bam")
        bam.write_bam(path, references, records)
        rows, tallies = _check_twin(path, [(references[0][0], 0, references[0][1])])
        if name.startswith("d"):
            n = int(name[1:])
            assert rows[49, 2] == n and tallies["insertions_hashed"] == 2 * n // 5


def test_bin_rule_equals_the_float_expression():
    lib = pm.load()
    checked = 0

    def vectors(n, parts, most):
        """the count vectors of n entries over `parts` symbols, largest count first (every multiset of counts once)"""
        if parts == 1:
            if n <= most:
                yield (n,)
            return
        for a in range(min(n, most), -1, -1):
            if a * parts < n:
                break
            for rest in vectors(n - a, parts - 1, a):
                yield (a,) + rest
    for n in range(1, 41):                                              # every base-count vector at n <= 40, in both orders
        for c in vectors(n, 5, n):
            S = sum(v * v for v in c)
            for order in (c, c[::-1]):
                x = 0
                for v in order:
                    x += (v / n) ** 2
                assert lib.pur_twin_bin(S, n) == pm.float_bin(x) == purity.bin_of(S, n), (order, n)
            checked += 1
    assert checked > 10000
    rng = np.random.default_rng(3)
    for _ in range(20000):
        n = int(rng.integers(1, 1001))
        if rng.random() < .5:                                           # base counts in a random order of the five symbols
            cuts = np.sort(rng.integers(0, n + 1, size=4))
            c = np.diff(np.concatenate([[0], cuts, [n]])).tolist()
            x = 0
            for v in c:
                x += (v / n) ** 2
        else:                                                           # insertions: the non-inserting reads first
            t = int(rng.integers(0, n + 1))
            k = int(rng.integers(1, 6))
            cuts = np.sort(rng.integers(0, t + 1, size=k - 1))
            vs = [v for v in np.diff(np.concatenate([[0], cuts, [t]])).tolist() if v]
            c = [n - t] + vs
            x = ((n - t) / n) ** 2
            for v in vs:
                x += (v / n) ** 2
        S = sum(v * v for v in c)
        assert lib.pur_twin_bin(S, n) == pm.float_bin(x), (c, n)
    assert lib.pur_twin_bin(1, 1) == 99 and lib.pur_twin_bin((1 << 20) - 1, (1 << 20) - 1) == 0


def test_key_is_injective_for_short_strings_and_hashed_for_long_ones():
    letters = "=ACMGRSVTWYHKDBN"
    keys = {}
    for k in range(0, 4):
        for s in itertools.product(letters, repeat=k):
            keys["".join(s)] = pm.key_of("".join(s))
    assert len(set(keys.values())) == len(keys) == 1 + 16 + 256 + 4096
    rng = np.random.default_rng(9)
    strings = {"".join(rng.choice(list(letters), size=int(rng.integers(4, 15)))) for _ in range(3000)}
    ks = {s: pm.key_of(s) for s in strings}
    assert len(set(ks.values())) == len(ks) and not set(ks.values()) & set(keys.values())
    for s, key in list(ks.items())[:50]:
        assert key >> 56 == len(s)
        assert all((key >> (4 * i)) & 15 == letters.index(ch) for i, ch in enumerate(s))
    a, b2 = "ACGTACGTACGTACG", "ACGTACGTACGTACT"
    assert pm.key_of(a) >> 56 == 0xFF and pm.key_of(a) != pm.key_of(b2) and pm.key_of(a) == pm.key_of(a)
    assert pm.key_of("A" * 14) >> 56 == 14 and pm.key_of("A" * 15) >> 56 == 0xFF and pm.key_of("A" * 15) != pm.key_of("A" * 16)


def test_region_parsing_and_the_header_symbol():
    refs, lens = ["chr1", "HLA:01", "c"], [1000, 500, 30]
    assert purity.parse_region(None, refs, lens) == [("chr1", 0, 1000), ("HLA:01", 0, 500), ("c", 0, 30)]
    assert purity.parse_region("chr1", refs, lens) == [("chr1", 0, 1000)]
    assert purity.parse_region("chr1:11", refs, lens) == [("chr1", 10, 1000)]
    assert purity.parse_region("chr1:11-20", refs, lens) == [("chr1", 10, 20)]
    assert purity.parse_region("chr1:1,001-2,000", ["chr1"], [5000]) == [("chr1", 1000, 2000)]
    assert purity.parse_region("chr1:900-5000", refs, lens) == [("chr1", 899, 1000)]
    assert purity.parse_region("HLA:01", refs, lens) == [("HLA:01", 0, 500)]
    assert purity.parse_region("HLA:01:5-6", refs, lens) == [("HLA:01", 4, 6)]
    for bad in ("chrX", "chr1:0-5", "chr1:9-3", "chr1:a-b"):
        with pytest.raises(ValueError):
            purity.parse_region(bad, refs, lens)
    assert purity.merged_positions([("c", 0, 10), ("c", 5, 20), ("c", 25, 99), ("chr1", -5, 3)], dict(zip(refs, lens)), refs) == 20 + 5 + 3
    pairs = purity.pair_summary([([1] + [0] * 99, [0] * 100), ([1] + [0] * 99, [2] + [0] * 99), ([4] + [0] * 99, [0] * 100), ([0] * 100, [1] + [0] * 99)])
    assert pairs[0]["base_counts"][0] == 2 and "base_ratio" not in pairs[0]
    assert pairs[1]["base_ratio"][0] == 2.0 and pairs[1]["ins_ratio"][0] == 0.5 and pairs[1]["base_ratio"][1] == 0
    from npore_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "npore_amd.h")).read()
    assert re.search(r"\bint npore_bam_purity\(npore_ctx \*ctx, npore_bam \*bam, int64_t n_ranges", header)
    assert "npore_bam_purity" in _lib.SIGNATURES and len(_lib.SIGNATURES["npore_bam_purity"][1]) == 13
    assert len(purity.PURITY_TALLIES) == 16 and purity.PURITY_TALLIES[:13] == pm.TALLY_NAMES
