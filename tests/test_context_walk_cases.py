"""tests/context_walk_cases.py on the CPU: the walk covers every ordered pair of operations once, the quarters lose none, every
reference is computable without a GPU and holds what its operation is there for, and the walk's loop names the offending pair."""
import collections
import re

import numpy as np
import pytest

import context_walk_cases as cw
import scale_edge_cases as sc
from test_bam_out import split_records
import bam_cs_cases as cc


# ---- the walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 13])
def test_walk_covers_every_ordered_pair_once(n):
    w = cw.walk(n)
    assert len(w) == n * n + 1 and w[0] == w[-1] == 0
    seen = collections.Counter(cw.pairs(w))
    assert set(seen) == {(a, b) for a in range(n) for b in range(n)} and set(seen.values()) == {1}
    assert w == cw.walk(n)                                       # deterministic


def test_walk_of_the_thirteen_operations():
    assert len(cw.NAMES) == 13 == len(set(cw.NAMES))
    w = cw.walk(13)
    assert len(w) == 170 and len(set(cw.pairs(w))) == 169
    # both directions of every pair, so "large then small" as well as "small then large", and every operation behind itself
    assert all((b, a) in set(cw.pairs(w)) for a, b in cw.pairs(w))


@pytest.mark.parametrize("n,k", [(13, 4), (4, 4), (3, 2), (13, 7)])
def test_quarters_lose_no_pair(n, k):
    w = cw.walk(n)
    q = cw.quarters(w, k)
    assert len(q) == k and all(len(p) >= 2 for p in q)
    assert all(a[-1] == b[0] for a, b in zip(q, q[1:])) and q[0][0] == w[0] and q[-1][-1] == w[-1]
    assert collections.Counter(p for piece in q for p in cw.pairs(piece)) == collections.Counter(cw.pairs(w))
    assert max(map(len, q)) - min(map(len, q)) <= 1


# ---- the references ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    return cw.ops()


def test_every_setting_has_another_legal_value():
    assert all(a != b for a, b in cw.SETTINGS.values()) and len(cw.SETTINGS) == 9


@pytest.mark.parametrize("name,n_reads,longest", [("align30", 6, 700), ("align100_groups", 24, 2800), ("align260", 3, 600)])
def test_align_references(ops, name, n_reads, longest):
    refs, seqs, cigs = cw.align_reads(name)
    want = ops[name].want
    assert len(want["strings"]) == n_reads == len(refs) and max(map(len, refs + seqs)) <= longest
    assert not want["status"].any()
    text = "".join(want["strings"])
    assert re.search("II", text) and re.search("DD", text)       # runs of I and of D
    assert all(len(s) > 100 for s in want["strings"])


def test_align100_needs_a_group_per_read():
    """24 reads under tb_budget_mb = 8 at r = 100: a read's traceback words alone take more than half the budget (run_core's
    estimate: (2 L + chunks) * tb_stride(r) * 4 bytes), so every read is a group of its own and the three work sets rotate"""
    refs, seqs, cigs = cw.align_reads("align100_groups")
    need = [2 * len(c) * ((2 * 100 + 1 + 3) & ~3) * 4 for c in cigs]
    assert min(need) > 4 << 20 and len(need) >= 4 * 3


def test_align_final_reference(ops):
    want = ops["align_final"].want
    assert want["status"].tolist().count(32) == 1 and want["strings"][2] == "" and want["status"][2] == 32
    kept = [s for s in want["strings"] if s]
    assert len(kept) == 5 and all(re.fullmatch(r"(\d+[MID])+", s) for s in kept) and any("I" in s for s in kept) and any("D" in s for s in kept)


def test_annotation_references(ops):
    seq = cw.np_info_sequence()
    assert len(seq) == 20_000 > sc.NP_INFO_SEG
    info = ops["np_info"].want["info"]
    assert info.shape == (20_000, 2, 6) and info[sc.NP_INFO_SEG, 0, 5] == 30       # the planted hexamer starts on the border
    assert (info[sc.NP_INFO_SEG + 1:, 0] != 0).any()
    slices = cw.region_slices()
    assert len(slices) == 171 and sc.scan_per(171, 6) == 2
    regions = ops["np_regions"].want["regions"]
    assert len(regions) == 171 and sum(len(r) for per in regions for r in per) > 400


def test_pileup_references(ops):
    _, tallies = cw.confusion_expected(cw.shipped())
    assert tallies["copy_insertion"] > 0 and tallies["copy_deletion"] > 0
    want = ops["confusion"].want
    assert sum(int(m.sum()) for m in want["matrices"]) > 1000 and want["tallies"]["records"] > 30
    pur = ops["purity64"].want
    assert pur["tallies"]["insertions_hashed"] > 0 and pur["tallies"]["insertions_counted"] > 0 and cw.purity_windows() > 1
    assert len(pur["scores"]) > 100 and pur["rows"].shape[0] == sum(l for _, l in cw.pileup_files()[2])


def test_file_references(ops):
    sam = ops["file_sam"].want
    assert len(sam["status"]) == 12 and sam["status"].tolist().count(32) == 1 and sam["status"][7] == 32
    assert sam["text"].count(b"\n") == 11
    cigars = [l.split(b"\t")[5] for l in sam["text"].splitlines()]
    assert any(b"I" in c for c in cigars) and any(b"D" in c for c in cigars)
    tags = ops["file_bam_tags"].want
    assert len(tags["status"]) == 40 and tags["status"].tolist().count(32) == 1
    recs = split_records(tags["records"])
    assert len(recs) == 39 and len(tags["records"]) > 65280                        # more than one BGZF member
    cs = "".join(cc.new_tags_of(rec)[0] for _, rec in recs)
    assert "*" in cs and "+" in cs and "-" in cs and "=" in cs                     # the long form
    one = ops["onepass_huffman"].want
    assert one["bad"] == [(7, 32)] and one["selected"] == 12 and len(split_records(one["records"])) == 11
    late = ops["err_contig_late"].want["prefixes"]
    assert len(late) == 2 and late[0] == b"" and late[1].count(b"\n") == 7 and sam["text"].startswith(late[1])


def test_other_tables_give_other_references():
    a, b = cw.ops(), cw.ops(cw.family())
    assert (b["align30"].t.max_n, b["align30"].t.max_l) == (4, 20)
    assert a["align30"].want["strings"] != b["align30"].want["strings"]
    assert a["np_info"].want["info"].shape[2] == 6 and b["np_info"].want["info"].shape[2] == 4
    assert a["file_sam"].want["text"] != b["file_sam"].want["text"]


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def _stub(bad_pair=None, raises_at=None, drifts=None):
    """operations as integers; the result of an operation is its own number, unless the one before it was bad_pair[0]"""
    state = {"prev": None, "calls": 0}

    def run(name):
        prev, state["prev"] = state["prev"], name
        state["calls"] += 1
        if raises_at is not None and state["calls"] == raises_at:
            raise RuntimeError("boom")
        if bad_pair is not None and (prev, name) == bad_pair:
            return {"value": name + 1000, "extra": 0}
        return {"value": name, "extra": state["calls"] if drifts == name else 0}
    return run, state


@pytest.mark.parametrize("bad_pair", [(3, 5), (5, 3), (7, 7), (12, 0)])
def test_the_loop_names_the_offending_pair(bad_pair):
    w = cw.walk(13)
    at = cw.pairs(w).index(bad_pair) + 1
    run, _ = _stub(bad_pair)
    failures = cw.run_walk(w, run, lambda name: {"value": name})
    assert len(failures) == 1
    f = failures[0]
    assert (f.prev, f.op, f.index) == (bad_pair[0], bad_pair[1], at) and w[at] == bad_pair[1] and w[at - 1] == bad_pair[0]
    assert f"walk[{at}]: {bad_pair[0]} -> {bad_pair[1]}" in repr(f)
    # ... and in quarters, with the offsets of the pieces
    found, offset = [], 0
    for piece in cw.quarters(w):
        run, _ = _stub(bad_pair)
        found += cw.run_walk(piece, run, lambda name: {"value": name}, offset=offset)
        offset += len(piece) - 1
    assert [(f.prev, f.op, f.index) for f in found] == [(bad_pair[0], bad_pair[1], at)]
    # a clean stub: nothing
    run, _ = _stub()
    assert cw.run_walk(w, run, lambda name: {"value": name}) == []


def test_the_loop_stops_at_an_exception_and_sees_drift():
    w = cw.walk(4)
    run, state = _stub(raises_at=6)
    failures = cw.run_walk(w, run, lambda name: {"value": name})
    assert len(failures) == 1 and failures[0].index == 5 and "raised RuntimeError: boom" in failures[0].why and state["calls"] == 6
    assert (failures[0].prev, failures[0].op) == (w[4], w[5])
    # a key the reference does not hold that changes between the occurrences of operation 2
    run, _ = _stub(drifts=2)
    failures = cw.run_walk(w, run, lambda name: {"value": name})
    assert [f.op for f in failures] == [2] * (w.count(2) - 1) and all("first occurrence" in f.why for f in failures)
    # ... unless the operation says that only `value` has to repeat
    run, _ = _stub(drifts=2)
    assert cw.run_walk(w, run, lambda name: {"value": name}, steady_of=lambda name: (lambda got: {"value": got["value"]})) == []
