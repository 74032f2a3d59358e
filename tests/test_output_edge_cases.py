"""The inputs of tests/output_edge_cases.py on the CPU: that each of them reaches the path it is built for -- indel runs
that slide 64 positions and more, more than 256 BGZF members, every alignment and length class of wave_copy -- and that
the host twins the GPU tests compare with agree with the oracle and the Python statements on them.  No GPU."""
import argparse
import collections

import numpy as np
import pytest

import oracle
import output_edge_cases as oc
from npore_amd import bam, cfg, cig, synth
from test_bam_match import ALL
from test_bam_out import decoded_lines, header_len, make_bam, split_records, write_native


# ---- 1. slides of 64 positions and more ------------------------------------------------------------------------------------
def probed_standardize(aln, ref, seq):
    """cig.standardize_runs with an instrumented copy of cig.push_indels_left_runs: -> (runs, [(op, slide, ending)]) with one
    entry per indel run that had a match run in front of it; ending 'exhausted' when the slide used the whole match run
    up, 'differ' when it stopped on a base that differs."""
    seen = []

    def push(runs, s_, push_op):
        out, p = [], 0
        for op, k in runs:
            if op != push_op:
                cig._push(out, op, k)
                if op == 0:
                    p += k
                continue
            m = out[-1][1] if out and out[-1][0] == 0 else 0
            s = 0
            while s < m and s_[p - s - 1] == s_[p - s - 1 + k]:
                s += 1
            if m:
                seen.append(("MID"[push_op], s, "exhausted" if s == m else "differ"))
            if s:
                out[-1][1] -= s
                if out[-1][1] == 0:
                    out.pop()
            cig._push(out, push_op, k)
            cig._push(out, 0, s)
            p += k
        return out

    runs = cig.to_runs(0 if c in "X=M" else (1 if c == "I" else 2) for c in aln)
    runs = cig.inss_before_dels_runs(push(runs, np.asarray(ref).tolist(), 2))       # stage A, over the reference
    runs = cig.inss_before_dels_runs(push(runs, np.asarray(seq).tolist(), 1))       # stage C, over the read
    return runs, seen


@pytest.fixture(scope="module")
def slides(tables):
    """the cases, and per context of SLIDE_CONTEXTS the oracle's raw strings and the probes of their standardisation"""
    sub, nps = tables
    refs, seqs, cigs, labels = oc.slide_cases()
    per = {}
    for r, mbr in oc.SLIDE_CONTEXTS:
        raws = [oracle.align(refs[k], seqs[k], cigs[k], sub, nps, r=r, max_b_rows=mbr) for k in range(len(refs))]
        per[(r, mbr)] = raws, [probed_standardize(raws[k], refs[k], seqs[k])[1] for k in range(len(refs))]
    return refs, seqs, cigs, labels, per


def test_slide_cases_are_what_the_module_says():
    refs, seqs, cigs, labels = oc.slide_cases()
    assert oc.SLIDE_TARGETS == (63, 64, 65, 127, 128, 129, 191, 192, 193) and oc.SLIDE_LONG == 257
    assert 300 <= len(refs) <= 1200 and max(max(len(a), len(b)) for a, b in zip(refs, seqs)) <= oc.SLIDE_MAX_BASES
    assert {l[0] for l in labels} == {"flank", "break", "foreign", "family"} and {l[1] for l in labels} == {"D", "I"}
    assert {l[2] for l in labels if l[0] == "family"} == {1, 2, 3}
    for ref, seq, cg in zip(refs, seqs, cigs):
        assert cg.count("=") + cg.count("D") == len(ref) and cg.count("=") + cg.count("I") == len(seq)
    r2, s2, c2, l2 = oc.slide_cases()
    assert all(np.array_equal(a, b) for a, b in zip(refs + seqs, r2 + s2)) and cigs == c2


@pytest.mark.parametrize("ctx", oc.SLIDE_CONTEXTS)
def test_slides_cross_every_round_of_the_probe(slides, ctx):
    """for D (stage A) and I (stage C), for slides that end on a differing base and for those that use the match run up:
    one less than, exactly and one more than one, two and three rounds of 64, and one of five rounds"""
    refs, seqs, cigs, labels, per = slides
    got = collections.defaultdict(set)
    for probes in per[ctx][1]:
        for op, s, ending in probes:
            got[(op, ending)].add(s)
    for op in "DI":
        for ending in ("differ", "exhausted"):
            seen = got[(op, ending)]
            assert set(oc.SLIDE_TARGETS) <= seen, (ctx, op, ending, sorted(set(oc.SLIDE_TARGETS) - seen))
            assert max(seen) >= oc.SLIDE_LONG, (ctx, op, ending, max(seen))
    # the families of short periods: blocks of I and D runs in the raw strings (stages B / D), and long slides among them
    fam = [k for k, l in enumerate(labels) if l[0] == "family"]
    if ctx == (30, 333):
        assert any("I" in per[ctx][0][k] and "D" in per[ctx][0][k] for k in fam)
    assert max(s for k in fam for _, s, _ in per[ctx][1][k]) >= oc.PROBE_ROUND


def test_no_slide_of_the_glue_test_reaches_a_round(tables):
    """tests/test_gpu_parity.py::test_device_glue_equals_host_glue never takes WaveProbe into a second round: the gap that
    test_gpu_output_edges.py closes.  (Should this fail one day because that test's reads changed: so much the better.)"""
    sub, nps = tables
    refs, seqs, cigs, contexts = oc.glue_test_inputs(synth.make_batch)
    assert len(refs) == 24 + 40 + 12 + 3 and contexts == [(30, 20000), (100, 700), (10, 37)]
    for r, mbr in contexts:
        longest = n = 0
        for k in range(len(refs)):
            raw = oracle.align(refs[k], seqs[k], cigs[k], sub, nps, r=r, max_b_rows=mbr)
            probes = probed_standardize(raw, refs[k], seqs[k])[1]
            n += len(probes)
            longest = max([longest] + [s for _, s, _ in probes])
        assert n > 5000 and longest < oc.PROBE_ROUND, (r, mbr, n, longest)


def test_host_glue_equals_the_python_statement_on_the_slides(slides):
    """npore_standardize_batch (the host's StdStream with ScalarProbe, what cig.standardize_batch calls) == the five passes
    of cig.standardize_runs == the instrumented copy above, on the oracle's strings of every case"""
    refs, seqs, cigs, labels, per = slides
    for ctx, (raws, _) in per.items():
        got = cig.standardize_batch(raws, refs, seqs)
        for k in range(len(refs)):
            want = "".join(f"{n}{c}" for c, n in cig.standardize_runs(raws[k], refs[k], seqs[k]))
            assert got[k] == want, (ctx, labels[k])
        for k in range(len(refs)):                                       # the instrumented copy moves what the original moves
            runs = cig.to_runs(0 if c in "X=M" else (1 if c == "I" else 2) for c in raws[k])
            runs = cig.inss_before_dels_runs(cig.push_indels_left_runs(runs, refs[k].tolist(), 2))
            runs = cig.inss_before_dels_runs(cig.push_indels_left_runs(runs, seqs[k].tolist(), 1))
            assert probed_standardize(raws[k], refs[k], seqs[k])[0] == runs, (ctx, labels[k])


# ---- 2. more than 256 members ----------------------------------------------------------------------------------------------
def test_member_cases_give_every_thread_of_the_placement_more_than_one_member():
    assert oc.PLACE_THREADS == 256 and oc.P == 65280
    for n_bytes, phase, n, seg, first_empty in oc.MEMBER_CASES:
        head, whole, tail = oc.member_cuts(n_bytes, phase)
        assert whole == n > oc.PLACE_THREADS and head + whole * oc.P + tail == n_bytes
        got_seg, shares = oc.place_shares(n)
        assert got_seg == seg == -(-n // oc.PLACE_THREADS) and seg > 1
        assert [t for t, (k0, k1) in enumerate(shares) if k0 == k1][0] == first_empty == -(-n // seg)
        assert sum(k1 - k0 for k0, k1 in shares) == n and all(a[1] == b[0] for a, b in zip(shares, shares[1:]))
        last = shares[first_empty - 1]
        assert (last[1] - last[0] < seg) == (n % seg != 0)
    assert [oc.member_cuts(nb, ph)[0] for nb, ph, *_ in oc.MEMBER_CASES] == [0, 3, oc.P - 777]
    assert [c[2] % c[3] for c in oc.MEMBER_CASES] == [1, 0, 2]              # the last share that is not empty: partial, full, partial
    # mixed_buffer's contents repeat with the number of kinds: the host twin codes a few dozen payloads at any phase
    assert len(ALL) <= 16 and np.gcd(5, len(ALL)) == 1


# ---- 3. wave_copy by alignment and length class -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def copies(tables, tmp_path_factory):
    """the BAM of copy_records(), the final CIGARs of its reads from the oracle, the host twin's records"""
    sub, nps = tables
    references, contig, records, pairs = oc.copy_records()
    finals = []
    for ref, seq, ops in pairs:
        raw = oracle.align(ref, seq, ops, sub, nps, r=30)
        finals.append(cig.collapse_cigar(cig.standardize(raw, ref, seq)))
    d = tmp_path_factory.mktemp("copies")
    src = str(d / "copies.bam")
    make_bam(src, references, records)
    return src, d, references, contig, records, finals


def _final_ops(finals):
    return [sum(1 for c in f if c in "MID") for f in finals]


def test_copy_records_are_the_product():
    references, contig, records, pairs = oc.copy_records()
    assert len(records) == len(oc.NAME_LENGTHS) * len(oc.LEADS) * len(oc.SHORT_SL + oc.LONG_SL) == 408
    assert {len(r["name"]) + 1 for r in records} == {2, 3, 4, 5} and len({r["name"] for r in records}) > 200
    assert {(len(r["name"]), r["_lead"], r["_sl"]) for r in records} == {(a, b, c) for a in oc.NAME_LENGTHS for b in oc.LEADS for c in oc.SHORT_SL + oc.LONG_SL}
    assert {r["_lead"] & 1 for r in records} == {0, 1} and {(r["_lead"] >> 1) & 3 for r in records} == {0, 1, 3}
    for sl in oc.SHORT_SL + oc.LONG_SL:
        mine = [r for r in records if r["_sl"] == sl]
        assert {r["_trail"] for r in mine} == {0, 1} and {r["qual"] is None for r in mine} == {False, True}
        assert {r["cigar"][0][0] == 5 for r in mine} == {False, True}
        assert {oc._hp_bytes(r["hp"]) for r in mine} == {1, 2, 4} and any(r["hp"] is None for r in mine)
    assert [r["pos"] for r in records] == sorted(r["pos"] for r in records)
    assert all(r["pos"] + len(p[0]) <= q["pos"] - 3 for r, p, q in zip(records, pairs, records[1:]))
    assert all(contig[r["pos"]:r["pos"] + len(p[0])] == "".join("NACGT"[x] for x in p[0]) for r, p in zip(records, pairs))
    assert sum(any(op == 1 for op, _ in r["cigar"]) and any(op == 2 for op, _ in r["cigar"]) for r in records) == 4 * 6 * 9


def test_copy_layout_is_the_host_twins(copies):
    """the offsets copy_calls() works with are those of the twin's records and of the input's staged heads"""
    src, d, references, contig, records, finals = copies
    nb = bam.NativeBam(src, stream=False)
    idx, st = np.arange(len(records), dtype=np.int64), np.zeros(len(records), np.int32)
    stream = nb.format_bam(idx, finals, st)
    nb.close()
    _, offsets = oc.copy_calls(records, _final_ops(finals), len(records))
    assert offsets == [off for off, _ in split_records(stream)]
    assert len(stream) == offsets[-1] + oc.record_size(records[-1], _final_ops(finals)[-1])
    # a staged head is the input record up to the end of its qualities: all but its tags ('XAA!' and HP)
    data = bam._bgzf_decompress(src)
    for (off, rec), r in zip(split_records(data[header_len(data):]), records):
        aux = 4 + (0 if r["hp"] is None else 3 + oc._hp_bytes(r["hp"]))
        assert oc.staged_head_size(r) == len(rec) - aux, r["name"]


@pytest.mark.parametrize("batch_reads", [5, 1000])
def test_copy_calls_cover_every_alignment_and_length_class(copies, batch_reads):
    src, d, references, contig, records, finals = copies
    calls, _ = oc.copy_calls(records, _final_ops(finals), batch_reads)
    pairs = collections.defaultdict(set)
    classes = collections.defaultdict(set)
    clear = collections.defaultdict(set)
    for what, da, sa, nib, clear_low, head, words, tail in calls:
        pairs[(what, nib)].add((da, sa))
        clear[nib].add(clear_low)
        full_head = (4 - da) & 3
        if head < full_head:
            assert words == "0" and tail == 0
            classes[nib].add("n < head")
        if words == "0":
            classes[nib].add("no words")
        if tail == 0 and words != "0":
            classes[nib].add("no tail")
        classes[nib].add(("words", words))
        classes[nib].add(("tail", tail))
        classes[nib].add(("head", head))
    every = {(a, b) for a in range(4) for b in range(4)}
    for key in (("bases", 0), ("bases", 1), ("quals", 0)):
        assert pairs[key] == every, (key, sorted(every - pairs[key]))
    assert pairs[("cigar", 0)] == {(a, 0) for a in range(4)}             # the slots of the CIGAR words lie at multiples of 4
    want = {"n < head", "no words", "no tail"} | {("words", w) for w in ("0", "1-63", "64", "65")} | \
        {("tail", t) for t in range(4)} | {("head", h) for h in range(4)}
    for nib in (0, 1):
        assert want <= classes[nib], (nib, want - classes[nib])
        assert clear[nib] == {False, True}
    assert ("words", "66+") in classes[0]                                # (the qualities of the long reads; NIB 1 moves 261 bytes at most)


def test_copy_twin_decodes_back_to_the_input(copies):
    src, d, references, contig, records, finals = copies
    refs = {oc.COPY_CONTIG: contig}
    nb = bam.NativeBam(src, stream=False)
    idx, st = np.arange(len(records), dtype=np.int64), np.zeros(len(records), np.int32)
    out = str(d / "twin.bam")
    info = write_native(nb, idx, finals, st, out, 5)
    nb.close()
    assert info["records"] == len(records) and info["indexed"] == 1
    old = cfg.args
    cfg.args = argparse.Namespace(max_reads=0, regions=[(oc.COPY_CONTIG, 0, len(contig))])
    try:
        rds = list(bam.get_read_data(bam.BamFile(src), refs))
    finally:
        cfg.args = old
    assert len(rds) == len(records)
    assert decoded_lines(out, refs) == [bam.sam_line(rd, f) for rd, f in zip(rds, finals)]
    back = bam.BamFile(out)
    assert [r.query_name for r in back.records] == [r["name"] for r in records]
    assert [r.hp for r in back.records] == [r["hp"] or 0 for r in records]
