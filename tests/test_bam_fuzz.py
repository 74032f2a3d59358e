"""Random input and final CIGARs through the record chain of --records full, host side: the reads of bam_fuzz_cases (about 100 a
seed; inputs over M I D = X P with words of length 0 and clips, finals that are the input's canonical form, a near miss of it, the
input's words as they stand, or unrelated words over all nine ops) under all 48 option sets md x cs {none, short, long} x de x eqx
x oc -- the host twin npore_bam_format_bam_full_pass against the Python statement, byte for byte, without and with a pass mask;
the report of which seam of the device walks each seed hits; and the record buffer's bound as the file pipeline and the debug
entry sum it (tests/model/record_bounds.cpp over csrc/hostio.hpp's record_bound) against the statement's record sizes.  No GPU here: the device side
of the same reads is tests/test_gpu_bam_fuzz.py.

The statement is assembled from each read's tag texts, computed once (bam_fuzz_cases.read_texts / assemble); one seed goes
through bam.full_record itself under all 48 sets and holds that assembly to it.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from npore_amd import bam
from conftest import REPO
from test_bam_out import split_records
import bam_full_cases as fc
import bam_fuzz_cases as fz
import bam_oc_cases as oc
import long_cigar_cases as lc


def open_all(bp, fa):
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in zip(nb.references, nb.lengths)], pass_mask=bam.PASS_FLAGS)      # (the records that would pass too)
    return nb, nf, idx


@pytest.fixture(scope="module")
def seeds(tmp_path_factory):
    """per seed: the files, the input records as they lie in the file, the code arrays and every read's tag texts -- once"""
    tmp = tmp_path_factory.mktemp("bam_fuzz")
    out = {}
    for seed in fz.SEEDS:
        references, refs, records, finals, status = fz.fuzz_reads(seed)
        bp, fa = fc.write_inputs(tmp, references, refs, records, f"s{seed}")
        raws, packs = fc.input_records(bp), fz.fuzz_packs(seed)
        assert len(raws) == len(records)
        texts = [fz.read_texts(raw, rc, sc, fin) for raw, (rc, sc), fin in zip(raws, packs, finals)]
        out[seed] = dict(bp=bp, fa=fa, records=records, finals=finals, status=status, raws=raws, packs=packs, texts=texts)
    return out


# ---- 1. the seeds hit every seam they were picked for ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.SEEDS)
def test_every_situation_occurs(seed):
    """a condition on the inputs, not a measurement: the seeds were picked so that it holds"""
    _, _, records, finals, status = fz.fuzz_reads(seed)
    assert 90 <= len(records) <= 110 and [r["pos"] for r in records] == sorted(r["pos"] for r in records)
    assert len({r["name"] for r in records}) == len(records) and {len(r["name"]) for r in records} >= {1, 2, 3, 4, 5, 6}
    assert max(len(r["cigar"]) for r in records) <= 264 and max(n for r in records for _, n in r["cigar"]) <= 200
    for r in records:
        assert len(r["seq"]) == sum(n for op, n in r["cigar"] if op in lc.CONSUMES_QUERY) > 0, r["name"]
    count = fz.situations(records, finals, fz.fuzz_packs(seed))
    print(seed, count)
    assert set(count) == set(fz.SITUATIONS)
    assert not [name for name, n in count.items() if n < 1]


def test_situations_on_reads_written_by_hand():
    """the report itself, on reads whose situations are known: bam_oc_cases' and bam_eqx_cases' crafted reads name them"""
    import bam_eqx_cases as ec
    _, refs, records, finals = oc.oc_reads()[:4]
    by = {r["name"]: k for k, r in enumerate(records)}

    def of(names, recs=records, fins=finals, ctg=refs["ctg"]):
        pick = [by[n] for n in names] if recs is records else names
        rs = [recs[k] for k in pick]
        return fz.situations(rs, [fins[k] for k in pick], [lc.expected_pack(r, r["cigar"], ctg)[:2] for r in rs])
    c = of(["zero_edges"])
    assert c["zero_word_input_lane0"] == c["zero_word_input_lane63"] == c["unchanged"] == 1 and c["zero_tile_of_input"] == 0
    c = of(["zero_tile", "zero_tile_off"])
    assert c["zero_tile_of_input"] == 2 and c["input_run_merges_over_tile_seam"] == 2 and c["unchanged"] == c["changed"] == 1
    c = of(["straddle", "n65_same"])
    assert c["input_run_merges_over_tile_seam"] == 1 and c["unchanged"] == 2
    c = of(["n129_last", "n64_last"])
    assert c["near_miss_last_word"] == 2 and c["near_miss_first_word"] == 0 and c["final_past_read"] == 2
    c = of(["shorter_64", "longer_65", "second_tile"])
    assert c["final_fewer_words"] == c["final_more_words"] == 1 and c["near_miss_last_word"] == 2 and c["changed"] == 3
    assert of(["refused"])["refused"] == 1 and of(["secondary"])["passes_under_0x904"] == 1 and of(["has_oc_same"])["own_oc_tag"] == 1
    _, erefs, erecs, efins, _ = ec.eqx_reads()
    eby = {r["name"]: k for k, r in enumerate(erecs)}
    for letter in "IDN":                                         # an I, a D, an N as the first word of a tile behind an open X run
        c = of([eby[f"tile_{letter}"]], erecs, efins, erefs["ctg"])
        assert c[f"tile_first_{letter}_behind_open_X"] == 1 and sum(c[f"tile_first_{o}_behind_open_{k}"] for o in "IDN" for k in ("X", "EQ")) == 1
    c = of([eby["three_words"], eby["no_words"], eby["past_end"]], erecs, efins, erefs["ctg"])
    assert c["empty_final"] == 1 and c["final_past_reference"] == c["final_past_read"] == 1 and c["compared_run_over_tile_seam"] == 0
    # a count that gets another digit behind the end of a round of 64 positions, in one word of 130 positions
    rec = dict(name="x", flag=0, cigar=[(0, 130)], tags=b"", qual=None, _status=0)

    def seams(*differ):
        rc = np.ones(130, np.uint8)
        sc = rc.copy()
        sc[list(differ)] = 2
        c = fz.situations([rec], ["130M"], [(rc, sc)])
        assert c["md_count_10_over_round_seam"] == c["cs_count_10_over_round_seam"] and c["md_count_100_over_round_seam"] == c["cs_count_100_over_round_seam"]
        return c["md_count_10_over_round_seam"], c["md_count_100_over_round_seam"]
    assert seams(3, 129) == (0, 1)                               # 60 at the first seam, 124 at the second, 125 written
    assert seams(60, 129) == (1, 0)                              # 3, 67, 68 written
    assert seams(129) == (0, 1)                                  # 64, 128, 129 written
    assert seams(63, 127) == (0, 0)                              # 0 at either seam, 63 written
    assert seams(20, 40, 62) == (1, 0)                           # 1 at the first seam; the closing count is 67
    assert seams(*range(0, 130, 5)) == (0, 0)


# ---- 2. the assembly from texts is the statement ---------------------------------------------------------------------------------------
def test_assembly_is_full_record(seeds):
    """bam_fuzz_cases.assemble against bam.full_record itself: one seed, all 48 option sets, both masks"""
    s = seeds[fz.SEEDS[0]]
    for kw in fz.OPTION_SETS:
        want = fz.statement_stream(s["raws"], s["records"], s["packs"], s["finals"], s["status"], **kw)
        assert fz.assembled_stream(s["texts"], s["raws"], s["records"], s["status"], **kw) == want, fz.set_name(kw)
    assert len(split_records(want)) == len(s["records"]) - 3     # (the refused reads have no record)
    for mask in (0x904, 0x100):
        want = fz.statement_stream(s["raws"], s["records"], s["packs"], s["finals"], s["status"], mask=mask, **fz.FULL_SET)
        assert fz.assembled_stream(s["texts"], s["raws"], s["records"], s["status"], mask=mask, **fz.FULL_SET) == want


# ---- 3. host twin == statement, byte for byte, under every option set -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.SEEDS)
def test_host_twin_equals_statement(seeds, seed):
    s = seeds[seed]
    nb, nf, idx = open_all(s["bp"], s["fa"])
    assert len(idx) == len(s["records"])
    sizes = set()
    for kw in fz.OPTION_SETS:
        got = nb.format_bam_full(nf, idx, s["finals"], s["status"], **kw)
        want = fz.assembled_stream(s["texts"], s["raws"], s["records"], s["status"], **kw)
        assert got == want, (fz.set_name(kw), fz.describe_difference(got, want, s["records"], s["finals"], s["status"]))
        sizes.add(len(got))
    assert len(sizes) == 48                                      # (no two option sets write the same stream)
    nb.close(); nf.close()


@pytest.mark.parametrize("mask", [0x904, 0x100])
def test_host_twin_with_a_pass_mask(seeds, mask):
    s = seeds[fz.SEEDS[0]]
    nb, nf, idx = open_all(s["bp"], s["fa"])
    for kw in fz.OPTION_SETS:
        got = nb.format_bam_full(nf, idx, s["finals"], s["status"], pass_mask=mask, **kw)
        want = fz.assembled_stream(s["texts"], s["raws"], s["records"], s["status"], mask=mask, **kw)
        assert got == want, (fz.set_name(kw), fz.describe_difference(got, want, s["records"], s["finals"], s["status"]))
    passed = [raw for raw, r, st in zip(s["raws"], s["records"], s["status"]) if r["flag"] & mask and not st & 32]
    assert passed and all(raw in got for raw in passed)
    nb.close(); nf.close()


def test_mask_sets_cover_every_option():
    for key, on in (("md", True), ("de", True), ("eqx", True), ("oc", True), ("cs", "short"), ("cs", "long")):
        assert sum(kw[key] == on for kw in fz.MASK_SETS) >= 2 and sum(not kw[key] for kw in fz.MASK_SETS) >= 2, key
    assert len(fz.OPTION_SETS) == 48 and len({fz.set_name(kw) for kw in fz.OPTION_SETS}) == 48 and fz.FULL_SET in fz.OPTION_SETS


# ---- 4. the record buffer's bound ----------------------------------------------------------------------------------------------------
def terms_of(l_rn, rl, sl, l_seq, aux, words, kw):
    """the bound's terms as csrc/hostio.hpp's comment states them, written out once more: (what a record has for certain, what the
    terms allow on top of it)"""
    fixed = 36 + l_rn + (l_seq + 1) // 2 + l_seq + aux
    allowed = 4 * (rl + sl) + 32 + 7 + 16                        # the final's words, four clip words and eight bytes, NM, placeholder + CG head
    if kw["md"]:
        allowed += 4 + 3 * rl + 11
    if kw["cs"] or kw["de"]:
        allowed += 4 + 3 * (rl + sl) + 7
    if kw["oc"]:
        allowed += 4 + 10 * words
    return fixed, allowed


def test_record_bound_holds(tmp_path, seeds):
    """The file pipeline's bound of a batch's record bytes is a sum over its reads of csrc/hostio.hpp's record_bound
    (csrc/file_pipeline.hpp plan_staged_heads, which slot_pack_heads and the debug entry both are); a term that is too small
    fails a run with "BAM record buffer overflow" on the one read dense enough.  Per read and option set: the statement's
    record is no longer than the sum, and the sum is what the terms' own statement gives -- no more.  The reads: those of
    every seed whose final is the input's canonical form or a near miss of it, and bam_fuzz_cases.dense_reads.
    The bound of a CALLER's final words (the debug entry's: words_final_extent) is held to the statement's record on every
    read of every seed that is not refused -- finals past or short of the reference or the read and empty finals included --
    and on the dense reads.
    Measured (printed, not asserted): the largest bound / size is 12.83 -- 1078 bytes for a record of 84 -- on seed 108's read
    `qqqq40`, 5H 127D 2M under de + oc: de alone takes the whole cs term, three bytes per covered position, for a tag of seven.
    Among the dense reads the bound is closest on `md` ((1M 1D) x 300, all differing) under md alone, 1.35, and on `mi`
    ((1M 1I) x 300) under eqx alone, 1.37; their largest, 9.85, is `alt`'s (one 600M, every second position differing) under
    de + oc, for the same reason as above."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "record_bounds")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(REPO, "tests", "model", "record_bounds.cpp"), "-lz", "-pthread"])
    reads, own = [], []                                          # (name, raw, rc, sc, final, texts); whether the final is a batch's own
    for seed, s in seeds.items():
        for k, (r, raw, (rc, sc), fin, t) in enumerate(zip(s["records"], s["raws"], s["packs"], s["finals"], s["texts"])):
            if not r["_status"] & 32:
                reads.append((f"{seed}:{r['name']}", raw, rc, sc, fin, t))
                own.append(k % 4 < 2)
    references, refs, records, finals = fz.dense_reads()
    bp, _ = fc.write_inputs(tmp_path, references, refs, records, "dense")
    for r, raw, fin in zip(records, fc.input_records(bp), finals):
        rc, sc, _ = lc.expected_pack(r, r["cigar"], refs["ctg"])
        reads.append((r["name"], raw, rc, sc, fin, fz.read_texts(raw, rc, sc, fin)))
        own.append(True)
    assert sum(own) > 120 and len(own) - sum(own) > 120
    rows = []
    for name, raw, rc, sc, fin, t in reads:
        aux = t["aux"]
        rows.append((t["fixed"][2], len(rc), len(sc), t["fixed"][5], len(bam.filter_aux(aux)), len(bam.filter_aux(aux, oc=True)),
                     len(oc.runs_of(t["oc"]))))
    cases = str(tmp_path / "reads.bin")
    with open(cases, "wb") as fh:
        fh.write(b"".join(struct.pack("<7q", *row) for row in rows))
    callers = str(tmp_path / "finals.bin")                       # per read: the count and the words of its final, as a caller gives them
    with open(callers, "wb") as fh:
        for name, raw, rc, sc, fin, t in reads:
            words = [(n << 4) | op for op, n in oc.runs_of(fin)]
            fh.write(struct.pack(f"<q{len(words)}I", len(words), *words))
    out = subprocess.run([exe, cases, callers], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    bounds = [[int(x) for x in line.split()] for line in out.stdout.splitlines()]
    assert len(bounds) == 2 * len(reads) and all(len(b) == 48 for b in bounds)
    bounds, caller_bounds = bounds[:len(reads)], bounds[len(reads):]
    sizes = [[len(fz.assemble(t, **kw)) for kw in fz.OPTION_SETS] for name, raw, rc, sc, fin, t in reads]
    for (name, *_), size, bound in zip(reads, sizes, caller_bounds):
        for kw, sz, cap in zip(fz.OPTION_SETS, size, bound):
            assert sz <= cap, ("a caller's final", name, fz.set_name(kw), sz, cap)
    keep = [k for k, o in enumerate(own) if o]                   # from here on: the file pipeline's bound, of a batch's own finals
    reads, rows, bounds, sizes = ([v[k] for k in keep] for v in (reads, rows, bounds, sizes))
    worst, best = (0.0, None), (1e9, None)
    for (name, raw, rc, sc, fin, t), row, bound, size_row in zip(reads, rows, bounds, sizes):
        for kw, cap, size in zip(fz.OPTION_SETS, bound, size_row):
            fixed, allowed = terms_of(row[0], row[1], row[2], row[3], row[5] if kw["oc"] else row[4], row[6], kw)
            assert size <= cap, (name, fz.set_name(kw), size, cap)
            assert cap == fixed + allowed and size >= fixed, (name, fz.set_name(kw), size, cap, fixed, allowed)
            worst = max(worst, (cap / size, (name, fz.set_name(kw), size, cap)))
            best = min(best, (cap / size, (name, fz.set_name(kw), size, cap)))
    print("largest bound / size:", worst, "smallest:", best)
    for (name, raw, rc, sc, fin, t), bound in zip(reads[-5:], bounds[-5:]):
        ratios = [(cap / len(fz.assemble(t, **kw)), fz.set_name(kw)) for kw, cap in zip(fz.OPTION_SETS, bound)]
        print(" dense read", name, "smallest", min(ratios), "largest", max(ratios))
    # the dense reads take of their term what the rule says they take: the bound's factor is no guess
    by = {name: t for name, _, _, _, _, t in reads}
    n = len(by["md"]["md"]) // 5
    assert by["md"]["md"] == "".join(f"0{a}0^{b}" for a, b in zip(refs["ctg"][records[0]["pos"]:][0:2 * n:2], refs["ctg"][records[0]["pos"]:][1:2 * n:2])) + "0"
    assert len(by["alt"]["cs"]["short"]) == len(by["alt"]["cs"]["long"]) == 5 * n and len(oc.runs_of(by["alt"]["eqx"])) == 2 * n
    assert len(by["all_x"]["cs"]["short"]) == 3 * 2 * n and len(by["mi"]["cs"]["long"]) == 4 * n
    assert by["oc"]["changed"] and len(by["oc"]["oc"]) == 2 * 10 + 2 * 2 * n


# ---- 5. the crafted read that is long only through the split: host twin == statement --------------------------------------------------------
def test_split_long_read_on_the_host(tmp_path):
    import bam_eqx_cases as ec
    references, refs, records, finals = fz.split_long_read()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "split")
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in references])
    rc, sc, _ = lc.expected_pack(records[0], records[0]["cigar"], refs["ctg"])
    raw, = fc.input_records(bp)
    assert bam.cigar_changed(oc.inner(records[0]["cigar"]), finals[0]) and len(oc.runs_of(bam.eqx_of(rc, sc, finals[0]))) + 2 == 65536
    for kw in (fz.FULL_SET, dict(fz.FULL_SET, eqx=False), dict(fz.EMPTY_SET, eqx=True, oc=True)):
        got = nb.format_bam_full(nf, idx, finals, np.zeros(1, np.int32), **kw)
        assert got == bam.full_record(raw, rc, sc, finals[0], **kw), fz.set_name(kw)
        assert ec.record_cigar_text(got)[1] == (2 if kw["eqx"] else 4)
        assert oc.oc_of_record(got)[1][-2:] == ([b"OC", b"CG"] if kw["eqx"] else [b"de", b"OC"])
    nb.close(); nf.close()
