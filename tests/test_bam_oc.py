"""The OC tag of the FULL records (--records full --oc, NPORE_TAG_OC), host side: the rule of npore_amd/csrc/oc_rec.hpp through its
Python statement (bam.cigar_changed, bam.oc_of, bam.full_record(oc=True)), its host twin npore_bam_format_bam_full_pass and the
header's sequential code under the sanitizers -- texts pinned by hand, the crafted reads of bam_oc_cases (which check themselves
here), inputs of more than 65 535 words, a pass mask, the surface, and the reference's own finals on the pipeline's reads.
No GPU here: the final CIGARs are given.
"""
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from npore_amd import bam, _lib
from conftest import GOLDEN, REPO
from test_bam_out import split_records
import bam_full_cases as fc
import bam_oc_cases as oc
from full_record_driver import host_full

EOF, PART, DEFLATE, MATCH, FULL, MD = bam.OUT_EOF, bam.OUT_PART, bam.OUT_DEFLATE, bam.OUT_MATCH, bam.OUT_FULL, bam.OUT_MD      # npore_bam_set_output's flags
CS, CS_LONG, DE = bam.TAG_CS, bam.TAG_CS_LONG, bam.TAG_DE                  # npore_bam_set_output_tags' word
ALL_TAGS = dict(md=True, cs="long", de=True, eqx=True)
COMBOS = {"alone": dict(), "tags": ALL_TAGS}
OC, EQX = bam.TAG_OC, bam.CIGAR_EQX


def open_all(bp, fa):
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in zip(nb.references, nb.lengths)], pass_mask=bam.PASS_FLAGS)      # (the secondary record too)
    return nb, nf, idx


# ---- 1. the Python statement against texts written out by hand ------------------------------------------------------------------
def test_statement_on_the_table():
    seen = [(c, f) for c, f, _, _ in oc.TABLE]
    for must in (("5=1X4=2I0D3M2M", "10M2I5M"), ("3M2M", "5M"), ("3M0I2M", "5M"), ("10M1I1D10M", "21M"), ("10M2I10M", "10M2I11M"),
                 ("10M2I10M", "10M2I"), ("10M2I10M", "10M2I10M1I"), ("", "")):
        assert must in seen
    for cig, fin, changed, text in oc.TABLE:
        words = oc.runs_of(cig)
        assert bam.cigar_changed(oc.inner(words), fin) is changed, (cig, fin)
        assert bam.oc_of(words) == cig                           # every word as it stands: clips, 0-length words, = and X
        assert oc.runs_of(bam.oc_of(words)) == words             # ... and the text parsed back gives the input's words
        assert (text == cig) if changed else text is None
    # literally, once more, what the rule says and the table cannot hold
    assert bam.oc_of([(5, 268435455), (4, 1), (0, 0), (7, 12), (8, 1), (6, 3), (3, 9), (2, 100)]) == "268435455H1S0M12=1X3P9N100D"
    assert bam.oc_of([]) == ""
    assert not bam.cigar_changed([(7, 3), (1, 0), (8, 2), (0, 1)], "6M") and bam.cigar_changed([(7, 3), (1, 1), (8, 2)], "6M")
    assert bam.cigar_changed([(0, 5)], "5=")                     # the final is compared as it stands, in M form
    big = [(0, (1 << 28) - 1)] * 20                              # a merged length beyond 32 bits is no word's length
    assert bam.cigar_changed(big, f"{((1 << 28) - 1) * 20 % (1 << 32)}M")
    # the option's word and the filter
    assert bam.output_tags(None, False) == 0 and bam.output_tags(None, False, oc=True) == OC and bam.output_tags("long", True, True, True) == OC | EQX | CS | CS_LONG | DE
    aux = b"XAZa\0" + b"OCZ5M\0" + b"NMC\x01" + b"XBC\x02"
    assert bam.filter_aux(aux) == b"XAZa\0" + b"OCZ5M\0" + b"XBC\x02" and bam.filter_aux(aux, oc=True) == b"XAZa\0" + b"XBC\x02"
    assert b"OC" not in bam.STALE_TAGS


# ---- 2. the cases module checks itself: the lanes it claims, the changed flags it pins -----------------------------------------
def test_cases_hit_the_lanes_they_claim():
    references, refs, records, finals, changed, pinned = oc.oc_reads()
    by = {r["name"]: (r, f) for r, f in zip(records, finals)}
    assert len(by) == len(records) and set(changed) == set(by)
    for name, (r, fin) in by.items():                            # the flag pinned by hand is the statement's
        assert bam.cigar_changed(oc.inner(r["cigar"]), fin) is changed[name], name
        if name in pinned:
            assert pinned[name] == bam.oc_of(r["cigar"]), name
        assert len(r["seq"]) == sum(n for op, n in r["cigar"] if op in (0, 1, 4, 7, 8)), name
    cig = lambda name: by[name][0]["cigar"]
    assert [len(cig(f"n{n}_same")) for n in (1, 63, 64, 65, 128, 129)] == [1, 63, 64, 65, 128, 129]
    for n in (1, 63, 64, 65, 128, 129):
        a, b = oc.runs_of(by[f"n{n}_last"][1]), cig(f"n{n}_last")
        assert a[:-1] == b[:-1] and a[-1][0] == b[-1][0] and a[-1][1] == b[-1][1] + 1
    assert len(oc.runs_of(by["shorter_64"][1])) == 64 and len(cig("shorter_64")) == 65 and len(oc.runs_of(by["longer_65"][1])) == 65
    w = cig("straddle")                                          # M in lane 63, = in lane 0 of the next tile: one run of 7
    assert w[63] == (0, 3) and w[64] == (7, 4) and w[62][0] == 1 and w[65][0] == 1 and oc.runs_of(by["straddle"][1])[63] == (0, 7)
    assert oc.runs_of(by["straddle_off"][1])[63] == (0, 6)
    w = cig("zero_edges")
    assert w[0][1] == 0 and w[63][1] == 0 and w[64][1] > 0 and w[62][0] != w[64][0] and all(n > 0 for _, n in w[1:63])
    w = cig("zero_tile")
    assert w[63] == (0, 2) and all(n == 0 for _, n in w[64:128]) and w[128] == (0, 5) and len({op for op, _ in w[64:128]}) == 7
    w = cig("three_tiles")
    end = next(k for k in range(61, len(w)) if w[k][1] > 0 and w[k][0] not in (0, 7, 8))      # the word that ends the run
    live = [k for k in range(61, end) if w[k][1] > 0]
    assert w[60][0] == 1 and live[0] == 61 and live[-1] // 64 - live[0] // 64 >= 2 and w[end] == (1, 1)
    assert {w[k][0] for k in live} == {0, 7, 8} and any(n == 0 for _, n in w[61:193])
    a, b = oc.runs_of(by["second_tile"][1]), cig("second_tile")
    assert [k for k in range(100) if a[k] != b[k]] == [80]
    # clips of every kind on either end; widths of 1 ... 9 digits up to 2^28 - 1; names of 1 ... 8 bytes; the other record kinds
    kinds = {(tuple(op for op, _ in c[:2] if op in (4, 5)), tuple(op for op, _ in c[-2:] if op in (4, 5))) for c in (cig(f"clip{k}") for k in range(16))}
    assert len(kinds) == 16
    digits = {len(str(n)) for name, (r, _) in by.items() if name.startswith("d") for _, n in r["cigar"]}
    assert digits >= set(range(1, 10)) and any(n == (1 << 28) - 1 for _, n in cig("d100000000"))
    assert {len(n) for n in by if changed[n] and n in "abcdefgh"} == set(range(1, 9))
    names = [r["name"] for r in records]
    assert names[names.index("refused") - 1] == "refused_before" and names[names.index("refused") + 1] == "refused_after" and by["refused"][0]["_status"] == 32
    assert b"OCZ" in by["has_oc_changed"][0]["tags"] and b"OCZ" in by["has_oc_same"][0]["tags"] and by["secondary"][0]["flag"] == 0x100
    # the long reads: more than 65 535 words in; one final short, one equal, one long and different
    _, _, lrec, lfin, lchg = oc.long_reads()
    assert all(len(r["cigar"]) > 0xFFFF for r in lrec) and [len(oc.runs_of(f)) > 0xFFFF for f in lfin] == [False, True, True]
    assert [bam.cigar_changed(r["cigar"], f) for r, f in zip(lrec, lfin)] == [True, False, True] == [lchg[r["name"]] for r in lrec]


def test_the_reference_alone_gives_both_kinds(tables):
    """the pipeline's file: on the reads that match, the reference's final is the input's nM; where the input's CIGAR has the
    deletion at the right end of the homopolymer, its standardisation moves it to the left end -- so some reads change, some do not"""
    references, refs, records = oc.pipeline_reads()
    assert 36 <= len(records) <= 44 and max(len(r["seq"]) for r in records) < 200
    finals = oc.oracle_finals(records, refs, tables)
    kinds = [bam.cigar_changed(oc.inner(r["cigar"]), f) for r, f in zip(records, finals)]
    for k, (r, f, chg) in enumerate(zip(records, finals, kinds)):
        body = oc.inner(r["cigar"])
        if k % 2 == 0:
            assert not chg and f == oc.text_of(body), (k, f)
        else:
            (_, a), _, (_, b) = body
            assert chg and f == f"{a - 4}M1D{b + 4}M", (k, f)
    reads = [k for k, r in enumerate(records) if not r["flag"] & bam.PASS_FLAGS]
    assert any(kinds[k] for k in reads) and not all(kinds[k] for k in reads)


# ---- 3. host twin == Python statement, byte for byte ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_oc")
    sets = {}
    for key, pack in (("oc", oc.oc_reads()), ("long", oc.long_reads())):
        references, refs, records, finals, changed = pack[:5]
        bp, fa = fc.write_inputs(tmp, references, refs, records, key)
        nb, nf, idx = open_all(bp, fa)
        assert len(idx) == len(records)
        status = np.array([r["_status"] for r in records], np.int32)
        got = {name: nb.format_bam_full(nf, idx, finals, status, oc=True, **kw) for name, kw in COMBOS.items()}
        plain = {name: nb.format_bam_full(nf, idx, finals, status, **kw) for name, kw in COMBOS.items()}
        nb.close(); nf.close()
        sets[key] = dict(bp=bp, fa=fa, refs=refs, records=records, finals=finals, changed=changed, pinned=pack[5] if key == "oc" else {},
                         status=status, got=got, plain=plain, raws=fc.input_records(bp))
    return tmp, sets


def test_host_twin_equals_statement(crafted):
    tmp, sets = crafted
    for key, s in sets.items():
        for name, kw in COMBOS.items():
            assert s["got"][name] == oc.want_stream(s["raws"], s["records"], s["refs"], s["finals"], s["status"], **kw), (key, name)
            # with the bit off: the bytes of the existing entry, which are the statement's without the option
            assert s["plain"][name] == oc.want_stream(s["raws"], s["records"], s["refs"], s["finals"], s["status"], oc=False, **kw), (key, name)
        assert s["got"]["alone"] != s["plain"]["alone"]


def test_which_records_carry_the_tag(crafted):
    tmp, sets = crafted
    for key, s in sets.items():
        kept = [r for r in s["records"] if not r["_status"]]
        for name, kw in COMBOS.items():
            recs, plain = split_records(s["got"][name]), split_records(s["plain"][name])
            assert len(recs) == len(plain) == len(kept)
            for (_, rec), (_, old), r in zip(recs, plain, kept):
                texts, tags = oc.oc_of_record(rec)
                own = [b"OC"] if b"OCZ" in r["tags"] else []
                if s["changed"][r["name"]]:                      # ONE tag: the input's words, behind de and in front of CG
                    assert texts == [oc.text_of(r["cigar"])], r["name"]
                    want_tail = [b"NM"] + ([b"MD", b"cs", b"de"] if kw else []) + [b"OC"]
                    at = tags.index(b"NM")
                    assert tags[at:at + len(want_tail)] == want_tail and tags[at + len(want_tail):] in ([], [b"CG"]), (r["name"], tags)
                    assert len(rec) == len(old) + 4 + len(texts[0]) - (len(own) and len(b"OCZ7M7I\0" if r["name"] != "secondary" else b"OCZ3M17I\0"))
                else:                                            # none, the input's own included
                    assert texts == [], r["name"]
                    assert len(rec) == len(old) - (len(own) and len(b"OCZ7M7I\0"))
                assert oc.oc_of_record(old)[0] == ([r["tags"].split(b"OCZ")[1].split(b"\0")[0].decode()] if own else [])      # without the bit it stays
                if r["name"] in s["pinned"]:
                    assert texts == [s["pinned"][r["name"]]], r["name"]
    # the order ... OC CG where the final is long, and the text of a long input comes from its CG tag's words
    s = sets["long"]
    (_, a), (_, b), (_, c) = split_records(s["got"]["tags"])
    assert oc.oc_of_record(a) == (["1M1I" * 33000], [b"RG", b"NM", b"MD", b"cs", b"de", b"OC"])
    assert oc.oc_of_record(b) == ([], [b"RG", b"NM", b"MD", b"cs", b"de", b"CG"])
    assert oc.oc_of_record(c) == (["1M1I" * 33000], [b"RG", b"NM", b"MD", b"cs", b"de", b"OC", b"CG"])
    # the decision does not depend on --eqx, --md or the tags: the same reads carry it in both runs
    for s in sets.values():
        with_tag = [[bool(oc.oc_of_record(rec)[0]) for _, rec in split_records(s["got"][name])] for name in COMBOS]
        assert with_tag[0] == with_tag[1] and any(with_tag[0]) and not all(with_tag[0])


@pytest.mark.parametrize("mask", [0x904, 0x100])
def test_with_a_pass_mask(crafted, mask):
    """the secondary record passes as it came, its own OC included; every other record is the statement's"""
    tmp, sets = crafted
    s = sets["oc"]
    nb, nf, idx = open_all(s["bp"], s["fa"])
    for kw in COMBOS.values():
        got = nb.format_bam_full(nf, idx, s["finals"], s["status"], pass_mask=mask, oc=True, **kw)
        assert got == oc.want_stream(s["raws"], s["records"], s["refs"], s["finals"], s["status"], mask=mask, **kw)
    k = [r["name"] for r in s["records"]].index("secondary")
    assert s["raws"][k] in [rec for _, rec in split_records(got)] and b"OCZ3M17I\0" in s["raws"][k]
    nb.close(); nf.close()


# ---- 4. the surface -----------------------------------------------------------------------------------------------------------------
def test_surface(crafted):
    tmp, sets = crafted
    s = sets["oc"]
    nb, nf, idx = open_all(s["bp"], s["fa"])
    lib = nb._lib
    hdr = open(os.path.join(REPO, "include", "npore_amd.h")).read()
    assert re.search(r"#define NPORE_TAG_OC 256\b", hdr) and re.search(r"#define NPORE_ABI_VERSION 2\b", hdr) and lib.npore_abi_version() == 2
    assert hdr.index("#define NPORE_CIGAR_EQX 32") < hdr.index("#define NPORE_TAG_OC 256") < hdr.index("int npore_bam_set_output_tags(")
    doc = hdr[hdr.index("#define NPORE_CIGAR_EQX 32"):hdr.index("#define NPORE_TAG_OC 256")]
    assert "--oc" in doc and "OC:Z" in doc and "UNCHANGED" in doc
    declared = set(re.findall(r"\b(npore_[a-z_0-9]+)\s*\(", hdr)) - {"npore_ctx"}
    assert declared == set(_lib.SIGNATURES)                      # no entry point was added for it
    # the ladder of test_bam_eqx.py::test_surface, for the bit alone and beside every valid word
    assert lib.npore_bam_set_output_tags(nb.handle, OC) != 0       # (a fresh handle writes SAM)
    for fmt, flags in ((0, 0), (1, EOF), (1, DEFLATE | EOF), (1, PART)):
        assert lib.npore_bam_set_output(nb.handle, fmt, None, flags) == 0
        for tags in (OC, OC | CS, OC | CS | CS_LONG | DE, OC | EQX):
            assert lib.npore_bam_set_output_tags(nb.handle, tags) != 0, (fmt, flags, tags)
    assert lib.npore_bam_set_output(nb.handle, 0, None, FULL | EOF) != 0                  # (FULL in SAM format is refused outright)
    for full in (FULL | EOF, FULL | PART, FULL | MD | EOF, FULL | DEFLATE | EOF):
        assert lib.npore_bam_set_output(nb.handle, 1, None, full) == 0
        for tags in [OC | eqx | word for eqx in (0, EQX) for word in (0, CS, CS | CS_LONG, DE, CS | CS_LONG | DE)]:
            assert lib.npore_bam_set_output_tags(nb.handle, tags) == 0, tags
        for tags in (OC | CS_LONG, OC | CS_LONG | DE, 8, OC | 8, 16, OC | 16, 64, OC | 64, 128, OC | 128, 512, OC | 512, 1 << 30, -1):
            assert lib.npore_bam_set_output_tags(nb.handle, tags) != 0, tags
    # set_output sets it back; the pass setter behind the bit keeps it
    assert lib.npore_bam_set_output(nb.handle, 1, None, FULL | EOF) == 0 and lib.npore_bam_set_output_tags(nb.handle, OC) == 0
    assert lib.npore_bam_set_output_pass(nb.handle, 0x904) == 0
    assert lib.npore_bam_set_output(nb.handle, 0, None, 0) == 0
    assert lib.npore_bam_set_output_tags(nb.handle, OC) != 0 and lib.npore_bam_set_output_tags(nb.handle, 0) != 0
    # npore_bam_write_file keeps refusing FULL, with the bit as without
    assert lib.npore_bam_set_output(nb.handle, 1, None, FULL | EOF) == 0 and lib.npore_bam_set_output_tags(nb.handle, OC) == 0
    out = tmp / "never.bam"
    assert lib.npore_bam_write_file(nb.handle, None, 0, 1, None, None, None, None, 0, str(out).encode()) != 0
    assert b"FULL records" in lib.npore_last_error() and not out.exists()
    # the host entries: accepted by _tags and _pass, refused beside an undefined bit or with FULL / a writer's bit in `flags`
    host = lambda entry, **words: host_full(nb, nf, idx, s["finals"], s["status"], entry=entry, **words)
    assert host("_tags", tags=OC) == (0, s["got"]["alone"])
    assert host("_pass", flags=MD, tags=OC | EQX | CS | CS_LONG | DE) == (0, s["got"]["tags"])
    assert host("_tags") == (0, s["plain"]["alone"])
    for flags, tags in ((0, OC | CS_LONG), (0, OC | 8), (0, OC | 128), (0, OC | 16), (FULL, OC), (EOF, OC), (64, OC)):
        assert host("_tags", flags=flags, tags=tags)[0] != 0, (flags, tags)
    # Python: the option needs records "full"
    for kw in (dict(out_format="bam", oc=True), dict(out_format="sam", oc=True), dict(out_format="bam", records="reference", oc=True)):
        with pytest.raises(ValueError):
            nb.set_output(**kw)
    nb.set_output("bam", records="full", oc=True)
    nb.set_output("bam", records="full", md=True, cs="long", de=True, pass_mask=0x904, eqx=True, oc=True)
    nb.set_output("sam")
    nb.close(); nf.close()


def test_cli_oc_needs_full_records(tmp_path):
    data = os.path.join(GOLDEN, "data")
    common = [sys.executable, "-m", "npore_amd.realign", "--bam", os.path.join(data, "reads.bam"), "--ref", os.path.join(data, "ref.fasta"),
              "--out_prefix", str(tmp_path / "bad"), "--oc"]
    for extra in ([], ["--out_format", "bam"], ["--out_format", "bam", "--records", "reference"], ["--out_format", "sam"]):
        out = subprocess.run(common + extra, cwd=REPO, capture_output=True, text=True, timeout=120)
        assert out.returncode == 1, out.stdout[-2000:] + out.stderr[-2000:]
        errors = [l for l in out.stdout.splitlines() if l.startswith("ERROR")]
        assert len(errors) == 1 and "--oc" in errors[0] and "--records full" in errors[0], out.stdout
        assert not os.path.exists(str(tmp_path / "bad.bam")) and not os.path.exists(str(tmp_path / "bad.sam"))
    text = " ".join(subprocess.run([sys.executable, "-m", "npore_amd.realign", "--help"], cwd=REPO, capture_output=True, text=True, timeout=120).stdout.split())
    assert "--oc" in text and "OC:Z" in text and "unchanged read has none" in text


# ---- 5. the header's sequential code under the sanitizers: the count is the stored length ----------------------------------------------
def test_sequential_code_under_sanitizers(tmp_path, crafted):
    tmp, sets = crafted
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = os.path.join(REPO, "tests", "model", "bam_oc_sanitize.cpp")
    exe = str(tmp_path / "bam_oc_sanitize")
    # (the runtimes linked statically: the program needs nothing preloaded and does not mind what is)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + san + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is missing")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + san + ["-o", exe, src])
    blob, want = [], []

    def case(words, final):
        fin = oc.runs_of(final)
        ci, cj = oc.clip_range(words)
        body = words[ci:cj]
        blob.append(struct.pack("<qqqq", len(words), ci, cj, len(fin)) + b"".join(struct.pack("<I", n << 4 | op) for op, n in words) +
                    b"".join(struct.pack("<I", n << 4 | op) for op, n in fin))
        want.append(f"{int(bam.cigar_changed(body, final))} {bam.oc_of(words)}")
    for cig, fin, _, _ in oc.TABLE:
        case(oc.runs_of(cig), fin)
    for s in sets.values():
        for r, fin in zip(s["records"], s["finals"]):
            case(r["cigar"], fin)
    cases = str(tmp_path / "cases.bin")
    with open(cases, "wb") as fh:
        fh.write(b"".join(blob))
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(want)
    for line, text in zip(lines, want):
        assert line == text
