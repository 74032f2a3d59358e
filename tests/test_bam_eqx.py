"""The =/X form of the FULL records' CIGARs (--records full --eqx, NPORE_CIGAR_EQX), host side: the rule of
npore_amd/csrc/eqx_rec.hpp through its Python statement bam.eqx_of and its host twin npore_bam_format_bam_full_pass -- CIGARs
pinned by hand, the identities with NM and cs, crafted reads (bam_eqx_cases, bam_cs_cases, bam_md_cases, bam_full_cases), random
reads, a pass mask, the CG threshold, the surface, two halves written as one indexed file, and the sequential twin under the
sanitizers.  No GPU here: the final CIGARs are given.
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
from test_bam_out import Hdr, check_index, split_records
import bam_cs_cases as cc
import bam_eqx_cases as ec
import bam_full_cases as fc
import bam_md_cases as mc
import bam_pass_cases as pc
import long_cigar_cases as lc
from full_record_driver import host_full

EOF, PART, DEFLATE, MATCH, FULL, MD = bam.OUT_EOF, bam.OUT_PART, bam.OUT_DEFLATE, bam.OUT_MATCH, bam.OUT_FULL, bam.OUT_MD      # npore_bam_set_output's flags
CS, CS_LONG, DE = bam.TAG_CS, bam.TAG_CS_LONG, bam.TAG_DE                  # npore_bam_set_output_tags' word
ALL_TAGS = dict(md=True, cs="long", de=True)
COMBOS = {"alone": dict(), "md": dict(md=True), "tags": ALL_TAGS}
EQX = bam.CIGAR_EQX


def open_pair(bp, fa):
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in zip(nb.references, nb.lengths)])
    return nb, nf, idx


# ---- 1. the table, pinned by hand, on raw code arrays ---------------------------------------------------------------------------
def test_table_of_the_rule():
    finals = [row[2] for row in ec.TABLE]
    for must in ("3=2X3M", "4M2N2M", "0M2M0I0D", "2D1I1D", ""):
        assert must in finals
    for ref, seq, fin, want in ec.TABLE:
        r, q = np.array(ref, np.uint8), np.array(seq, np.uint8)
        assert bam.eqx_of(r, q, fin) == want, fin
        ec.eqx_identities(want, fin, bam.nm_of(r, q, fin), bam.cs_of(r, q, fin))
    # the declared difference from minimap2, as in NM: an ambiguous base is X, on both sides
    assert bam.eqx_of(mc.codes("ACRT"), mc.codes("ACRT"), "4M") == "2=1X1="


# ---- the crafted reads of the four case files and the seam reads, through the host twin with and without the bit ------------------
@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_eqx")
    sets = {}
    for key, pack in (("eqx", ec.eqx_reads()), ("cs", cc.crafted_reads()), ("seam", cc.seam_reads()), ("md", mc.crafted_reads()),
                      ("full", fc.crafted_reads())):
        references, refs, records, finals = pack[:4]
        bp, fa = fc.write_inputs(tmp, references, refs, records, key)
        nb, nf, idx = open_pair(bp, fa)
        assert len(idx) == len(records)
        status = np.array([r["_status"] for r in records], np.int32)
        got = {name: nb.format_bam_full(nf, idx, finals, status, eqx=True, **kw) for name, kw in COMBOS.items()}
        plain = {name: nb.format_bam_full(nf, idx, finals, status, **kw) for name, kw in COMBOS.items()}
        nb.close(); nf.close()
        texts = []                                               # the Python statement, once per read: (=/X form, NM, cs short)
        for r, fin in zip(records, finals):
            rc, sc, _ = lc.expected_pack(r, r["cigar"], refs[r.get("_ctg", "ctg")])
            texts.append((bam.eqx_of(rc, sc, fin), bam.nm_of(rc, sc, fin), bam.cs_of(rc, sc, fin)))
        sets[key] = dict(bp=bp, fa=fa, refs=refs, records=records, finals=finals, pinned=pack[4] if key == "eqx" else {}, status=status, got=got,
                         plain=plain, texts=texts)
    return tmp, sets


# ---- 2. host twin == Python statement, byte for byte ----------------------------------------------------------------------------------
def test_host_twin_equals_statement(crafted):
    tmp, sets = crafted
    for key, s in sets.items():
        raws = fc.input_records(s["bp"])
        for name, kw in COMBOS.items():
            assert s["got"][name] == ec.want_stream(raws, s["records"], s["refs"], s["finals"], s["status"], **kw), (key, name)
            # a run without the bit writes today's bytes, which are the statement's without the option
            assert s["plain"][name] == ec.want_stream(raws, s["records"], s["refs"], s["finals"], s["status"], eqx=False, **kw), (key, name)
        assert s["got"]["alone"] != s["plain"]["alone"]


def test_random_reads(tmp_path):
    references, refs, records, finals, arrays = mc.random_reads(n_reads=300)
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "rnd")
    nb, nf, idx = open_pair(bp, fa)
    st = np.zeros(len(idx), np.int32)
    raws = fc.input_records(bp)
    for kw in (dict(), ALL_TAGS):
        got = split_records(nb.format_bam_full(nf, idx, finals, st, eqx=True, **kw))
        assert len(got) == 300
        for (_, rec), raw, fin, (rc, sc) in zip(got, raws, finals, arrays):
            assert rec == bam.full_record(raw, rc, sc, fin, eqx=True, **kw), fin
    for (_, rec), fin, (rc, sc) in zip(got, finals, arrays):
        text, n_cig = ec.record_cigar_text(rec)
        assert text == bam.eqx_of(rc, sc, fin) and n_cig == len(ec.runs_of(text))
        ec.eqx_identities(text, fin, bam.nm_of(rc, sc, fin), bam.cs_of(rc, sc, fin))
    nb.close(); nf.close()


@pytest.mark.parametrize("mask", [0x904, 0x100])
def test_with_a_pass_mask(tmp_path, mask):
    """a record that passes is written as it came; every other record is the statement's with the split words"""
    references, refs, records = pc.pass_file()
    bp, fa = str(tmp_path / "p.bam"), str(tmp_path / "p.fa")
    pc.write_bam(bp, references, records)
    lc.write_fasta(fa, refs)
    raws, flags, finals = fc.input_records(bp), [r["flag"] for r in records], pc.finals_of(records)
    status = np.array([32 if r["_kind"] == "refused" else 0 for r in records], np.int32)
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = np.array(pc.py_select(raws, [(0, 0, 1 << 28), (1, 0, 1 << 28)], 0, mask), np.int64)
    for kw in (dict(), ALL_TAGS):
        rest = []
        for k in idx:
            if not pc.passes(flags[k], mask) and not status[k]:
                rc, sc, _ = lc.expected_pack(records[k], records[k]["cigar"], refs[f"ctg{records[k]['ref_id']}"])
                rest.append(bam.full_record(raws[k], rc, sc, finals[k], eqx=True, **kw))
        want = b"".join(pc.compose(raws, flags, mask, idx.tolist(), {12}, rest))
        assert nb.format_bam_full(nf, idx, [finals[k] for k in idx], status[idx], pass_mask=mask, eqx=True, **kw) == want, kw
    assert any(b"=" in ec.record_cigar_text(r)[0].encode() for r in rest)
    nb.close(); nf.close()


# ---- 3. the identities on every crafted read; nothing but the CIGAR changes -----------------------------------------------------------
def no_cg(aux):
    return [t for t in mc.parse_tags(aux) if t[0] != b"CG"]


def test_identities_and_nothing_else_changes(crafted):
    tmp, sets = crafted
    seen = {}
    for key, s in sets.items():
        kept = [(r, fin, t) for r, fin, t in zip(s["records"], s["finals"], s["texts"]) if not r["_status"]]
        for name in COMBOS:
            with_bit, without = split_records(s["got"][name]), split_records(s["plain"][name])
            assert len(with_bit) == len(without) == len(kept)
            for (_, a), (_, b), (r, fin, (eqx, nm, cs)) in zip(with_bit, without, kept):
                fa_, name_a, _, body_a, aux_a = fc.parse_full(a)
                fb_, name_b, _, body_b, aux_b = fc.parse_full(b)
                ta, na = ec.record_cigar_text(a)
                tb, nb_ = ec.record_cigar_text(b)
                # the split words between the same clip words; collapsing gives the CIGAR of the run without the bit
                assert ec.without_outer_clips(ta) == eqx, r["name"]
                assert ec.canonical_m(ta) == ec.canonical_m(tb), r["name"]
                assert ec.split_clips(ta)[0::2] == ec.split_clips(tb)[0::2], r["name"]
                # every other byte: the fixed fields but n_cigar_op (bin, tlen included), the name, bases, qualities, every tag but CG
                assert fa_[:5] + fa_[6:] == fb_[:5] + fb_[6:] and name_a == name_b and body_a == body_b, r["name"]
                assert no_cg(aux_a) == no_cg(aux_b), r["name"]
                assert na == (2 if len(ec.runs_of(ta)) > 0xFFFF else len(ec.runs_of(ta)))
                ec.eqx_identities(eqx, fin, nm, cs)
                nm_rec = [int.from_bytes(v, "little") for t, _, v in mc.parse_tags(aux_a) if t == b"NM"]
                assert nm_rec == [nm], r["name"]
                seen[(key, r["name"])] = eqx
    for name, text in sets["eqx"]["pinned"].items():
        assert seen[("eqx", name)] == text, name
    # what the case files are for, in the statement's words: the seam read where nothing differs is ONE run through the tile's end
    k = [r["name"] for r in sets["seam"]["records"]].index("seam64X")
    assert seen[("seam", "seam64X")] == "2=1I" * 31 + "76=1D70="
    assert seen[("cs", "three_words")] == "2I139=1D3=" and seen[("cs", "mi300")] == "1=1I" * 150 and seen[("cs", "diff_all")] == "130X"
    assert seen[("md", "m100001")] == "100001=" and seen[("md", "past_end")] == "20=5D10X" and seen[("md", "no_words")] == ""
    # the CIGAR field at every byte alignment, and a refused read between two good ones
    names = [r["name"] for r in sets["eqx"]["records"] if not r["_status"]]
    assert names[names.index("refused_before") + 1] == "refused_after"
    assert {len(n) for n in names} >= {1, 2, 3, 4}


# ---- 4. the CG threshold --------------------------------------------------------------------------------------------------------------
def test_cg_threshold(crafted, tmp_path):
    references, refs, records, finals = ec.cg_reads()
    assert finals == ["65533M", "65534M"]                        # the M form is one word
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "cg")
    nb, nf, idx = open_pair(bp, fa)
    st = np.zeros(2, np.int32)
    raws = fc.input_records(bp)
    for kw in (dict(), ALL_TAGS):
        got = nb.format_bam_full(nf, idx, finals, st, eqx=True, **kw)
        assert got == ec.want_stream(raws, records, refs, finals, st, **kw)
        (_, plain), (_, long) = split_records(got)
        text, n_cig = ec.record_cigar_text(plain)                # 65 533 + 2 clip words: the most n_cigar_op holds
        assert n_cig == 65535 and text == "1S" + "1=1X" * 32766 + "1=" + "2S" and b"CGBI" not in plain
        text, n_cig = ec.record_cigar_text(long)                 # one more: placeholder + CG behind the other tags
        assert n_cig == 2 and text == "1S" + "1=1X" * 32767 + "2S"
        f, _, words, _, aux = fc.parse_full(long)
        assert words == [65537 << 4 | 4, 65534 << 4 | 3]
        tags = mc.parse_tags(aux)
        assert tags[-1][0] == b"CG" and tags[-1][2][:5] == b"I" + struct.pack("<I", 65536) and len(tags[-1][2]) == 5 + 4 * 65536
        assert [t for t, _, _ in tags][1:] == [b"NM"] + ([b"MD", b"cs", b"de"] if kw else []) + [b"CG"]
        # without the bit both are plain records of three words
        assert [ec.record_cigar_text(r) for _, r in split_records(nb.format_bam_full(nf, idx, finals, st, **kw))] == [("1S65533M2S", 3), ("1S65534M2S", 3)]
    nb.close(); nf.close()
    # the crafted `long` read: (1M1I) x 32 767 between three clip words is as long in either form
    tmp, sets = crafted
    s = sets["cs"]
    names = [r["name"] for r in s["records"] if not r["_status"]]
    rec = split_records(s["got"]["tags"])[names.index("long")][1]
    text, n_cig = ec.record_cigar_text(rec)
    assert n_cig == 2 and text == "1H2S" + "1=1I" * 32767 + "1S"
    assert [t for t, _, _ in mc.parse_tags(fc.parse_full(rec)[4])][-5:] == [b"NM", b"MD", b"cs", b"de", b"CG"]


# ---- 5. the surface -------------------------------------------------------------------------------------------------------------------
def test_surface(crafted):
    tmp, sets = crafted
    s = sets["eqx"]
    nb, nf, idx = open_pair(s["bp"], s["fa"])
    lib = nb._lib
    hdr = open(os.path.join(REPO, "include", "npore_amd.h")).read()
    # (the bit is 32, not the word's next one: test_bam_cs.py and test_bam_pass.py pin 8, 9, 16 and 64 as refused behind FULL, and
    # they stay as they are -- so "bit 8 alone is accepted" cannot hold beside them; every case below is asked of the bit that is)
    assert re.search(r"#define NPORE_CIGAR_EQX 32\b", hdr) and re.search(r"#define NPORE_ABI_VERSION 2\b", hdr) and lib.npore_abi_version() == 2
    doc = hdr[hdr.index("#define NPORE_TAG_DE 4"):hdr.index("#define NPORE_CIGAR_EQX 32")]
    assert "not a tag" in doc and "--eqx" in doc and "NPORE_OUT_FULL" in doc
    declared = set(re.findall(r"\b(npore_[a-z_0-9]+)\s*\(", hdr)) - {"npore_ctx"}
    assert declared == set(_lib.SIGNATURES)                      # no entry point was added for it
    # the bit alone, and beside every valid tag word, behind BAM + FULL; not without FULL, not in SAM format; no undefined bit
    assert lib.npore_bam_set_output_tags(nb.handle, EQX) != 0      # (a fresh handle writes SAM)
    for fmt, flags in ((0, 0), (1, EOF), (1, DEFLATE | EOF), (1, PART)):
        assert lib.npore_bam_set_output(nb.handle, fmt, None, flags) == 0
        for tags in (EQX, EQX | CS, EQX | CS | CS_LONG | DE):
            assert lib.npore_bam_set_output_tags(nb.handle, tags) != 0, (fmt, flags, tags)
    assert lib.npore_bam_set_output(nb.handle, 0, None, FULL | EOF) != 0                  # (FULL in SAM format is refused outright)
    for full in (FULL | EOF, FULL | PART, FULL | MD | EOF, FULL | DEFLATE | EOF):
        assert lib.npore_bam_set_output(nb.handle, 1, None, full) == 0
        for tags in (EQX, EQX | CS, EQX | CS | CS_LONG, EQX | DE, EQX | CS | CS_LONG | DE):
            assert lib.npore_bam_set_output_tags(nb.handle, tags) == 0, tags
        for tags in (EQX | CS_LONG, EQX | CS_LONG | DE, 8, EQX | 8, 16, EQX | 16, 64, EQX | 64, 128, 1 << 30, -1):
            assert lib.npore_bam_set_output_tags(nb.handle, tags) != 0, tags
    # set_output sets it back: the packed sizes cannot show it, the host entry can -- a handle set to EQX and then set again
    # refuses the tags of a SAM run, and npore_bam_set_output_pass behind the bit keeps it (the pass setter rebuilds the spec)
    assert lib.npore_bam_set_output(nb.handle, 1, None, FULL | EOF) == 0 and lib.npore_bam_set_output_tags(nb.handle, EQX) == 0
    assert lib.npore_bam_set_output_pass(nb.handle, 0x904) == 0
    assert lib.npore_bam_set_output(nb.handle, 0, None, 0) == 0
    assert lib.npore_bam_set_output_tags(nb.handle, EQX) != 0 and lib.npore_bam_set_output_tags(nb.handle, 0) != 0
    # npore_bam_write_file keeps refusing FULL, with the bit as without
    assert lib.npore_bam_set_output(nb.handle, 1, None, FULL | EOF) == 0 and lib.npore_bam_set_output_tags(nb.handle, EQX) == 0
    out = tmp / "never.bam"
    assert lib.npore_bam_write_file(nb.handle, None, 0, 1, None, None, None, None, 0, str(out).encode()) != 0
    assert b"FULL records" in lib.npore_last_error() and not out.exists()
    # the host entries: the bit is accepted by _tags and _pass, refused with an undefined bit or with FULL / a writer's bit in `flags`
    host = lambda entry, **words: host_full(nb, nf, idx, s["finals"], s["status"], entry=entry, **words)
    assert host("_tags", tags=EQX) == (0, s["got"]["alone"])
    assert host("_pass", flags=MD, tags=EQX | CS | CS_LONG | DE) == (0, s["got"]["tags"])
    assert host("_tags") == (0, s["plain"]["alone"])
    for flags, tags in ((0, 16), (0, EQX | 16), (0, EQX | CS_LONG), (0, EQX | 8), (FULL, EQX), (EOF, EQX), (64, EQX)):
        assert host("_tags", flags=flags, tags=tags)[0] != 0, (flags, tags)
    # Python: the option needs records "full"
    assert bam.output_tags(None, False, eqx=True) == EQX and bam.output_tags("long", True, True) == EQX | CS | CS_LONG | DE and bam.output_tags("short", False) == CS
    for kw in (dict(out_format="bam", eqx=True), dict(out_format="sam", eqx=True), dict(out_format="bam", records="reference", eqx=True)):
        with pytest.raises(ValueError):
            nb.set_output(**kw)
    nb.set_output("bam", records="full", eqx=True)
    nb.set_output("bam", records="full", md=True, cs="long", de=True, pass_mask=0x904, eqx=True)
    nb.set_output("sam")
    nb.close(); nf.close()


def test_cli_eqx_needs_full_records(tmp_path):
    data = os.path.join(GOLDEN, "data")
    common = [sys.executable, "-m", "npore_amd.realign", "--bam", os.path.join(data, "reads.bam"), "--ref", os.path.join(data, "ref.fasta"),
              "--out_prefix", str(tmp_path / "bad"), "--eqx"]
    for extra in ([], ["--out_format", "bam"], ["--out_format", "bam", "--records", "reference"], ["--out_format", "sam"]):
        out = subprocess.run(common + extra, cwd=REPO, capture_output=True, text=True, timeout=120)
        assert out.returncode == 1, out.stdout[-2000:] + out.stderr[-2000:]
        errors = [l for l in out.stdout.splitlines() if l.startswith("ERROR")]
        assert len(errors) == 1 and "--eqx" in errors[0] and "--records full" in errors[0], out.stdout
        assert not os.path.exists(str(tmp_path / "bad.bam")) and not os.path.exists(str(tmp_path / "bad.sam"))
    text = subprocess.run([sys.executable, "-m", "npore_amd.realign", "--help"], cwd=REPO, capture_output=True, text=True, timeout=120).stdout
    assert "--eqx" in text and "minimap2 --eqx" in " ".join(text.split())


# ---- two parts: the record bytes of two halves are those of one run, and go into one indexed file as they come --------------------
def test_two_parts_one_file(crafted, tmp_path):
    tmp, sets = crafted
    s = sets["eqx"]
    nb, nf, idx = open_pair(s["bp"], s["fa"])
    half = len(idx) // 2
    parts = [nb.format_bam_full(nf, idx[lo:hi], s["finals"][lo:hi], s["status"][lo:hi], eqx=True, **ALL_TAGS) for lo, hi in ((0, half), (half, len(idx)))]
    whole = s["got"]["tags"]
    assert b"".join(parts) == whole
    out = str(tmp_path / "two.bam")
    bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
    nb.close(); nf.close()
    w = bam.BamRecordWriter(out, bai=out + ".bai")
    for part in parts:                                           # (a part's records, appended as they come)
        w.add([rec for _, rec in split_records(part)])
    assert w.close() and w.n_records == len(split_records(whole))
    assert bam._bgzf_decompress(out).endswith(whole)
    check_index(out, out + ".bai")                               # the walk finds every read: reference lengths, bins did not change


# ---- 6. the sequential twin under the sanitizers --------------------------------------------------------------------------------------
def test_sequential_twin_under_sanitizers(tmp_path, crafted):
    tmp, sets = crafted
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = os.path.join(REPO, "tests", "model", "bam_eqx_sanitize.cpp")
    exe = str(tmp_path / "bam_eqx_sanitize")
    # (the runtimes linked statically: the program needs nothing preloaded and does not mind what is)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + san + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is missing")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + san + ["-o", exe, src])
    blob, want = [], []

    def case(words, rc, sc, text):
        blob.append(struct.pack("<qqq", len(words), len(rc), len(sc)) + struct.pack(f"<{len(words)}I", *words) + bytes(rc) + bytes(sc))
        want.append(text)
    for ref, seq, fin, text in ec.TABLE:                         # (codes 0 and 5, N S H P words, words of length 0, the empty CIGAR)
        case(cc.words_of(fin), ref, seq, text)
    for s in sets.values():
        for r, fin, t in zip(s["records"], s["finals"], s["texts"]):
            if r["_status"]:
                continue
            rc, sc, _ = lc.expected_pack(r, r["cigar"], s["refs"][r.get("_ctg", "ctg")])
            case(cc.words_of(fin), rc.tobytes(), sc.tobytes(), t[0])
    cases = str(tmp_path / "cases.bin")
    with open(cases, "wb") as fh:
        fh.write(b"".join(blob))
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(want)
    for line, text in zip(lines, want):
        assert line == text
