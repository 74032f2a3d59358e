"""The cs and de tags of the FULL records (--records full --cs short|long --de, NPORE_TAG_*), host side: the rule of
npore_amd/csrc/cs_rec.hpp through its Python statement bam.cs_of / bam.de_of and its host twin npore_bam_format_bam_full_tags --
texts pinned by hand, the identities with NM and MD, crafted reads (bam_cs_cases and bam_md_cases), random reads, today's bytes
with exactly the new tags spliced in, the surface, two halves written as one indexed file, and the sequential twin under the
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
import bam_full_cases as fc
import bam_md_cases as mc
import long_cigar_cases as lc
from full_record_driver import host_full

EOF, PART, DEFLATE, MATCH, FULL, MD = bam.OUT_EOF, bam.OUT_PART, bam.OUT_DEFLATE, bam.OUT_MATCH, bam.OUT_FULL, bam.OUT_MD      # npore_bam_set_output's flags
CS, CS_LONG, DE = bam.TAG_CS, bam.TAG_CS_LONG, bam.TAG_DE                  # npore_bam_set_output_tags' word
COMBOS = [(md, cs, de) for md in (False, True) for cs in cc.FORMS for de in (False, True)]


def open_pair(bp, fa):
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in zip(nb.references, nb.lengths)])
    return nb, nf, idx


# ---- 1. a dozen and more texts pinned by hand, on raw code arrays ----------------------------------------------------------------
def test_table_of_the_rule():
    assert len(cc.TABLE) >= 12
    for ref, seq, fin, short, long, (e, x, g) in cc.TABLE:
        r, q = np.array(ref, np.uint8), np.array(seq, np.uint8)
        assert bam.cs_of(r, q, fin) == short, fin
        assert bam.cs_of(r, q, fin, long=True) == long, fin
        de = bam.de_of(r, q, fin)
        assert de.dtype == np.float32 and de == cc.table_de(e, x, g), fin
        if "N" not in fin:
            cc.cs_identities(short, long, bam.nm_of(r, q, fin), fin, bam.md_of(r, q, fin))
    # de in numbers: one substitution and one gap open over 7 + 1 + 1; nothing compared and no gap: 0
    assert bam.de_of(mc.codes("ACGTACGTAC"), mc.codes("ACGTCTAC"), "4M2D4M") == np.float32(2 / 9)
    assert bam.de_of(mc.codes(""), mc.codes("ACGT"), "4S") == 0.0
    # the declared difference from minimap2: an ambiguous base is a mismatch here, on both sides
    assert bam.cs_of(mc.codes("ACRT"), mc.codes("ACRT"), "4M") == ":2*nn:1" and bam.nm_of(mc.codes("ACRT"), mc.codes("ACRT"), "4M") == 1


# ---- the crafted reads of both case files, through the host twin once in every combination --------------------------------------
@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_cs")
    sets = {}
    for key, (references, refs, records, finals, pinned) in (("cs", cc.crafted_reads()), ("md", mc.crafted_reads())):
        bp, fa = fc.write_inputs(tmp, references, refs, records, key)
        nb, nf, idx = open_pair(bp, fa)
        assert len(idx) == len(records)
        status = np.array([r["_status"] for r in records], np.int32)
        got = {(md, cs, de): nb.format_bam_full(nf, idx, finals, status, md=md, cs=cs, de=de) for md, cs, de in COMBOS}
        nb.close(); nf.close()
        texts = []                                               # the Python statement, once per read: (cs short, cs long, de, NM, MD)
        for r, fin in zip(records, finals):
            rc, sc, _ = lc.expected_pack(r, r["cigar"], refs[r["_ctg"]])
            texts.append((bam.cs_of(rc, sc, fin), bam.cs_of(rc, sc, fin, long=True), bam.de_of(rc, sc, fin), bam.nm_of(rc, sc, fin),
                          bam.md_of(rc, sc, fin)))
        sets[key] = dict(bp=bp, fa=fa, refs=refs, records=records, finals=finals, pinned=pinned, status=status, got=got, texts=texts)
    return tmp, sets


def new_tag_bytes(text, cs, de):
    short, long, dev = text[:3]
    return (b"csZ" + (long if cs == "long" else short).encode() + b"\0" if cs else b"") + (b"def" + struct.pack("<f", dev) if de else b"")


# ---- 2. host twin == Python statement, today's bytes, the splice ------------------------------------------------------------------
def test_host_twin_equals_statement(crafted):
    tmp, sets = crafted
    for key, s in sets.items():
        raws = fc.input_records(s["bp"])
        kept_texts = [t for t, r in zip(s["texts"], s["records"]) if not r["_status"]]
        # without the options: today's bytes, which are the Python statement's (bam.full_record(md=))
        for md in (False, True):
            assert s["got"][(md, None, False)] == mc.want_stream(raws, s["records"], s["refs"], s["finals"], s["status"], md=md), (key, md)
        # with them: those bytes with exactly the new tags spliced in before CG, the tags the Python statement's
        for md, cs, de in COMBOS:
            plain = split_records(s["got"][(md, None, False)])
            assert len(plain) == len(kept_texts)
            want = b"".join(cc.splice(rec, new_tag_bytes(t, cs, de)) for (_, rec), t in zip(plain, kept_texts))
            assert s["got"][(md, cs, de)] == want, (key, md, cs, de)
        # bam.full_record itself with the options, byte for byte
        for md, cs, de in ((True, "short", True), (False, "long", False), (False, None, True)):
            assert s["got"][(md, cs, de)] == cc.want_stream(raws, s["records"], s["refs"], s["finals"], s["status"], md=md, cs=cs, de=de), (key, md, cs, de)


def test_seam_reads_host_twin_equals_statement(tmp_path):
    """the reads at the seams of the device walk's frame (cc.seam_reads): the host twin, which the device is held to, against
    bam.full_record in every combination"""
    references, refs, records, finals = cc.seam_reads()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "seam")
    nb, nf, idx = open_pair(bp, fa)
    assert len(idx) == len(records) == 13
    raws, status = fc.input_records(bp), np.zeros(len(records), np.int32)
    for md, cs, de in COMBOS:
        assert nb.format_bam_full(nf, idx, finals, status, md=md, cs=cs, de=de) == cc.want_stream(raws, records, refs, finals, status, md=md, cs=cs, de=de), (md, cs, de)
    # what the seams are for, pinned by hand on the read where nothing differs: (2M1I) x 31, then ONE stretch from the = word
    # through the M at the tile's end into the next tile's X and M, the deleted base, the closing = word
    k = [r["name"] for r in records].index("seam64X")
    assert finals[k] == "2M1I" * 31 + "3=64M5X4M1D70="
    last_ins = 3 * 30 + 2                                        # the read's 31st inserted base
    stretch = 3 + 64 + 5 + 4
    deleted = records[k]["pos"] + 2 * 31 + stretch               # the reference base under D
    text = cc.new_tags_of(split_records(nb.format_bam_full(nf, idx, finals, status, cs="short"))[k][1])[0]
    assert text.endswith(f"+{records[k]['seq'][last_ins].lower()}:{stretch}-{refs['ctg'][deleted].lower()}:70"), text
    nb.close(); nf.close()


# ---- 3. the texts pinned by hand, the order of the tags, the alignments -----------------------------------------------------------
def test_crafted_reads(crafted):
    tmp, sets = crafted
    s = sets["cs"]
    kept = [(r, t) for r, t in zip(s["records"], s["texts"]) if not r["_status"]]
    names = [r["name"] for r, _ in kept]
    at = names.index("refused_before")
    assert names[at + 1] == "refused_after" and "refused" not in names          # the refused read lay between two good ones
    out = split_records(s["got"][(True, "short", True)])
    assert len(out) == len(kept)
    seen, where, lengths = {}, set(), set()
    for (off, rec), (r, t) in zip(out, kept):
        text, de, tags = cc.new_tags_of(rec)
        seen[r["name"]] = (text, de)
        assert text == t[0] and struct.pack("<f", de) == struct.pack("<f", t[2]), r["name"]
        tail = [x for x in tags if x in (b"NM", b"MD", b"cs", b"de", b"CG")]
        assert tail == [b"NM", b"MD", b"cs", b"de"] + ([b"CG"] if r["name"] == "long" else []) and tags[-len(tail):] == tail, (r["name"], tags)
        where.add((off + cc.tag_offset(rec, b"cs")) % 4)
        lengths.add(len(text))
    for name, (text, exg) in s["pinned"].items():
        assert seen[name][0] == text, name
        assert struct.pack("<f", seen[name][1]) == struct.pack("<f", cc.table_de(*exg)), name
    assert where == {0, 1, 2, 3} and {0, 2, 3, 4, 63, 64, 65} <= lengths      # (no cs text has one byte)
    assert len(seen["diff_all"][0]) == 3 * 130 and seen["diff_all"][1] == 1.0  # three bytes per base: the bound's worst case
    assert re.fullmatch(r"(\*[acgt]{2}:9)(\*[acgt]{2}:10)(\*[acgt]{2}:99)(\*[acgt]{2}:100)(\*[acgt]{2}:999)(\*[acgt]{2}:1000)(\*[acgt]{2}:9999)"
                        r"(\*[acgt]{2}:10000)\*[acgt]{2}", seen["counts"][0])
    # the long read: placeholder CIGAR, and CG behind cs and de with all the words
    rec = out[names.index("long")][1]
    f, _, words, _, aux = fc.parse_full(rec)
    cg = mc.parse_tags(aux)[-1]
    assert f[5] == 2 and cg[0] == b"CG" and cg[2][:5] == b"I" + struct.pack("<I", 65537) and len(cg[2]) == 5 + 4 * 65537
    # the stale cs and de are replaced, RG and the B array are kept in order
    rec = out[names.index("stale")][1]
    tags = mc.parse_tags(fc.parse_full(rec)[4])
    assert [t for t, _, _ in tags] == [b"RG", b"ML", b"NM", b"MD", b"cs", b"de"]
    assert tags[1][1:] == (b"B", b"C" + struct.pack("<i", 5) + bytes(range(5))) and tags[4][2] == s["pinned"]["stale"][0].encode() + b"\0"
    # bam_md_cases' reads: the one stretch of 100 001, N in the reference, the final past the arrays
    m = sets["md"]
    by_name = {r["name"]: t for r, t in zip(m["records"], m["texts"])}
    assert by_name["m100001"][0] == ":100001" and by_name["m100001"][1] == "=" + m["refs"]["big"][50:100051]
    assert by_name["all_i"][0].startswith("+") and len(by_name["all_i"][0]) == 41 and by_name["all_d"][0] == "-" + m["refs"]["ctg"][7100:7140].lower()
    assert by_name["past_end"][0] == ":20-nnnnn" + "*nn" * 10 and by_name["no_words"][0] == ""


# ---- 4. the identities, on the crafted and on 2 000 random reads ------------------------------------------------------------------
def test_identities_crafted(crafted):
    tmp, sets = crafted
    for key, s in sets.items():
        for r, fin, (short, long, de, nm, md) in zip(s["records"], s["finals"], s["texts"]):
            cc.cs_identities(short, long, nm, fin, md)
            assert 0.0 <= de <= 1.0


def test_random_reads(tmp_path):
    references, refs, records, finals, arrays = mc.random_reads()
    assert len(records) == 2000
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "rnd")
    nb, nf, idx = open_pair(bp, fa)
    st = np.zeros(len(idx), np.int32)
    short = split_records(nb.format_bam_full(nf, idx, finals, st, md=True, cs="short", de=True))
    long = split_records(nb.format_bam_full(nf, idx, finals, st, cs="long"))
    nb.close(); nf.close()
    assert len(short) == len(long) == 2000
    for (_, rs), (_, rl), r, fin, (rc, sc) in zip(short, long, records, finals, arrays):
        ts, de, _ = cc.new_tags_of(rs)
        tl, none, names = cc.new_tags_of(rl)
        assert none is None and names[-2:] == [b"NM", b"cs"]
        assert ts == bam.cs_of(rc, sc, fin) and tl == bam.cs_of(rc, sc, fin, long=True), r["name"]
        assert struct.pack("<f", de) == struct.pack("<f", bam.de_of(rc, sc, fin)), r["name"]
        md, nm, _, _ = mc.md_and_nm(rs)
        cc.cs_identities(ts, tl, nm, fin, md)


# ---- 5. the surface ---------------------------------------------------------------------------------------------------------------
def test_surface(crafted, tmp_path):
    tmp, sets = crafted
    s = sets["cs"]
    nb, nf, idx = open_pair(s["bp"], s["fa"])
    lib = nb._lib
    full = FULL | EOF
    # tags only behind a BAM + FULL set_output; bad bits and LONG without CS refused; set_output clears them
    assert lib.npore_bam_set_output_tags(nb.handle, CS) != 0                          # (a fresh handle writes SAM)
    for fmt, flags in ((0, 0), (1, EOF), (1, DEFLATE | EOF), (1, PART)):
        assert lib.npore_bam_set_output(nb.handle, fmt, None, flags) == 0
        for tags in (CS, CS | CS_LONG, DE, CS | DE, CS | CS_LONG | DE):
            assert lib.npore_bam_set_output_tags(nb.handle, tags) != 0, (fmt, flags, tags)
    assert lib.npore_bam_set_output(nb.handle, 1, None, full) == 0
    for tags in (CS_LONG, CS_LONG | DE, 8, 8 | CS, 16, 64, -1):
        assert lib.npore_bam_set_output_tags(nb.handle, tags) != 0, tags
    for tags in (0, CS, CS | CS_LONG, DE, CS | DE, CS | CS_LONG | DE):
        assert lib.npore_bam_set_output_tags(nb.handle, tags) == 0, tags
    assert lib.npore_bam_set_output(nb.handle, 0, None, 0) == 0                      # ... back to SAM: the tags are gone with it
    assert lib.npore_bam_set_output_tags(nb.handle, CS) != 0
    # flag bit 64 is still refused by both old entry points; the ABI version is 2
    assert lib.npore_bam_set_output(nb.handle, 1, None, 64 | FULL | EOF) != 0
    host = lambda entry, **words: host_full(nb, nf, idx, s["finals"], s["status"], entry=entry, **words)
    assert host("_md", flags=64)[0] != 0
    assert lib.npore_abi_version() == 2
    # the new host entry point: tags = 0 is the _md entry point; bad flags and bad tags refused
    for flags, md in ((0, False), (MD, True)):
        assert host("_tags", flags=flags, tags=0) == (0, s["got"][(md, None, False)])
    assert host("_tags", flags=MD, tags=CS | DE) == (0, s["got"][(True, "short", True)])
    for flags, tags in ((64, CS), (FULL, CS), (0, CS_LONG), (0, 8), (MD, CS_LONG | DE), (0, -1)):
        assert host("_tags", flags=flags, tags=tags)[0] != 0, (flags, tags)
    # Python: the options need records "full"; a bad form is refused
    for kw in (dict(out_format="bam", cs="short"), dict(out_format="bam", de=True), dict(out_format="sam", cs="long"),
               dict(out_format="bam", records="full", cs="both")):
        with pytest.raises(ValueError):
            nb.set_output(**kw)
    nb.set_output("bam", records="full", md=True, cs="long", de=True)
    nb.set_output("sam")
    nb.close(); nf.close()
    # the header: the constants, the entry points, all bound
    hdr = open(os.path.join(REPO, "include", "npore_amd.h")).read()
    for name, v in (("NPORE_TAG_CS", 1), ("NPORE_TAG_CS_LONG", 2), ("NPORE_TAG_DE", 4), ("NPORE_ABI_VERSION", 2), ("NPORE_OUT_MD", 32)):
        assert re.search(rf"#define {name} {v}\b", hdr), name
    assert not re.search(r"#define NPORE_OUT_\w+ 64\b", hdr)
    assert hdr.index("#define NPORE_OUT_MD 32") < hdr.index("#define NPORE_TAG_CS 1")
    doc = hdr[hdr.index("#define NPORE_OUT_MD 32"):hdr.index("#define NPORE_TAG_CS 1")]
    assert "minimap2" in doc and "IUPAC" in doc and "--cs" in doc and "--de" in doc and "NPORE_OUT_FULL" in doc
    declared = set(re.findall(r"\b(npore_[a-z_0-9]+)\s*\(", hdr)) - {"npore_ctx"}
    new = {"npore_bam_set_output_tags", "npore_bam_format_bam_full_tags", "npore_debug_format_bam_full_tags_device"}
    assert declared == set(_lib.SIGNATURES) and new <= declared
    assert len(_lib.SIGNATURES["npore_bam_format_bam_full_tags"][1]) == len(_lib.SIGNATURES["npore_bam_format_bam_full_md"][1]) + 1
    assert len(_lib.SIGNATURES["npore_debug_format_bam_full_tags_device"][1]) == len(_lib.SIGNATURES["npore_debug_format_bam_full_md_device"][1]) + 1


def test_cli_cs_de_need_full_records(tmp_path):
    data = os.path.join(GOLDEN, "data")
    common = [sys.executable, "-m", "npore_amd.realign", "--bam", os.path.join(data, "reads.bam"), "--ref", os.path.join(data, "ref.fasta"),
              "--out_prefix", str(tmp_path / "bad")]
    for opt, extra in ((["--cs", "short"], []), (["--cs", "long"], ["--out_format", "bam"]),
                       (["--cs", "short"], ["--out_format", "bam", "--records", "reference"]), (["--de"], ["--out_format", "bam"])):
        out = subprocess.run(common + opt + extra, cwd=REPO, capture_output=True, text=True, timeout=120)
        assert out.returncode == 1, out.stdout[-2000:] + out.stderr[-2000:]
        errors = [l for l in out.stdout.splitlines() if l.startswith("ERROR")]
        assert len(errors) == 1 and opt[0] in errors[0] and "--records full" in errors[0], out.stdout
        assert not os.path.exists(str(tmp_path / "bad.bam")) and not os.path.exists(str(tmp_path / "bad.sam"))
    out = subprocess.run(common + ["--cs", "both", "--out_format", "bam", "--records", "full"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--cs" in out.stderr                               # (argparse's own refusal)


# ---- 6. two parts: the record bytes of two halves are those of one run, and go into one indexed file as they come ---------------
def test_two_parts_one_file(crafted, tmp_path):
    tmp, sets = crafted
    s = sets["cs"]
    nb, nf, idx = open_pair(s["bp"], s["fa"])
    half = len(idx) // 2
    parts = []
    for lo, hi in ((0, half), (half, len(idx))):
        parts.append(nb.format_bam_full(nf, idx[lo:hi], s["finals"][lo:hi], s["status"][lo:hi], md=True, cs="short", de=True))
    whole = s["got"][(True, "short", True)]
    assert b"".join(parts) == whole
    out = str(tmp_path / "two.bam")
    bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
    nb.close(); nf.close()
    w = bam.BamRecordWriter(out, bai=out + ".bai")
    for part in parts:                                                                # (a part's records, appended as they come)
        w.add([rec for _, rec in split_records(part)])
    assert w.close() and w.n_records == len(split_records(whole))
    data = bam._bgzf_decompress(out)
    assert data.endswith(whole)
    check_index(out, out + ".bai")                                                    # the walk finds every read


# ---- 7. the sequential twin under the sanitizers ----------------------------------------------------------------------------------
def test_sequential_twin_under_sanitizers(tmp_path, crafted):
    tmp, sets = crafted
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = os.path.join(REPO, "tests", "model", "bam_cs_sanitize.cpp")
    exe = str(tmp_path / "bam_cs_sanitize")
    # (the runtimes linked statically: the program needs nothing preloaded and does not mind what is)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + san + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is missing")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + san + ["-o", exe, src])
    blob, want = [], []

    def case(words, rc, sc, short, long, de):
        blob.append(struct.pack("<qqq", len(words), len(rc), len(sc)) + struct.pack(f"<{len(words)}I", *words) + bytes(rc) + bytes(sc))
        want.append((short, long, struct.unpack("<I", struct.pack("<f", de))[0]))
    for ref, seq, fin, short, long, exg in cc.TABLE:                                  # (codes 0 and 5, N words, words of length 0)
        case(cc.words_of(fin), ref, seq, short, long, cc.table_de(*exg))
    for s in sets.values():
        for r, fin, t in zip(s["records"], s["finals"], s["texts"]):
            if r["_status"]:
                continue
            rc, sc, _ = lc.expected_pack(r, r["cigar"], s["refs"][r["_ctg"]])
            case(cc.words_of(fin), rc.tobytes(), sc.tobytes(), t[0], t[1], t[2])
    cases = str(tmp_path / "cases.bin")
    with open(cases, "wb") as fh:
        fh.write(b"".join(blob))
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(want)
    for line, (short, long, bits) in zip(lines, want):
        got = line.split("\t")
        assert got[0] == short and got[1] == long and int(got[5]) == bits, short[:60]
