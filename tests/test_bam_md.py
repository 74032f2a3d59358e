"""The MD tag of the FULL records (--records full --md, NPORE_OUT_MD), host side: the rule of npore_amd/csrc/md_rec.hpp through
its Python statement bam.md_of and its host twin npore_bam_format_bam_full_md -- the rule's table, an independent brute-force
statement and an MD reader, crafted reads, random reads, the surface, and the sequential twin under the sanitizers.  No GPU
here: the final CIGARs are given.
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
import bam_md_cases as mc
import long_cigar_cases as lc
from full_record_driver import host_full

EOF, PART, DEFLATE, MATCH, FULL, MD = bam.OUT_EOF, bam.OUT_PART, bam.OUT_DEFLATE, bam.OUT_MATCH, bam.OUT_FULL, bam.OUT_MD      # npore_bam_set_output's flags

def open_pair(bp, fa):
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in zip(nb.references, nb.lengths)])
    return nb, nf, idx


def kept(records):
    return [r for r in records if not r["_status"]]


# ---- 1. the table ----------------------------------------------------------------------------------------------------------
def test_table_of_the_rule(tmp_path):
    for ref, seq, fin, md in mc.TABLE:
        assert bam.md_of(mc.codes(ref), mc.codes(seq), fin) == md, (ref, seq, fin)
    references, refs, records, finals, mds = mc.table_reads()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "table")
    nb, nf, idx = open_pair(bp, fa)
    assert len(idx) == len(records)
    got = split_records(nb.format_bam_full(nf, idx, finals, np.zeros(len(idx), np.int32), md=True))
    assert len(got) == len(records)
    for (_, rec), r, fin, md in zip(got, records, finals, mds):
        text, nm, _, names = mc.md_and_nm(rec)
        assert text == md, r["name"]
        assert names == ([b"RG"] if r["tags"] else []) + [b"NM", b"MD"], r["name"]       # the stale MD is gone, the new one follows NM
        assert nm == sum(c.isalpha() for c in md) + sum(int(n) for n in re.findall(r"(\d+)I", fin)), r["name"]
    nb.close(); nf.close()


# ---- the crafted reads, through the host twin once -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_md")
    references, refs, records, finals, pinned = mc.crafted_reads()
    bp, fa = fc.write_inputs(tmp, references, refs, records, "md")
    nb, nf, idx = open_pair(bp, fa)
    assert len(idx) == len(records)
    status = np.array([r["_status"] for r in records], np.int32)
    got = nb.format_bam_full(nf, idx, finals, status, md=True)
    plain = nb.format_bam_full(nf, idx, finals, status)
    nb.close(); nf.close()
    return tmp, bp, fa, refs, records, finals, pinned, status, got, plain


# ---- 2. an independent statement -------------------------------------------------------------------------------------------
def test_brute_force_and_reader(crafted):
    tmp, bp, fa, refs, records, finals, pinned, status, got, plain = crafted
    out = iter(split_records(got))
    seen = {}
    for r, fin in zip(records, finals):
        if r["_status"]:
            continue
        _, rec = next(out)
        text, nm, _, _ = mc.md_and_nm(rec)
        ref, seq = mc.letters_of(r, refs, fin)
        want, subs, dels, ins = mc.brute_md(ref, seq, fin)
        rc, sc, _ = lc.expected_pack(r, r["cigar"], refs[r["_ctg"]])
        assert bam.md_of(rc, sc, fin) == want == text, r["name"]
        assert subs + dels + ins == nm == bam.nm_of(rc, sc, fin), r["name"]              # the invariant with NM
        assert sum(c.isalpha() for c in re.sub(r"\^[A-Z]+", "", text)) == subs and sum(len(d) - 1 for d in re.findall(r"\^[A-Z]+", text)) == dels
        seen[r["name"]] = text
        # what pysam's get_reference_sequence() would rebuild is the contig under the FINAL alignment (N where the final names
        # more reference than the record has: past_end; nothing where it has no words: no_words)
        rl_fin = sum(int(n) for n, op in re.findall(r"(\d+)([MD])", fin))
        assert mc.rebuild_reference(text, seq, fin) == (ref + "N" * rl_fin)[:rl_fin], r["name"]
    assert next(out, None) is None
    # the documented difference from calmd is in the letters that are not ACGT: R in the read is a mismatch that prints the
    # reference's letter (calmd agrees); N in the reference is a mismatch that prints N -- and so would any IUPAC letter there
    assert re.fullmatch(r"7[ACGT]12", seen["r_in_read"]) and seen["n_in_ref"].startswith("3N1^") and "NN" in seen["n_in_ref"]
    assert bam.md_of(mc.codes("ACRT"), mc.codes("ACRT"), "4M") == "2N1" and bam.nm_of(mc.codes("ACRT"), mc.codes("ACRT"), "4M") == 1


# ---- 3. crafted reads ----------------------------------------------------------------------------------------------------------
def test_crafted_reads(crafted):
    tmp, bp, fa, refs, records, finals, pinned, status, got, plain = crafted
    raws = fc.input_records(bp)
    assert got == mc.want_stream(raws, records, refs, finals, status)                   # bam.full_record(md=True), byte for byte
    assert plain == mc.want_stream(raws, records, refs, finals, status, md=False)
    # flags = 0: the new entry point is the old one
    nb, nf, idx = open_pair(bp, fa)
    assert host_full(nb, nf, idx, finals, status, entry="_md", flags=0) == (0, plain)
    for flags in (EOF, FULL, MD | EOF, 64):      # NPORE_OUT_MD is the only bit it knows
        assert host_full(nb, nf, idx, finals, status, entry="_md", flags=flags)[0] != 0, flags
    nb.close(); nf.close()
    # the texts pinned by hand, the tag's place and the order of the tags
    out = split_records(got)
    assert len(out) == len(kept(records))
    at, seen, where, lengths = 0, {}, set(), set()
    for (_, rec), r in zip(out, kept(records)):
        text, nm, tag_at, names = mc.md_and_nm(rec)
        seen[r["name"]] = text
        assert names[-2:] == [b"NM", b"MD"] and rec.endswith(b"MDZ" + text.encode() + b"\0"), r["name"]
        if r["name"] in ("a", "al", "aln", "alnx"):
            where.add(tag_at % 4)                                # (within its record; the records follow each other without gaps)
            lengths.add(len(text))
        at += len(rec)
    assert "refused" not in seen and set(pinned) <= set(seen)
    for name, text in pinned.items():
        assert seen[name] == text, name
    assert where == {0, 1, 2, 3} and lengths == {1, 2, 3, 4}     # the tag at every byte alignment
    assert seen["counts"].count("10000") == 1 and re.search(r"[ACGT]9[ACGT]10[ACGT]99[ACGT]100[ACGT]999[ACGT]1000[ACGT]9999[ACGT]10000[ACGT]0$", seen["counts"])
    assert len(seen["mis130"]) == 261 and seen["m100001"] == "100001"
    # the records without the flag are these records without the tag
    for (_, with_md), (_, without) in zip(out, split_records(plain)):
        text = mc.md_and_nm(with_md)[0]
        assert with_md[4:-(4 + len(text))] == without[4:] and len(with_md) == len(without) + 4 + len(text)


# ---- 4. random reads -----------------------------------------------------------------------------------------------------------
def test_random_reads(tmp_path):
    references, refs, records, finals, arrays = mc.random_reads()
    assert len(records) == 2000
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "rnd")
    nb, nf, idx = open_pair(bp, fa)
    assert len(idx) == len(records)
    got = split_records(nb.format_bam_full(nf, idx, finals, np.zeros(len(idx), np.int32), md=True))
    nb.close(); nf.close()
    assert len(got) == len(records)
    n_words = set()
    for (_, rec), r, fin, (rc, sc) in zip(got, records, finals, arrays):
        assert rec[36:36 + rec[12] - 1].decode() == r["name"]
        text, nm, _, _ = mc.md_and_nm(rec)
        assert text == bam.md_of(rc, sc, fin), r["name"]
        assert nm == sum(c.isalpha() for c in text) + sum(n for op, n in r["cigar"] if op == 1), r["name"]
        n_words.add(len(r["cigar"]))
    assert {1, 64, 65, 200} <= n_words


# ---- 5. the surface ------------------------------------------------------------------------------------------------------------
def test_surface(crafted, tmp_path):
    tmp, bp, fa, refs, records, finals, pinned, status, got, plain = crafted
    nb, nf, idx = open_pair(bp, fa)
    lib = nb._lib
    for fmt, flags in ((1, MD), (1, MD | EOF), (1, MD | PART), (1, MD | DEFLATE | EOF), (1, MD | FULL), (0, MD | FULL | EOF), (0, MD), (1, 64 | FULL | EOF)):
        assert lib.npore_bam_set_output(nb.handle, fmt, None, flags) != 0, (fmt, flags)      # MD only with FULL (which needs EOF or PART, and BAM)
    for flags in (MD | FULL | EOF, MD | FULL | PART, MD | FULL | DEFLATE | EOF, MD | FULL | DEFLATE | MATCH | PART):
        assert lib.npore_bam_set_output(nb.handle, 1, None, flags) == 0, flags
    # npore_bam_write_file keeps refusing FULL, with MD beside it too
    out = str(tmp_path / "w.bam")
    _keep, reads = bam.marshal_finals(idx, finals, status)
    assert lib.npore_bam_set_output(nb.handle, 1, None, MD | FULL | EOF) == 0
    rc = lib.npore_bam_write_file(nb.handle, *reads[:2], 5, *reads[2:], 0, os.fsencode(out))
    assert rc == -5 and not os.path.exists(out)
    with pytest.raises(ValueError):
        nb.set_output("bam", md=True)
    with pytest.raises(ValueError):
        nb.set_output("sam", md=True)
    nb.set_output("bam", records="full", md=True)
    nb.set_output("sam")
    nb.close(); nf.close()
    # the header: the flag, what it writes and its one difference from calmd; both entry points bound
    hdr = open(os.path.join(REPO, "include", "npore_amd.h")).read()
    assert re.search(r"#define NPORE_OUT_MD 32\b", hdr) and re.search(r"#define NPORE_ABI_VERSION 2\b", hdr) and lib.npore_abi_version() == 2
    doc = hdr[hdr.index("#define NPORE_OUT_FULL 16"):hdr.index("#define NPORE_OUT_MD 32")]
    assert "calmd" in doc and "IUPAC" in doc and "NPORE_OUT_FULL" in doc and "--md" in doc
    declared = set(re.findall(r"\b(npore_[a-z_0-9]+)\s*\(", hdr)) - {"npore_ctx"}
    assert declared == set(_lib.SIGNATURES) and {"npore_bam_format_bam_full_md", "npore_debug_format_bam_full_md_device"} <= declared
    assert len(_lib.SIGNATURES["npore_bam_format_bam_full_md"][1]) == len(_lib.SIGNATURES["npore_bam_format_bam_full"][1]) + 1
    assert len(_lib.SIGNATURES["npore_debug_format_bam_full_md_device"][1]) == len(_lib.SIGNATURES["npore_debug_format_bam_full_device"][1]) + 2


def test_cli_md_needs_full_records(tmp_path):
    data = os.path.join(GOLDEN, "data")
    common = [sys.executable, "-m", "npore_amd.realign", "--bam", os.path.join(data, "reads.bam"), "--ref", os.path.join(data, "ref.fasta"),
              "--out_prefix", str(tmp_path / "bad"), "--md"]
    for extra in ([], ["--out_format", "bam"], ["--out_format", "bam", "--records", "reference"]):
        out = subprocess.run(common + extra, cwd=REPO, capture_output=True, text=True, timeout=120)
        assert out.returncode == 1, out.stdout[-2000:] + out.stderr[-2000:]
        errors = [l for l in out.stdout.splitlines() if l.startswith("ERROR")]
        assert len(errors) == 1 and "--md" in errors[0] and "--records full" in errors[0], out.stdout
        assert not os.path.exists(str(tmp_path / "bad.bam")) and not os.path.exists(str(tmp_path / "bad.sam"))


# ---- 6. the sequential twin under the sanitizers -------------------------------------------------------------------------------
def test_sequential_twin_under_sanitizers(tmp_path, crafted):
    tmp, bp, fa, refs, records, finals, pinned, status, got, plain = crafted
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = os.path.join(REPO, "tests", "model", "bam_md_sanitize.cpp")
    exe = str(tmp_path / "bam_md_sanitize")
    # (the runtimes linked statically: the program needs nothing preloaded and does not mind what is)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + san + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is missing")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + san + ["-o", exe, src])
    blob, want = [], []
    for r, fin in zip(records, finals):
        if r["_status"]:
            continue
        rc, sc, _ = lc.expected_pack(r, r["cigar"], refs[r["_ctg"]])
        words = [int(n) << 4 | "MID".index(op) for n, op in re.findall(r"(\d+)([MID])", fin)]
        blob.append(struct.pack("<qqq", len(words), len(rc), len(sc)) + struct.pack(f"<{len(words)}I", *words) + rc.tobytes() + sc.tobytes())
        want.append(pinned.get(r["name"]) or bam.md_of(rc, sc, fin))
    for ref, seq, fin, md in mc.TABLE:
        words = [int(n) << 4 | "MID".index(op) for n, op in re.findall(r"(\d+)([MID])", fin)]
        blob.append(struct.pack("<qqq", len(words), len(ref), len(seq)) + struct.pack(f"<{len(words)}I", *words) + mc.codes(ref).tobytes() + mc.codes(seq).tobytes())
        want.append(md)
    cases = str(tmp_path / "cases.bin")
    with open(cases, "wb") as fh:
        fh.write(b"".join(blob))
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]
    assert out.stdout.split("\n")[:-1] == want
