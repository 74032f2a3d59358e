"""FULL records (--records full, NPORE_OUT_FULL), host side: the aux filter, the record encoder npore_bam_format_bam_full and
the NM rule against the statement in npore_amd/csrc/bam_reader.hpp ("FULL RECORD") and csrc/nm_rec.hpp and their
pure-Python twins bam.filter_aux / bam.full_record / bam.nm_of.  No GPU here: the final CIGARs are given.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from npore_amd import bam, _lib
from conftest import REPO
from test_bam_out import Hdr, decoded_lines, split_records
import bam_full_cases as fc
import long_cigar_cases as lc

EOF, PART, DEFLATE, MATCH, FULL, MD = bam.OUT_EOF, bam.OUT_PART, bam.OUT_DEFLATE, bam.OUT_MATCH, bam.OUT_FULL, bam.OUT_MD      # npore_bam_set_output's flags

def open_pair(bp, fa):
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in zip(nb.references, nb.lengths)])
    return nb, nf, idx


# ---- 1. the aux filter ---------------------------------------------------------------------------------------------------
def test_aux_filter(tmp_path):
    bp = str(tmp_path / "aux.bam")
    contig, records, auxs, kept = fc.aux_bam(bp)
    fa = lc.write_fasta(str(tmp_path / "aux.fa"), {"ctg": contig})
    for (name, aux, want) in fc.aux_cases():
        assert bam.filter_aux(aux) == want, name
    nb, nf, idx = open_pair(bp, fa)
    assert len(idx) == len(records)
    finals = ["20M1I9M"] * len(records)
    got = split_records(nb.format_bam_full(nf, idx, finals, np.zeros(len(idx), np.int32)))
    assert len(got) == len(records)
    for (_, rec), raw, aux, want in zip(got, fc.input_records(bp), auxs, kept):
        f, name, words, body, tags = fc.parse_full(rec)
        assert tags[:len(want)] == want and tags[len(want):len(want) + 3] == b"NMC" and len(tags) == len(want) + 4, name
        assert words == [1 << 4 | 4, 20 << 4, 1 << 4 | 1, 9 << 4, 2 << 4 | 5]
        assert raw.endswith(aux)
    nb.close(); nf.close()


# ---- 2. the record ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_full")
    references, refs, records, cigars = fc.full_records()
    bp, fa = fc.write_inputs(tmp, references, refs, records)
    finals = []
    for k, (rec, cig) in enumerate(zip(records, cigars)):
        rc, sc, _ = lc.expected_pack(rec, cig, refs["ctg"])
        finals.append(fc.simple_final(len(rc), len(sc), k))
    status = np.zeros(len(records), np.int32)
    status[7] = 32                                             # the read whose CIGAR disagrees with its sequence
    return tmp, bp, fa, references, refs, records, cigars, finals, status


def test_record_equals_python_statement(full_inputs):
    tmp, bp, fa, references, refs, records, cigars, finals, status = full_inputs
    nb, nf, idx = open_pair(bp, fa)
    assert len(idx) == len(records)
    got = nb.format_bam_full(nf, idx, finals, status)
    raws = fc.input_records(bp)
    assert got == fc.want_stream(raws, records, cigars, refs["ctg"], finals, status)
    # field by field, from the bytes
    kept = [k for k in range(len(records)) if k != 7]
    out = split_records(got)
    assert len(out) == len(kept)
    seen_lead, seen_trail = set(), set()
    for (_, rec), k in zip(out, kept):
        r, raw = records[k], raws[k]
        f, name, words, body, tags = fc.parse_full(rec)
        fin = struct.unpack_from("<iiBBHHHiiii", raw, 4)
        assert f[:4] == fin[:4] and f[6:] == fin[6:], k                    # all but bin and n_cigar_op are the input's
        assert (f[8], f[9], f[10]) == ((0, r["pos"] + 100 + k, 500 + k) if k % 2 else (-1, -1, 0))
        assert f[7] == len(r["seq"]) and name == r["name"].encode() + b"\0"
        q = 36 + fin[2] + 4 * fin[5]
        assert body == raw[q:q + len(body)]                                # bases and qualities verbatim, clips included
        if r["qual"] is None and len(r["seq"]):
            assert body[(len(r["seq"]) + 1) // 2] == 0xFF
        cig = [(w & 15, w >> 4) for w in words]
        lead = [c for c in r["cigar"][:2] if c[0] in (4, 5)] if r["cigar"][0][0] in (4, 5) else []
        if len(lead) == 2 and not (lead[0][0] == 5 and lead[1][0] == 4):
            lead = lead[:1]
        n_fin = finals[k].count("M") + finals[k].count("I") + finals[k].count("D")
        assert cig[:len(lead)] == lead and "".join(f"{n}{'MID'[op]}" for op, n in cig[len(lead):len(lead) + n_fin]) == finals[k], k
        assert cig[len(lead) + n_fin:] == [c for c in r["cigar"][-2:] if c[0] in (4, 5)][-(len(cig) - len(lead) - n_fin) or len(cig):], k
        seen_lead.add(tuple(op for op, _ in lead)); seen_trail.add(tuple(op for op, _ in cig[len(lead) + n_fin:]))
        hp = fc.HP_TAGS[k % len(fc.HP_TAGS)]
        assert (hp in tags) if hp else b"HP" not in tags
        for stale in (b"NMC\x05", b"MDZ", b"def"):
            assert stale not in tags[:-4]
        assert tags[-4:-1] in (b"NMC",) or tags[-5:-2] == b"NMS"
    assert seen_lead == {(), (4,), (5, 4), (5,)} and seen_trail == {(), (4,), (4, 5), (5,)}
    nb.close(); nf.close()


# ---- 3. the long threshold -------------------------------------------------------------------------------------------------
def test_long_threshold(tmp_path):
    rng = np.random.default_rng(2)
    contig = lc.random_contig(rng, 140000)
    recs, finals = [], []
    for k, n_d in enumerate((32766, 32767)):                   # 65 533 and 65 534 final operations, + 2 clips
        body = contig[100:100 + 32767] if k == 0 else contig[70000:70000 + 32767]
        recs.append(dict(name=f"t{k}", flag=0, ref_id=0, pos=100 if k == 0 else 70000, mapq=9, seq="GG" + body + "TTT",
                         cigar=[(4, 2), (0, 16000), (2, n_d), (0, 16767), (4, 3)], qual=bytes(32772), tags=b"RGZx\0NMi" + struct.pack("<i", 3)))
        finals.append("1M1D" * 32766 + ("1M" if k == 0 else "1M1D"))
    bp, fa = fc.write_inputs(tmp_path, [("ctg", len(contig))], {"ctg": contig}, recs, "long")
    nb, nf, idx = open_pair(bp, fa)
    got = nb.format_bam_full(nf, idx, finals, np.zeros(2, np.int32))
    raws = fc.input_records(bp)
    assert got == fc.want_stream(raws, recs, [r["cigar"] for r in recs], contig, finals, [0, 0])
    (_, plain), (_, lng) = split_records(got)
    f, _, words, _, tags = fc.parse_full(plain)
    assert f[5] == 65535 and words[0] == 2 << 4 | 4 and words[-1] == 3 << 4 | 4 and tags.startswith(b"RGZx\0NM") and b"CGB" not in tags
    f, _, words, _, tags = fc.parse_full(lng)
    assert f[5] == 2 and words == [32772 << 4 | 4, (32767 + 32767) << 4 | 3]
    assert tags.startswith(b"RGZx\0NM") and tags[5 + 3 + 2:5 + 3 + 2 + 8] == b"CGBI" + struct.pack("<I", 65536)     # (NM = 32 767+: type S)
    cg = struct.unpack_from("<65536I", tags, 5 + 3 + 2 + 8)
    assert cg[0] == 2 << 4 | 4 and cg[-1] == 3 << 4 | 4 and cg[1:3] == (1 << 4, 1 << 4 | 2) and len(tags) == 18 + 4 * 65536
    nb.close(); nf.close()


# ---- 4. NM -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_full_nm")
    references, refs, records, finals = fc.crafted_reads()
    bp, fa = fc.write_inputs(tmp, references, refs, records, "nm")
    return tmp, bp, fa, refs, records, finals


def test_nm_against_brute_force(crafted):
    tmp, bp, fa, refs, records, finals = crafted
    nb, nf, idx = open_pair(bp, fa)
    assert len(idx) == len(records)
    status = np.array([r["_status"] for r in records], np.int32)
    got = nb.format_bam_full(nf, idx, finals, status)
    raws = fc.input_records(bp)
    assert got == fc.want_stream(raws, records, [r["cigar"] for r in records], refs["ctg"], finals, status)
    out = iter(split_records(got))
    seen = {}
    for r, fin in zip(records, finals):
        if r["_status"]:
            continue
        _, rec = next(out)
        rc, sc, _ = lc.expected_pack(r, r["cigar"], refs["ctg"])
        ref = refs["ctg"][r["pos"]:r["pos"] + len(rc)]
        lead = sum(n for op, n in r["cigar"][:2] if op == 4)
        seq = r["seq"][lead:lead + len(sc)]
        want = fc.brute_nm(ref, seq, fin)
        assert bam.nm_of(rc, sc, fin) == want, r["name"]
        assert rec.endswith(fc.nm_tag(want)), r["name"]
        seen[r["name"]] = want
    assert next(out, None) is None
    assert (seen["nm255"], seen["nm256"], seen["nm65536"], seen["all_i"], seen["all_d"]) == (255, 256, 65536, 40, 40)
    assert (seen["n_in_ref"], seen["n_in_read"], seen["n_in_both"]) == (3, 1, 3)
    assert seen["run1"] == 2 + 3 + 1 and seen["run200"] == 2 + 3 + 4 and seen["run64"] == 2 + 3 + 2 and seen["run65"] == 2 + 3 + 3
    nb.close(); nf.close()


# ---- 5. decoding -----------------------------------------------------------------------------------------------------------
def test_decoded_lines_equal_sam(full_inputs):
    tmp, bp, fa, references, refs, records, cigars, finals, status = full_inputs
    nb, nf, idx = open_pair(bp, fa)
    out = str(tmp / "decoded.bam")
    bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
    with open(out, "ab") as fh:
        fh.write(bam.bgzf_stored(nb.format_bam_full(nf, idx, finals, status)) + bam.BGZF_EOF)
    sam = nb.format_sam(idx, finals, status)
    lines = decoded_lines(out, refs)
    assert fc.without_clips(lines) == sam.splitlines(keepends=True) and sam.count("\n") == len(records) - 1
    assert sum("S" in l.split("\t")[5] for l in lines) == 12 and sum("H" in l.split("\t")[5] for l in lines) == 11      # (read 7, refused, has H clips)
    hps = [int(l.rstrip("\n").split("HP:i:")[1]) for l in sam.splitlines()]
    assert hps == [r["_hp"] for k, r in enumerate(records) if k != 7] and len(set(hps)) == 7
    nb.close(); nf.close()


# ---- 6. the sanitizer ------------------------------------------------------------------------------------------------------
def test_malformed_records_under_sanitizers(tmp_path, crafted):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = os.path.join(REPO, "tests", "model", "bam_full_sanitize.cpp")
    exe = str(tmp_path / "bam_full_sanitize")
    # (the runtimes linked statically: the program needs nothing preloaded and does not mind what is)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + san + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is missing")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + san + ["-o", exe, src, "-lz", "-lpthread"])
    bp = str(tmp_path / "aux.bam")
    fc.aux_bam(bp)
    stream = str(tmp_path / "records.bin")
    raws = fc.input_records(bp) + fc.input_records(crafted[1])
    with open(stream, "wb") as fh:
        fh.write(b"".join(raws))
    out = subprocess.run([exe, stream], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.startswith(f"{len(raws)} records")


# ---- 7. errors -------------------------------------------------------------------------------------------------------------
def test_errors_and_surface(full_inputs, tmp_path):
    tmp, bp, fa, references, refs, records, cigars, finals, status = full_inputs
    nb, nf, idx = open_pair(bp, fa)
    lib = nb._lib
    assert lib.npore_bam_set_output(nb.handle, 0, None, FULL) != 0         # NPORE_OUT_FULL needs NPORE_OUT_BAM
    assert lib.npore_bam_set_output(nb.handle, 1, None, MD) != 0
    assert lib.npore_bam_set_output(nb.handle, 1, None, FULL) != 0         # ... and one of EOF / PART: FULL alone stays refused
    assert lib.npore_bam_set_output(nb.handle, 1, None, FULL | DEFLATE) != 0
    for flags in (FULL | EOF, FULL | PART, FULL | DEFLATE | EOF, FULL | DEFLATE | MATCH | PART):      # ... and combines with EOF, PART, DEFLATE, MATCH
        assert lib.npore_bam_set_output(nb.handle, 1, None, flags) == 0
    out = str(tmp_path / "w.bam")
    _keep, reads = bam.marshal_finals(idx, finals, status)
    assert lib.npore_bam_set_output(nb.handle, 1, None, FULL | EOF) == 0
    rc = lib.npore_bam_write_file(nb.handle, *reads[:2], 5, *reads[2:], 0, os.fsencode(out))
    assert rc == -5 and "NM" in _lib.last_error() and not os.path.exists(out)      # NPORE_E_UNSUPPORTED
    # (the setting held for that one run: the reference form again)
    bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
    assert nb.write_file(idx, finals, status, out, batch_reads=5)["records"] == len(records) - 1
    with pytest.raises(ValueError):
        nb.set_output("sam", records="full")
    with pytest.raises(ValueError):
        nb.set_output("bam", records="whole")
    import re
    hdr = open(os.path.join(REPO, "include", "npore_amd.h")).read()
    declared = set(re.findall(r"\b(npore_[a-z_0-9]+)\s*\(", hdr)) - {"npore_ctx"}
    assert declared == set(_lib.SIGNATURES) and {"npore_bam_format_bam_full", "npore_debug_format_bam_full_device"} <= declared
    assert re.search(r"#define NPORE_OUT_FULL 16\b", hdr) and re.search(r"#define NPORE_ABI_VERSION 2\b", hdr)
    for name in declared:
        assert hasattr(lib, name), name
    nb.close(); nf.close()
