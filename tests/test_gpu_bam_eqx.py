"""The =/X form of the FULL records' CIGARs (--records full --eqx) on the GPU: eqx_size_kernel in front of the placement and
emit_eqx_kernel behind the assembly (csrc/bam_emit_kernels.hpp, ONE walk with two sinks) against the host twin
npore_bam_format_bam_full_pass, which tests/test_bam_eqx.py holds to the Python statement -- on the crafted and the seam reads
through the debug entry with the bit alone, with all tags and with a pass mask, on either side of the CG threshold, over two
calls between which the engine's eqx_len buffer has to grow and in a batch cut into several groups, and on the golden BAM
through the tool.  The rule is stated in csrc/eqx_rec.hpp.  Every child process runs under its own time limit.
"""
import argparse
import os

import numpy as np
import pytest

from npore_amd import aln, bam, cfg
from conftest import GOLDEN
from test_bam_out import Hdr, check_index, members, split_records
from test_gpu_bam_full import realign_cli, record_stream
import bam_cs_cases as cc
import bam_eqx_cases as ec
import bam_full_cases as fc
import bam_md_cases as mc
import bam_pass_cases as pc
import long_cigar_cases as lc
from full_record_driver import device_full

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, "data")
ALL_TAGS = dict(md=True, cs="long", de=True)


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


def first_difference(got, want):
    """the first record that differs, by name (the assertion's message)"""
    for (_, a), (_, b) in zip(split_records(got), split_records(want)):
        if a != b:
            return b[36:36 + b[12] - 1], ec.record_cigar_text(a)[0][:200], ec.record_cigar_text(b)[0][:200]
    return len(got), len(want)


# ---- 1. the crafted and the seam reads through the debug entry: alone, with all tags ---------------------------------------------
@pytest.mark.parametrize("which", ["eqx", "cs", "seam", "md"])
def test_device_equals_host(ctx, tmp_path, which):
    pack = {"eqx": ec.eqx_reads, "cs": cc.crafted_reads, "seam": cc.seam_reads, "md": mc.crafted_reads}[which]()
    references, refs, records, finals = pack[:4]
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, which)
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in references])
    assert len(idx) == len(records)
    status = np.array([r["_status"] for r in records], np.int32)
    for kw in (dict(), ALL_TAGS):
        want = nb.format_bam_full(nf, idx, finals, status, eqx=True, **kw)
        got = device_full(ctx, nb, nf, idx, finals, status, cap=len(want) + 4096, eqx=True, **kw)[0]
        assert got == want, (kw, first_difference(got, want))
        # eqx_len, as the record says it: n_cigar_op (the CG tag's count) is the clip words plus the split words
        kept = [(r, f) for r, f in zip(records, finals) if not r["_status"]]
        for (_, rec), (r, fin) in zip(split_records(got), kept):
            rc, sc, _ = lc.expected_pack(r, r["cigar"], refs[r.get("_ctg", "ctg")])
            text, n_cig = ec.record_cigar_text(rec)
            lead, mid, trail = ec.split_clips(text)
            assert mid == bam.eqx_of(rc, sc, fin), r["name"]
            n_words = len(ec.runs_of(text))
            assert n_cig == (2 if n_words > 0xFFFF else n_words), r["name"]
        # without the bit the same entry writes the bytes it wrote before
        plain = nb.format_bam_full(nf, idx, finals, status, **kw)
        assert device_full(ctx, nb, nf, idx, finals, status, cap=len(plain) + 4096, eqx=False, **kw)[0] == plain != want
    if which == "eqx":                                           # the same reads picked in another order, in one call
        pick = np.random.default_rng(2).integers(0, len(records), 150)
        want = nb.format_bam_full(nf, idx[pick], [finals[k] for k in pick], status[pick], eqx=True, **ALL_TAGS)
        assert device_full(ctx, nb, nf, idx[pick], [finals[k] for k in pick], status[pick], cap=len(want) + 4096, eqx=True, **ALL_TAGS)[0] == want
    nb.close(); nf.close()


@pytest.mark.parametrize("mask", [0x904, 0x100])
def test_device_with_a_pass_mask(ctx, tmp_path, mask):
    references, refs, records = pc.pass_file()
    bp, fa = str(tmp_path / "p.bam"), str(tmp_path / "p.fa")
    pc.write_bam(bp, references, records)
    lc.write_fasta(fa, refs)
    raws, finals = fc.input_records(bp), pc.finals_of(records)
    status = np.array([32 if r["_kind"] == "refused" else 0 for r in records], np.int32)
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = np.array(pc.py_select(raws, [(0, 0, 1 << 28), (1, 0, 1 << 28)], 0, mask), np.int64)
    for kw in (dict(), ALL_TAGS):
        want = nb.format_bam_full(nf, idx, [finals[k] for k in idx], status[idx], pass_mask=mask, eqx=True, **kw)
        got = device_full(ctx, nb, nf, idx, [finals[k] for k in idx], status[idx], cap=len(want) + 4096, mask=mask, eqx=True, **kw)[0]
        assert got == want, (kw, first_difference(got, want))
    passed = [r for k, (_, r) in zip([k for k in idx if k != 12], split_records(got)) if pc.passes(records[k]["flag"], mask)]
    assert passed and all(r in raws for r in passed)             # as they came
    nb.close(); nf.close()


# ---- 2. either side of the CG threshold ---------------------------------------------------------------------------------------------
def test_cg_threshold_on_the_device(ctx, tmp_path):
    references, refs, records, finals = ec.cg_reads()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "cg")
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in references])
    st = np.zeros(2, np.int32)
    for kw in (dict(), ALL_TAGS):
        want = nb.format_bam_full(nf, idx, finals, st, eqx=True, **kw)
        got = device_full(ctx, nb, nf, idx, finals, st, cap=len(want) + 4096, eqx=True, **kw)[0]
        assert got == want, (kw, first_difference(got, want))
        (_, plain), (_, long) = split_records(got)
        assert ec.record_cigar_text(plain) == ("1S" + "1=1X" * 32766 + "1=" + "2S", 65535) and b"CGBI" not in plain
        assert ec.record_cigar_text(long) == ("1S" + "1=1X" * 32767 + "2S", 2)
        assert mc.parse_tags(fc.parse_full(long)[4])[-1][2][:5] == b"I" + (65536).to_bytes(4, "little")
    nb.close(); nf.close()


# ---- 3. the eqx_len buffer grows between two calls on one context; several groups give the bytes of one ------------------------------
def test_eqx_len_grows_and_groups_agree(ctx, tables, tmp_path):
    references, refs, records, cigars = fc.full_records(n_reads=120)
    bp, fa = fc.write_inputs(tmp_path, references, refs, records)
    regions = [("ctg", 0, references[0][1] - 1)]
    sub, nps = tables
    own = aln.Context(sub, nps, max_n=6, max_l=100, device=0)     # a context of its own for the two calls: its buffers start empty
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=regions, max_reads=0)
    try:
        nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
        idx = nb.select(regions)
        assert len(idx) == 120
        sam = tmp_path / "route.sam"
        st = nb.realign_file(ctx, nf, idx, str(sam), batch_reads=1000, r=30)
        assert ((st & 32) != 0).sum() == 1 and st[7] & 32
        it = iter(sam.read_text().splitlines())
        finals = ["" if st[k] & 32 else next(it).split("\t")[5] for k in range(120)]
        want = []                                                # the statement, once, for both whole runs
        for raw, rec, cig, fin, s in zip(fc.input_records(bp), records, cigars, finals, st):
            if not s & 32:
                rc, sc, _ = lc.expected_pack(rec, cig, refs["ctg"])
                want.append(bam.full_record(raw, rc, sc, fin, eqx=True, **ALL_TAGS))
        want = b"".join(want)

        def run(c, name, lo, hi, **kw):
            out = str(tmp_path / name)
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            stb = nb.realign_file(c, nf, idx[lo:hi], out, r=30, out_format="bam", bai=out + ".bai", records="full", eqx=True, **ALL_TAGS, **kw)
            assert np.array_equal(stb, st[lo:hi])
            check_index(out, out + ".bai")
            return record_stream(out)
        # 3 reads: eqx_len holds 3 * 4 + 64 bytes and its head-room, fewer than the 120 * 4 + 64 the second call needs
        assert run(own, "grow3.bam", 0, 3, batch_reads=1000) == nb.format_bam_full(nf, idx[:3], finals[:3], st[:3], eqx=True, **ALL_TAGS)
        assert run(own, "grow120.bam", 0, 120, batch_reads=1000) == want
        own.set("tb_budget_mb", 2)                               # every batch in several groups
        try:
            assert run(own, "groups.bam", 0, 120, batch_reads=12) == want
        finally:
            own.set("tb_budget_mb", 0)
        nb.close(); nf.close()
    finally:
        cfg.args = old
        own.close()


# ---- 4. the golden BAM through the tool ---------------------------------------------------------------------------------------------
def test_cli_eqx_on_the_golden_bam(tmp_path):
    bp, fa = os.path.join(DATA, "reads.bam"), os.path.join(DATA, "ref.fasta")
    common = ["--bam", bp, "--ref", fa, "--out_format", "bam", "--records", "full"]
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain", "eqx", "all"))
    realign_cli(common + ["--out_prefix", p0], 300)
    realign_cli(common + ["--out_prefix", p1, "--eqx"], 300)
    realign_cli(common + ["--out_prefix", p2, "--eqx", "--bam_compress", "match", "--md", "--cs", "long", "--de", "--pass_through"], 300)
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    regions = [(n, 0, l - 1) for n, l in zip(nb.references, nb.lengths)]
    idx = nb.select(regions)
    codes = lc.native_pack_per_read(nb, nf, idx)
    raws = fc.input_records(bp)
    passing = [int(k) for k in nb.select(regions, pass_mask=bam.PASS_FLAGS) if k not in set(idx.tolist())]
    nb.close(); nf.close()
    plain, eqx, full = (split_records(record_stream(p + ".bam")) for p in (p0, p1, p2))
    assert len(plain) == len(eqx) == len(idx) == 10 and len(full) == 10 + len(passing)
    assert [r for _, r in full if r in [raws[k] for k in passing]] == [raws[k] for k in passing]      # --pass_through: as they came
    full = [(o, r) for o, r in full if r not in [raws[k] for k in passing]]
    for (_, a), (_, b), (_, c), k, (rc, sc, _) in zip(plain, eqx, full, idx, codes):
        ta, tb = ec.record_cigar_text(a)[0], ec.record_cigar_text(b)[0]
        final = ec.without_outer_clips(ta)                       # the run's own final CIGAR, which has M
        assert "=" not in ta and "X" not in ta and ("=" in tb or "X" in tb)
        assert b == bam.full_record(raws[k], rc, sc, final, eqx=True)
        assert ec.canonical_m(tb) == ec.canonical_m(ta)          # collapsing gives the CIGAR of the run without --eqx
        fa_, name_a, _, body_a, aux_a = fc.parse_full(a)
        fb_, name_b, _, body_b, aux_b = fc.parse_full(b)
        assert fa_[:5] + fa_[6:] == fb_[:5] + fb_[6:] and name_a == name_b and body_a == body_b and aux_a == aux_b      # every other byte
        ec.eqx_identities(ec.without_outer_clips(tb), final, bam.nm_of(rc, sc, final), bam.cs_of(rc, sc, final))
        assert c == bam.full_record(raws[k], rc, sc, final, eqx=True, **ALL_TAGS)
    for p in (p0, p1, p2):
        members(p + ".bam")
        check_index(p + ".bam", p + ".bam.bai")
