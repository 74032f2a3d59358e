"""The OC tag of the FULL records (--records full --oc) on the GPU: oc_size_kernel in front of the placement -- it decides on the
device whether a read changed, which the host cannot: it never sees the final words -- and emit_oc_kernel behind the assembly
(csrc/bam_emit_kernels.hpp) against the host twin npore_bam_format_bam_full_pass, which tests/test_bam_oc.py holds to the Python
statement: on the crafted reads of bam_oc_cases through the debug entry with the bit alone, with all tags and the =/X form and
with a pass mask, the reads handed in one by one and four at a time, on inputs of more than 65 535 words, and in the file pipeline
on a file whose reads the reference changes and does not change.  The rule is stated in csrc/oc_rec.hpp.
"""
import argparse
import os

import numpy as np
import pytest

from npore_amd import aln, bam, cfg
from conftest import GOLDEN
from test_bam_out import Hdr, check_index, members, split_records
from test_gpu_bam_full import realign_cli, record_stream
import bam_full_cases as fc
import bam_oc_cases as oc
import long_cigar_cases as lc
from full_record_driver import device_full

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, "data")
ALL_TAGS = dict(md=True, cs="long", de=True, eqx=True)


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
            return b[36:36 + b[12] - 1], [t[:80] for t in oc.oc_of_record(a)[0]], [t[:80] for t in oc.oc_of_record(b)[0]], len(a), len(b)
    return len(got), len(want)


def open_all(bp, fa):
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in zip(nb.references, nb.lengths)], pass_mask=bam.PASS_FLAGS)      # (the secondary record too)
    return nb, nf, idx


# ---- 1. the crafted sets through the debug entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oc", "long"])
def test_device_equals_host(ctx, tmp_path, which):
    references, refs, records, finals, changed = {"oc": oc.oc_reads, "long": oc.long_reads}[which]()[:5]
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, which)
    nb, nf, idx = open_all(bp, fa)
    assert len(idx) == len(records)
    status = np.array([r["_status"] for r in records], np.int32)
    for kw in (dict(), ALL_TAGS, dict(mask=0x904), dict(mask=0x100, **ALL_TAGS)):
        host_kw = {("pass_mask" if k == "mask" else k): v for k, v in kw.items()}
        want = nb.format_bam_full(nf, idx, finals, status, oc=True, **host_kw)
        got = device_full(ctx, nb, nf, idx, finals, status, cap=len(want) + 4096, oc=True, **kw)[0]
        assert got == want, (kw, first_difference(got, want))
        # the bit off: the same entry writes the bytes it wrote before
        plain = nb.format_bam_full(nf, idx, finals, status, **host_kw)
        assert device_full(ctx, nb, nf, idx, finals, status, cap=len(plain) + 4096, oc=False, **kw)[0] == plain != want
    # which records carry the tag is the statement's answer (the host twin's bytes say no more than that they agree)
    kept = [r for r in records if not r["_status"]]
    for (_, rec), r in zip(split_records(device_full(ctx, nb, nf, idx, finals, status, cap=len(want) + 4096, oc=True)[0]), kept):
        assert oc.oc_of_record(rec)[0] == ([oc.text_of(r["cigar"])] if changed[r["name"]] else []), r["name"]
    # the reads handed in one by one and four at a time: every call's records are those of the one call
    for kw in (dict(), ALL_TAGS):
        want = split_records(nb.format_bam_full(nf, idx, finals, status, oc=True, **kw))
        for size in (1, 4):
            got = []
            for lo in range(0, len(idx), size):
                got += split_records(device_full(ctx, nb, nf, idx[lo:lo + size], finals[lo:lo + size], status[lo:lo + size],
                                                 cap=sum(len(r) for _, r in want) + 4096, oc=True, **kw)[0])
            assert [r for _, r in got] == [r for _, r in want], (kw, size)
    if which == "oc":                                            # the same reads picked in another order, in one call
        pick = np.random.default_rng(3).integers(0, len(records), 200)
        want = nb.format_bam_full(nf, idx[pick], [finals[k] for k in pick], status[pick], oc=True, **ALL_TAGS)
        assert device_full(ctx, nb, nf, idx[pick], [finals[k] for k in pick], status[pick], cap=len(want) + 4096, oc=True, **ALL_TAGS)[0] == want
    nb.close(); nf.close()


# ---- 2. the file pipeline on reads the reference changes and reads it does not ----------------------------------------------------------
def test_file_pipeline(ctx, tables, tmp_path):
    references, refs, records = oc.pipeline_reads()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "pipe")
    regions = [("ctg", 0, references[0][1] - 1)]
    finals = oc.oracle_finals(records, refs, tables)             # the reference's own, once
    raws = fc.input_records(bp)
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=regions, max_reads=0)
    try:
        nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
        reads, every = nb.select(regions), nb.select(regions, pass_mask=bam.PASS_FLAGS)
        assert len(every) == len(records) and len(reads) == len(records) - 4

        def want(idx, mask=0, **kw):
            pick = lambda xs: [xs[k] for k in idx]
            return oc.want_stream(pick(raws), pick(records), refs, pick(finals), np.zeros(len(idx), np.int32), mask=mask, **kw)

        def run(handle, name, idx, **kw):
            out = str(tmp_path / name)
            bam.create_bam_header(out, Hdr(handle.references, handle.lengths))
            st = handle.realign_file(ctx, nf, idx, out, batch_reads=16, r=30, out_format="bam", bai=out + ".bai", records="full", **kw)
            assert not (st & 32).any(), name
            check_index(out, out + ".bai")
            return record_stream(out)

        dev = run(nb, "dev.bam", reads, oc=True)
        assert dev == want(reads)                                # the Python records built from the oracle's finals
        with_tag = [bool(oc.oc_of_record(rec)[0]) for _, rec in split_records(dev)]
        assert any(with_tag) and not all(with_tag)               # both kinds of read
        for (_, rec), k in zip(split_records(dev), reads):       # an OC the input carried: replaced on a changed read, gone otherwise
            if b"OCZ1M\0" in records[k]["tags"]:
                assert oc.oc_of_record(rec)[0] == ([oc.text_of(records[k]["cigar"])] if k % 2 else [])
        ctx.set("device_pack", 0)                                # the host twin makes the records
        ctx.set("device_glue", 0)
        try:
            assert run(nb, "host.bam", reads, oc=True) == dev
        finally:
            ctx.set("device_pack", 1)
            ctx.set("device_glue", 1)
        assert run(nb, "match.bam", reads, oc=True, compress="match") == dev      # (the inflated bytes)
        members(str(tmp_path / "match.bam"))
        more = dict(eqx=True, md=True, cs="short", de=True)
        assert run(nb, "tags.bam", reads, oc=True, **more) == want(reads, **more)
        passed = run(nb, "pass.bam", every, oc=True, pass_mask=bam.PASS_FLAGS)
        assert passed == want(every, mask=bam.PASS_FLAGS)
        assert sum(rec in raws for _, rec in split_records(passed)) == 4 and passed.count(b"OCZ9M9I\0") == 4      # as they came
        # ---- the flag off: the bytes of a run on a handle that never heard of the option
        off = run(nb, "off.bam", reads)
        fresh = bam.NativeBam(bp)
        assert off == run(fresh, "fresh.bam", reads) == want(reads, oc=False) != dev
        assert off.count(b"OCZ1M\0") == 2                        # (an input's OC stays as it came)
        fresh.close(); nb.close(); nf.close()
    finally:
        cfg.args = old


# ---- 3. the tool -----------------------------------------------------------------------------------------------------------------------
def test_cli_oc_on_the_golden_bam(tmp_path):
    bp, fa = os.path.join(DATA, "reads.bam"), os.path.join(DATA, "ref.fasta")
    common = ["--bam", bp, "--ref", fa, "--out_format", "bam", "--records", "full"]
    p0, p1 = str(tmp_path / "plain"), str(tmp_path / "oc")
    realign_cli(common + ["--out_prefix", p0], 300)
    realign_cli(common + ["--out_prefix", p1, "--oc"], 300)
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l - 1) for n, l in zip(nb.references, nb.lengths)])
    codes = lc.native_pack_per_read(nb, nf, idx)
    raws = fc.input_records(bp)
    nb.close(); nf.close()
    plain, tagged = (split_records(record_stream(p + ".bam")) for p in (p0, p1))
    assert len(plain) == len(tagged) == len(idx) == 10
    for (_, a), (_, b), k, (rc, sc, _) in zip(plain, tagged, idx, codes):
        words = fc.parse_full(a)[2]
        i, j = oc.clip_range([(w & 15, w >> 4) for w in words])
        final = "".join(f"{w >> 4}{oc.OPS[w & 15]}" for w in words[i:j])      # the run's own final CIGAR
        assert a == bam.full_record(raws[k], rc, sc, final) and b == bam.full_record(raws[k], rc, sc, final, oc=True)
        assert bool(oc.oc_of_record(b)[0]) == bam.cigar_changed(oc.inner([(w & 15, w >> 4) for w in fc.parse_full(raws[k])[2]]), final)
    check_index(p1 + ".bam", p1 + ".bam.bai")
