"""The cs and de tags of the FULL records (--records full --cs short|long --de) on the GPU: cs_size_kernel and emit_cs_kernel
(csrc/bam_emit_kernels.hpp, ONE walk with two sinks) against the host twin npore_bam_format_bam_full_tags -- on the crafted and
the random final CIGARs through the debug entry in every combination of {cs short, cs long, none} x {de} x {md}, on the golden
BAM through the one-pass file pipeline with stored and with coded members, and over two calls between which the engine's cs_len
buffer has to grow.  The rule is stated in csrc/cs_rec.hpp.
"""
import argparse
import os
import struct

import numpy as np
import pytest

from npore_amd import aln, bam, cfg
from conftest import GOLDEN
from test_bam_out import Hdr, check_index, members, split_records
from test_gpu_bam_full import record_stream
import bam_cs_cases as cc
import bam_full_cases as fc
import bam_md_cases as mc
from full_record_driver import device_full

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, "data")
COMBOS = [(md, cs, de) for md in (False, True) for cs in cc.FORMS for de in (False, True)]


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


# ---- 1. the crafted and the random reads through the debug entry, every combination --------------------------------------------
@pytest.mark.parametrize("which", ["cs", "md", "random", "seam"])
def test_device_equals_host(ctx, tmp_path, which):
    if which == "random":
        references, refs, records, finals, _ = mc.random_reads()
        for r in records:
            r.setdefault("_status", 0)
    elif which == "seam":                                            # the seams of the walks' frame: a tile's last word, a round's last position
        references, refs, records, finals = cc.seam_reads()
    else:
        references, refs, records, finals, _ = (cc if which == "cs" else mc).crafted_reads()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, which)
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in references])
    assert len(idx) == len(records)
    status = np.array([r["_status"] for r in records], np.int32)
    seen = set()
    for md, cs, de in COMBOS:
        want = nb.format_bam_full(nf, idx, finals, status, md=md, cs=cs, de=de)
        got = device_full(ctx, nb, nf, idx, finals, status, cap=len(want) + 4096, entry="_tags", md=md, cs=cs, de=de)[0]
        if got != want:                                          # the first record that differs, by name
            for (_, a), (_, b) in zip(split_records(got), split_records(want)):
                assert a == b, (md, cs, de, b[36:36 + b[12] - 1], a[-80:], b[-80:])
        assert got == want, (md, cs, de)
        seen.add(want)
    assert len(seen) == len(COMBOS)                              # every combination writes bytes of its own
    if which == "cs":                                            # the same reads picked in another order, in one call
        pick = np.random.default_rng(2).integers(0, len(records), 200)
        want = nb.format_bam_full(nf, idx[pick], [finals[k] for k in pick], status[pick], md=True, cs="long", de=True)
        assert device_full(ctx, nb, nf, idx[pick], [finals[k] for k in pick], status[pick], cap=len(want) + 4096, entry="_tags", md=True, cs="long", de=True)[0] == want
    nb.close(); nf.close()


# ---- 2. the golden BAM through the one-pass pipeline, stored and coded, against the host-twin pipeline ---------------------------
def test_golden_bam_one_pass(ctx, tmp_path):
    bp, fa = os.path.join(DATA, "reads.bam"), os.path.join(DATA, "ref.fasta")
    probe = bam.NativeBam(bp)
    regions = [(n, 0, l - 1) for n, l in zip(probe.references, probe.lengths)]
    hdr = Hdr(probe.references, probe.lengths)
    probe.close()
    nf = bam.NativeFasta(fa)
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=regions, max_reads=0)
    try:
        one = bam.NativeBam(bp, one_pass=True)

        def run(name, cs="short", de=True, **kw):
            out = str(tmp_path / name)
            bam.create_bam_header(out, hdr)
            n, bad, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=4, r=30, out_format="bam", bai=out + ".bai", records="full",
                                               cs=cs, de=de, **kw)
            assert n == 10 and not bad
            return out
        host = None
        ctx.set("device_pack", 0)                                # the host twin makes the records
        try:
            host = run("host.bam")
        finally:
            ctx.set("device_pack", 1)
        want = record_stream(host)
        recs = split_records(want)
        assert len(recs) == 10
        for _, rec in recs:
            text, de, names = cc.new_tags_of(rec)
            assert names[-3:] == [b"NM", b"cs", b"de"] and names.count(b"cs") == 1 and names.count(b"de") == 1
            toks = cc.parse_cs(text)
            nm = int.from_bytes(mc.parse_tags(fc.parse_full(rec)[4])[-3][2], "little")
            assert sum(1 for s, _ in toks if s == "*") + sum(len(p) for s, p in toks if s in "+-") == nm
            assert 0.0 <= de < 1.0
        for name, kw in (("stored.bam", {}), ("match.bam", dict(compress="match"))):
            out = run(name, **kw)
            assert record_stream(out) == want, name               # the records decoded from the members
            members(out)
            check_index(out, out + ".bai")                        # the .bai walk finds every read
        assert open(str(tmp_path / "stored.bam"), "rb").read() == open(host, "rb").read()
        # the options hold for one run: the next one on a handle without them writes no cs and no de
        plain = split_records(record_stream(run("plain.bam", cs=None, de=False)))
        one.close()
        assert [cc.splice(p, b"csZ" + cc.new_tags_of(w)[0].encode() + b"\0def" + struct.pack("<f", cc.new_tags_of(w)[1]))
                for (_, p), (_, w) in zip(plain, recs)] == [w for _, w in recs]
        nf.close()
    finally:
        cfg.args = old


# ---- 3. the cs_len buffer grows between two calls on one context -----------------------------------------------------------------
def test_cs_len_grows_between_calls(ctx, tables, tmp_path):
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
        # 3 reads: cs_len holds 3 * 4 + 64 bytes and its head-room, fewer than the 120 * 4 + 64 the second call needs
        for lo, hi in ((0, 3), (0, 120)):
            out = str(tmp_path / f"grow{hi}.bam")
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            stb = nb.realign_file(own, nf, idx[lo:hi], out, batch_reads=1000, r=30, out_format="bam", bai=out + ".bai", records="full", md=True,
                                  cs="long", de=True)
            assert np.array_equal(stb, st[lo:hi])
            assert record_stream(out) == nb.format_bam_full(nf, idx[lo:hi], finals[lo:hi], st[lo:hi], md=True, cs="long", de=True), hi
            check_index(out, out + ".bai")
        nb.close(); nf.close()
    finally:
        cfg.args = old
        own.close()
