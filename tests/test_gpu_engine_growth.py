"""Work buffers that must grow between the groups of a call and between the calls of one context, in every output mode of
the align engine (csrc/align_engine.hpp: op strings, final text in slots, compacted text, BAM records built on the
device), and contexts made and destroyed in a row.  A context that has grown gives what a fresh one gives.
"""
import argparse

import numpy as np
import pytest

import oracle
from npore_amd import aln, bam, cfg, synth
from test_bam_out import Hdr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def large():
    return synth.make_batch(55, 40, ref_len=2500)


@pytest.fixture(scope="module")
def small():
    return synth.make_batch(56, 3, ref_len=300)


def fresh(tables):
    sub, nps = tables
    return aln.Context(sub, nps, max_n=6, max_l=100, device=0)


# ---- 1. growth through align_batch ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large_want(tables, large):
    """(r, final_cigars) -> what a fresh context gives for the large batch alone under the default budget"""
    c = fresh(tables)
    want = {(r, fin): c.align_batch(*large, r=r, return_status=True, final_cigars=fin) for r, fin in ((30, False), (30, True), (100, False))}
    c.close()
    return want


def test_growth_through_align_batch(tables, small, large, large_want):
    """3 short reads first, then 40 reads of 2.5 kb under an 8 MB traceback budget: about 5 reads per group, so at least 8
    groups through the 3 work sets, every set regrown; then r = 100 (four waves per chunk, wider traceback rows)."""
    sub, nps = tables
    c = fresh(tables)
    got, st = c.align_batch(*small, r=30, return_status=True)
    assert not st.any() and len(got) == 3
    c.set("tb_budget_mb", 8)
    for r, fin in ((30, False), (30, True), (100, False)):
        got, st = c.align_batch(*large, r=r, return_status=True, final_cigars=fin)
        want, want_st = large_want[(r, fin)]
        assert np.array_equal(st, want_st) and not st.any(), (r, fin)
        assert got == want, (r, fin)
        assert c.timing()["launches"] >= 4, (r, fin)
        if not fin:
            refs, seqs, cigs = large
            for k in (0, 39):
                assert got[k] == oracle.align(refs[k], seqs[k], cigs[k], sub, nps, r=r), (r, k)
    c.close()


# ---- 2. growth through the file pipeline ----------------------------------------------------------------------------------
def write_inputs(tmp, name, batch):
    """The reads of a synth batch on one contig, 20 random bases between them: BAM + FASTA"""
    rng = np.random.default_rng(9)
    dec = lambda a: "".join("NACGT"[x] for x in a)
    contig, recs = [], []
    for k, (rf, sq, cg) in enumerate(zip(*batch)):
        pos = len(contig) + 20
        contig += ["ACGT"[x] for x in rng.integers(0, 4, 20)] + list(dec(rf))
        cg = cg if isinstance(cg, str) else bytes(cg).decode()
        runs = []
        for ch in cg:
            if runs and runs[-1][0] == ch:
                runs[-1][1] += 1
            else:
                runs.append([ch, 1])
        recs.append(dict(name=f"{name}{k}", flag=16 if k % 4 == 1 else 0, ref_id=0, pos=pos, mapq=30,
                         cigar=[("MIDNSHP=XB".index(ch), n) for ch, n in runs], seq=dec(sq),
                         qual=None if k % 5 == 0 else bytes(rng.integers(0, 60, len(sq)).tolist()), hp=k % 3))
    contig = "".join(contig) + "ACGT" * 10
    bp, fa = str(tmp / f"{name}.bam"), str(tmp / f"{name}.fa")
    open(fa, "w").write(">ctg\n" + contig + "\n")
    bam.write_bam(bp, [("ctg", len(contig))], recs)
    return bp, fa, len(contig)


def test_growth_through_file_pipeline(tables, large, tmp_path):
    """A 5-read file, then a 40-read file in batches of 12 under a 2 MB budget (every batch in several groups), on one
    context: the files and status arrays of a fresh context that ran the large file alone.  As SAM (compacted texts)
    and as BAM (records built on the device)."""
    refs, seqs, cigs = large
    files = {"few": write_inputs(tmp_path, "few", (refs[:5], seqs[:5], cigs[:5])), "many": write_inputs(tmp_path, "many", large)}
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=None, max_reads=0)
    try:
        def run(c, which, fmt, tag, **kw):
            bp, fa, clen = files[which]
            nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
            idx = nb.select([("ctg", 0, clen - 1)])
            assert len(idx) == (5 if which == "few" else 40)
            out = str(tmp_path / f"{tag}_{which}.{fmt}")
            if fmt == "bam":
                bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            st = nb.realign_file(c, nf, idx, out, r=30, out_format=fmt, bai=out + ".bai" if fmt == "bam" else None, **kw)
            nb.close(); nf.close()
            return open(out, "rb").read(), st

        for fmt in ("sam", "bam"):
            c = fresh(tables)
            want, want_st = run(c, "many", fmt, "alone")
            c.close()
            c = fresh(tables)
            few, few_st = run(c, "few", fmt, "grown")
            assert len(few) > 0 and not few_st.any()
            c.set("tb_budget_mb", 2)
            got, st = run(c, "many", fmt, "grown", batch_reads=12)
            c.close()
            assert np.array_equal(st, want_st) and not st.any(), fmt
            assert got == want, fmt
    finally:
        cfg.args = old


# ---- 3. context lifetime --------------------------------------------------------------------------------------------------
def test_contexts_in_a_row(tables, small, tmp_path):
    """Make, use (a batch and a file run) and close a context three times in one process, close one that was never used,
    and an annotation-only one after get_np_info: nothing raises and every round gives the same."""
    refs, seqs, cigs = small
    bp, fa, clen = write_inputs(tmp_path, "life", small)
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=None, max_reads=0)
    try:
        rounds = []
        for k in range(3):
            c = fresh(tables)
            got, st = c.align_batch(refs, seqs, cigs, r=30, return_status=True)
            nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
            out = tmp_path / f"life{k}.sam"
            fst = nb.realign_file(c, nf, nb.select([("ctg", 0, clen - 1)]), str(out), r=30)
            nb.close(); nf.close()
            c.close()
            rounds.append((got, st.tolist(), out.read_bytes(), fst.tolist()))
        assert rounds[0] == rounds[1] == rounds[2]
        assert len(rounds[0][0]) == 3 and not any(rounds[0][1]) and rounds[0][2].count(b"\n") == 3
        fresh(tables).close()
        c = aln.Context(None, None, max_n=6, max_l=100, device=0)
        info = c.get_np_info(seqs[0])
        assert info.shape == (len(seqs[0]), 2, 6)
        c.close()
    finally:
        cfg.args = old
