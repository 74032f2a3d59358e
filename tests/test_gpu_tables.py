"""GPU parity (-m gpu) under score tables other than the shipped ones (tests/table_families.py, G8
tests/golden/tables_variety.npz): strings AND status bits against the live oracle, and against the reference's own strings
where G8 holds them.  The fill's hot loop is the generated assembly (fill_step_asm.inc), not cell.hpp: these tables put
ties, negative entries, a scored N, non-smooth rows of long polymers, signed zeros / denormals / +inf entries and the
reference's INF = 100 regime through it, at every wave count 1 ... 16 of a chunk.  test_table_inputs_are_sensitive
(test_oracle_golden.py) checks that the input set reaches the lookups a mis-indexed kernel would get wrong.  Tables made
from a --stats_dir also go through the file pipeline (realign CLI, realign_file, the one-pass path)."""
import os

import numpy as np
import pytest

import oracle
import table_families as tf
from npore_amd import aln, cig

pytestmark = pytest.mark.gpu

FAMILY_SETS = ["random", "grid", "equal", "recalc", "ulp", "inf_boundary"]
SHAPE_SETS = ["random_6_100", "random_6_127", "random_4_20", "random_6_5", "random_3_31"]
# the r of test_kernel_shapes and test_bands_of_nine_to_sixteen_waves plus 1, 5, 330, 360 and 470: a chunk of
# ceil((2r + 1) / 64) waves (align_engine.hpp pick_shape) = 1 1 1 2 3 3 4 4 5 6 7 8 9 10 11 12 13 14 15 16, every count
BANDS = [1, 5, 30, 40, 70, 95, 96, 100, 140, 170, 200, 230, 256, 300, 330, 360, 384, 447, 470, 511]
MBRS = (20000, 333, 7)


def _inputs(max_l):
    reads = tf.input_set(max_l, int(tf.g8()["input/seed"][0]))
    return [x[0] for x in reads], [x[1] for x in reads], [x[2] for x in reads]


def _vs_oracle(c, t, refs, seqs, cigs, r, mbr, keep=None):
    """One batch on the device, every read (or those with keep(k)) against the oracle: strings and status bits."""
    sub, nps, ist, iex, max_n, max_l = t
    got, st = c.align_batch(refs, seqs, cigs, indel_start=ist, indel_extend=iex, r=r, max_b_rows=mbr, return_status=True)
    for k in range(len(refs)):
        if keep is None or keep(k):
            want, wst = oracle.align(refs[k], seqs[k], cigs[k], sub, nps, indel_start=ist, indel_extend=iex, r=r,
                                     max_b_rows=mbr, max_n=max_n, max_l=max_l, return_status=True)
            assert got[k] == want and st[k] == wst, (r, mbr, k, st[k], wst)
    return got, st


@pytest.mark.parametrize("name", FAMILY_SETS + SHAPE_SETS)
def test_table_set_vs_reference_and_oracle(name):
    """The G8 configurations against the reference's digests and the oracle; then every band width of BANDS (max_b_rows
    rotating through 20000 / 333 / 7; above r = 255 a third of the long reads, as the oracle's state matrix is slow to set
    up there) against the oracle."""
    t = tf.load(name)
    sub, nps, ist, iex, max_n, max_l = t
    refs, seqs, cigs = _inputs(max_l)
    c = aln.Context(sub, nps, max_n=max_n, max_l=max_l, device=0)
    try:
        for r, mbr in tf.g8()["input/configs"].tolist():
            got, _ = _vs_oracle(c, t, refs, seqs, cigs, r, mbr)
            assert tf.g8_check(name, got, r, mbr) >= len(refs) - 4
        assert sorted({-(-(2 * r + 1) // 64) for r in BANDS}) == list(range(1, 17))
        bands = BANDS if name in FAMILY_SETS else BANDS[::3]
        for i, r in enumerate(bands):
            mbr = MBRS[i % 3] if r < 256 or i % 3 else 1500
            _vs_oracle(c, t, refs, seqs, cigs, r, mbr, keep=(lambda k: k % 3 == 0 or len(refs[k]) < 3) if r > 255 else None)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["random", "grid", "inf_boundary"])
def test_chunking_and_packings(name):
    """max_b_rows 20000 / 333 / 7 at one band width each of one, four and eight waves, and forced chunks-per-workgroup
    packings (test_kernel_shapes' force_chunks): chunk borders, the first row / column path and the workgroup's shared
    tables under these tables."""
    t = tf.load(name)
    sub, nps, ist, iex, max_n, max_l = t
    refs, seqs, cigs = _inputs(max_l)
    for chunks, rs in ((0, (30, 100, 230)), (1, (100,)), (3, (100,)), (5, (30,))):
        c = aln.Context(sub, nps, max_n=max_n, max_l=max_l, device=0)
        try:
            c.set("force_chunks", chunks)
            for r in rs:
                for mbr in MBRS:
                    _vs_oracle(c, t, refs, seqs, cigs, r, mbr)
        finally:
            c.close()


@pytest.mark.parametrize("name", ["inf_boundary", "random", "ulp"])
def test_device_glue_under_table_families(name):
    """final_cigars=True (the glue on the device) == the host glue on the same raw strings, and == the Python glue on the
    oracle's strings; under inf_boundary the reference's truncated strings (status bit 4) are new input to the glue."""
    t = tf.load(name)
    sub, nps, ist, iex, max_n, max_l = t
    refs, seqs, cigs = _inputs(max_l)
    c = aln.Context(sub, nps, max_n=max_n, max_l=max_l, device=0)
    try:
        truncated = 0
        for r, mbr in ((30, 20000), (100, 333), (5, 7)):
            raw, st = _vs_oracle(c, t, refs, seqs, cigs, r, mbr)
            fin, st2 = c.align_batch(refs, seqs, cigs, indel_start=ist, indel_extend=iex, r=r, max_b_rows=mbr,
                                     return_status=True, final_cigars=True)
            assert (st == st2).all(), (r, mbr)
            assert fin == cig.standardize_batch(raw, refs, seqs), (r, mbr)
            for k in range(0, len(refs), 5):
                assert fin[k] == cig.collapse_cigar(cig.standardize(raw[k], refs[k], seqs[k])), (r, mbr, k)
            truncated += int((st & 4).astype(bool).sum())
        if name == "inf_boundary":
            assert truncated > 0
    finally:
        c.close()


def test_non_finite_penalties_refused_and_inf_entries_accepted():
    """Non-finite indel penalties are refused loudly (NPORE_E_INVALID) at every align entry; +inf table entries (the ulp
    set holds some) are accepted and give the oracle's strings (test_table_set_vs_reference_and_oracle[ulp])."""
    sub, nps, ist, iex, max_n, max_l = tf.load("ulp")
    assert np.isposinf(nps).any()
    c = aln.Context(sub, nps, max_n=max_n, max_l=max_l, device=0)
    try:
        refs, seqs, cigs = _inputs(max_l)
        for a, b in ((float("nan"), 1.0), (5.0, float("inf")), (float("-inf"), 1.0), (5.0, float("nan"))):
            for final in (False, True):
                with pytest.raises(aln.NporeError, match="must be finite"):
                    c.align_batch(refs[:3], seqs[:3], cigs[:3], indel_start=a, indel_extend=b, final_cigars=final)
        got = c.align_batch(refs[:3], seqs[:3], cigs[:3])       # the context still works
        assert got == [oracle.align(refs[k], seqs[k], cigs[k], sub, nps) for k in range(3)]
    finally:
        c.close()


def _sam_cigars(path):
    return {f[0]: f[5] for f in (l.rstrip("\n").split("\t") for l in open(path) if not l.startswith("@"))}


def test_stats_dir_through_the_file_pipeline(tmp_path):
    """Count matrices in a --stats_dir (the cms.json counts as {subs,nps,inss,dels}_cm.npy) through the file pipeline:
    `realign --stats_dir` in one pass and with the indexed reader, bam.realign_file and the one-pass realign_sequential
    (the npore_bam_realign_* entries, not npore_align_batch).  Every record's CIGAR == collapse(standardize(oracle.align))
    under calc_score_matrices of those counts -- which differ from the shipped tables' on all ten reads."""
    import argparse
    import subprocess
    import sys
    from conftest import GOLDEN, REPO, enc, expand_cigar, load_json
    from npore_amd import bam, cfg
    d = tmp_path / "stats"
    d.mkdir()
    for key, a in zip(("subs", "nps", "inss", "dels"), tf.cms_counts(6, 100)):
        np.save(str(d / f"{key}_cm.npy"), a)
    sub, nps, _, _ = aln.load_default_tables(str(d))
    assert sub.tobytes() == tf.g8()["recalc/sub"].tobytes() and nps.tobytes() == tf.g8()["recalc/np"].tobytes()
    fasta = "".join(l.strip() for l in open(os.path.join(GOLDEN, "data", "ref.fasta")) if not l.startswith(">")).upper()
    shipped = {x["name"]: x["final_cigar"] for x in load_json("reads_e2e.json")}
    want = {}
    for line in open(os.path.join(GOLDEN, "data", "reads.sam")):
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        ex = expand_cigar(f[5]).replace("S", "").replace("H", "")
        start, rlen = int(f[3]) - 1, sum(1 for ch in expand_cigar(f[5]) if ch in "XD=M")
        ref, seq = enc(fasta[start:start + rlen]), enc(f[9])
        want[f[0]] = cig.collapse_cigar(cig.standardize(oracle.align(ref, seq, ex, sub, nps), ref, seq))
    assert len(want) == 10 and all(want[k] != shipped[k] for k in want)

    bam_path, ref_path = os.path.join(GOLDEN, "data", "reads.bam"), os.path.join(GOLDEN, "data", "ref.fasta")
    for tag, env in (("one_pass", {}), ("indexed", {"NPORE_BAM_ONE_PASS": "0"})):
        prefix = str(tmp_path / tag)
        subprocess.check_call([sys.executable, "-m", "npore_amd.realign", "--bam", bam_path, "--ref", ref_path,
                               "--out_prefix", prefix, "--stats_dir", str(d)], cwd=REPO, env=dict(os.environ, **env))
        assert _sam_cigars(prefix + ".sam") == want, tag

    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=[("ref", 0, 1000)], max_reads=0)
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    try:
        nf = bam.NativeFasta(ref_path)
        nb = bam.NativeBam(bam_path)
        idx = nb.select(cfg.args.regions)
        assert len(idx) == 10
        st = nb.realign_file(c, nf, idx, str(tmp_path / "file.sam"), batch_reads=3, r=30)
        assert not st.any() and _sam_cigars(str(tmp_path / "file.sam")) == want
        # non-finite penalties are refused by the file pipeline too, and nothing is written
        with pytest.raises(RuntimeError, match="must be finite"):
            nb.realign_file(c, nf, idx, str(tmp_path / "nan.sam"), batch_reads=3, r=30, indel_start=float("nan"))
        assert not os.path.exists(tmp_path / "nan.sam") or not _sam_cigars(str(tmp_path / "nan.sam"))
        nb.close()
        one = bam.NativeBam(bam_path, one_pass=True)
        n, bad, _ = one.realign_sequential(c, nf, cfg.args.regions, str(tmp_path / "seq.sam"), batch_reads=4, r=30)
        assert n == 10 and not bad and _sam_cigars(str(tmp_path / "seq.sam")) == want
        one.close()
        nf.close()
    finally:
        c.close()
        cfg.args = old
