"""Pins oracle/ (plain-C restatement) to golden vectors produced by the
reference's own compiled Cython code (tests/golden/make_golden.py).  CPU only."""
import hashlib
import os

import numpy as np
import pytest

import oracle
from npore_amd import synth
from conftest import load_json, enc, expand_cigar, collapse_cigar, GOLDEN


def sha(s):
    return hashlib.sha256(s.encode()).hexdigest()


def test_np_info_golden():
    seqs = load_json("np_info_seqs.json")
    z = np.load(os.path.join(GOLDEN, "np_info.npz"))
    for i, s in enumerate(seqs):
        got = oracle.get_np_info(enc(s))
        assert got.shape == z[f"info_{i}"].shape
        assert np.array_equal(got, z[f"info_{i}"]), (i, s)


def test_np_info_docstring_example():
    # reference src/aln.pyx:182-194
    info = oracle.get_np_info(enc("ATATATATTTTTTAAAGCGCGC"))
    assert info[:, 0, 0].tolist() == [0, 0, 0, 0, 0, 0, 0, 6, 6, 6, 6, 6, 6, 3, 3, 3, 0, 0, 0, 0, 0, 0]
    assert info[:, 1, 0].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 0, 1, 2, 0, 0, 0, 0, 0, 0]
    assert info[:, 0, 1].tolist() == [4, 3, 4, 3, 4, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 3, 0, 3, 0]
    assert info[:, 1, 1].tolist() == [0, 0, 1, 1, 2, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 0]
    assert not info[:, :, 2].any()


def test_unit_aligns(tables):
    sub, nps = tables
    for c in load_json("unit_aligns.json"):
        ex = expand_cigar(c["cigar"])
        a = oracle.align(enc(c["ref"]), enc(c["seq"]), ex, sub, nps, max_b_rows=20, r=10)
        b = oracle.align(enc(c["ref"]), enc(c["seq"]), ex, sub, nps)
        assert a == c["aln_20_10"], c
        assert b == c["aln_default"], c
        assert collapse_cigar(a) == c["collapsed_20_10"]


def test_reads_e2e_raw(tables):
    sub, nps = tables
    fasta = "".join(l.strip() for l in open(os.path.join(GOLDEN, "data", "ref.fasta")) if not l.startswith(">")).upper()
    want = {r["name"]: r for r in load_json("reads_e2e.json")}
    n = 0
    for line in open(os.path.join(GOLDEN, "data", "reads.sam")):
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        ex = expand_cigar(f[5]).replace("S", "").replace("H", "")
        start = int(f[3]) - 1
        rlen = sum(1 for ch in ex if ch in "XD=M")
        got, st = oracle.align(enc(fasta[start:start + rlen]), enc(f[9]), ex, sub, nps, return_status=True)
        assert st == 0
        assert got == want[f[0]]["raw_align"], f[0]
        n += 1
    assert n == 10


@pytest.mark.parametrize("big", [False, True])
def test_synthetic(tables, big):
    sub, nps = tables
    recs = [r for r in load_json("synthetic.json") if (r["ref_len"] >= 10_000) == big]
    assert recs
    for r in recs:
        ref, seq, cig = synth.make_pair(r["base_seed"], r["index"], r["ref_len"], r["p_np"], r["p_cnv"], r["mixed"])
        got, st = oracle.align(ref, seq, cig, sub, nps, max_b_rows=r["max_b_rows"], r=r["r"], return_status=True)
        assert st == 0
        assert len(got) == r["len"] and sha(got) == r["sha256"], r
        if "collapsed" in r:
            assert collapse_cigar(got) == r["collapsed"]


def test_edge_inputs(tables):
    sub, nps = tables
    assert oracle.align(enc(""), enc(""), "", sub, nps) == ""
    assert oracle.align(enc("ACGT"), enc(""), "DDDD", sub, nps) == "DDDD"
    assert oracle.align(enc(""), enc("ACGT"), "IIII", sub, nps) == "IIII"
    with pytest.raises(ValueError):
        oracle.align(enc("ACGT"), enc("ACGT"), "===", sub, nps)      # lengths disagree
    with pytest.raises(ValueError):
        oracle.align(enc("ACGT"), enc("ACGT"), "==N=", sub, nps)     # unsupported op


def test_fullsize_digests_are_the_oracles(tables):
    """tests/golden/fullsize_digests.npz (per-read length + sha256[:16] of every full-size configuration, which the GPU
    tests compare all reads against) really is what the pinned oracle gives: spot checks of each configuration."""
    import hashlib
    from npore_amd import synth
    sub, nps = tables
    z = np.load(os.path.join(GOLDEN, "fullsize_digests.npz"))
    # (round 5: c2 / r30 cover what the ranks of an 8-GPU run hold -- indices 0 ... 7 999, and 0 ... 31 999 sampled; c4 is new)
    assert [len(z[k + "_idx"]) for k in ("c2", "r30", "c5", "c3", "c4")] == [8000, 8000, 256, 19000, 17822]
    for name, seed, ref_len, mixed, r, i in (("c2", 2, 10_000, False, 100, 511), ("c2", 2, 10_000, False, 100, 7_777),
                                             ("r30", 2, 10_000, False, 30, 2048), ("r30", 2, 10_000, False, 30, 4000 + 7 * 3999),
                                             ("c3", 3, 10_000, True, 100, 99_990), ("c3", 3, 10_000, True, 100, 4_321),
                                             ("c4", 4, 10_000, True, 100, 7_001), ("c4", 4, 10_000, True, 100, 8000 + 101 * 9821)):
        ref, seq, cig = synth.make_pair(seed, i, ref_len, mixed=mixed)
        s = oracle.align(ref, seq, cig, sub, nps, r=r)
        k = int(np.nonzero(z[name + "_idx"] == i)[0][0])
        assert len(s) == z[name + "_len"][k] and int(hashlib.sha256(s.encode()).hexdigest()[:16], 16) == int(z[name + "_dig"][k])


# ---- G8 (tests/golden/make_golden_tables.py): score tables other than the shipped ones

def _g8_sets():
    import table_families as tf
    return list(tf.TABLE_SETS)


@pytest.mark.parametrize("name", _g8_sets())
def test_oracle_vs_reference_table_families(name):
    """oracle == the reference's compiled align() under every G8 table set (random entries with N scored, grids of ties,
    all-equal, calc_score_matrices of sparse counts, G1 moved by ulps with signed zeros / denormals / +inf entries,
    penalties at the reference's INF = 100, other max_n / max_l), on the input set of the GPU test."""
    import table_families as tf
    sub, nps, ist, iex, max_n, max_l = tf.load(name)
    reads = tf.input_set(max_l, int(tf.g8()["input/seed"][0]))
    n = 0
    for r, mbr in tf.g8()["input/configs"].tolist():
        got = [oracle.align(ref, seq, cig, sub, nps, indel_start=ist, indel_extend=iex, max_b_rows=mbr, r=r,
                            max_n=max_n, max_l=max_l) for ref, seq, cig, _ in reads]
        n += tf.g8_check(name, got, r, mbr)
    assert n >= 7 * (len(reads) - 4)


def test_calc_score_matrices_sparse_counts():
    """aln.calc_score_matrices == the reference's, bit for bit, on the sparse counts of cms.json (what --recalc_cms over a
    small region hands the kernel: mostly eps plus fix_matrix_properties' ramps); G1 pins only the shipped counts."""
    import table_families as tf
    from npore_amd import aln
    z = tf.g8()
    sub, nps, ins, dels = aln.calc_score_matrices(*tf.cms_counts(6, 100))
    for got, key in ((sub, "recalc/sub"), (nps, "recalc/np"), (ins, "recalc/ins"), (dels, "recalc/del")):
        want = z[key]
        assert got.dtype == np.float32 and got.shape == want.shape, key
        assert got.tobytes() == want.tobytes(), (key, np.argwhere(got != want)[:4])


SENSITIVITY_MIN = 3


def test_table_inputs_are_sensitive():
    """What makes tests/test_gpu_tables.py fail on a subtly wrong kernel: on its input set, under the `random` table set,
    every table lookup a mis-indexed kernel could get wrong changes the strings of at least SENSITIVITY_MIN reads (so no
    single tie-breaking read carries a lookup) -- in at least one of the two band widths the GPU test runs them at.
    Under G1 (the shipped tables) zeroing the N row or column changes nothing: they are 0 already, the value the device's
    LDS table puts in its unused slots."""
    import table_families as tf
    sub, nps, ist, iex, max_n, max_l = tf.load("random")
    reads = [x for x in tf.input_set(max_l, int(tf.g8()["input/seed"][0]))]

    def run(s, t, a=ist, b=iex, r=30, mbr=333):
        return [oracle.align(ref, seq, cig, s, t, indel_start=a, indel_extend=b, max_b_rows=mbr, r=r, max_n=max_n,
                             max_l=max_l) for ref, seq, cig, _ in reads]

    base = {r: run(sub, nps, r=r) for r in (5, 30)}

    def changed(s=sub, t=nps, a=ist, b=iex):
        return max(sum(x != y for x, y in zip(base[r], run(s, t, a, b, r=r))) for r in (5, 30))

    def with_np(fn):
        t = nps.copy(); fn(t); return t

    def with_sub(fn):
        s = sub.copy(); fn(s); return s

    big = np.zeros(nps.shape, bool)
    big[:, 32:, :] = True; big[:, :, 32:] = True
    shifted = np.concatenate([nps[:, :, 1:], nps[:, :, -1:]], axis=2)
    corruptions = {
        "sub transposed": changed(s=np.ascontiguousarray(sub.T)),
        "sub N row zeroed": changed(s=with_sub(lambda s: s.__setitem__(0, 0))),
        "sub N column zeroed": changed(s=with_sub(lambda s: s.__setitem__((slice(None), 0), 0))),
        "np call index + 1": changed(t=with_np(lambda t: t.__setitem__((slice(None), slice(None), slice(0, -1)), nps[:, :, 1:]))),
        "np L index + 1": changed(t=with_np(lambda t: t.__setitem__((slice(None), slice(0, -1)), nps[:, 1:]))),
        "np period rolled": changed(t=np.ascontiguousarray(np.roll(nps, 1, axis=0))),
        "np L or call >= 32 shifted": changed(t=np.where(big, shifted, nps).astype(np.float32)),
        "np clamp row max_l - 1 = its neighbour": changed(t=with_np(lambda t: t.__setitem__((slice(None), max_l - 1), nps[:, max_l - 2]))),
        "indel_start and indel_extend swapped": changed(a=iex, b=ist),
    }
    weak = {k: v for k, v in corruptions.items() if v < SENSITIVITY_MIN}
    assert not weak, (weak, corruptions)
