"""The output half of the file pipeline -- traceback runs -> final CIGAR -> BAM records -> BGZF members -- on inputs above
its kernels' size thresholds (tests/output_edge_cases.py states each threshold next to the constant it comes from;
tests/test_output_edge_cases.py shows on the CPU that the inputs cross them):

  * WaveProbe (standardize_kernel, standardize_words_kernel): indel runs that slide 63 ... 600 positions, two to ten rounds
    of 64, ending on a differing base and on a used-up match run, for D and for I;
  * place_deflate_kernel with 2 and 3 members per thread and empty threads, plan_* / emit_* beyond member 256;
  * wave_copy<NIB> at every (destination, source) alignment and every length class: fewer bytes than the head, no whole
    word, no tail bytes, 64 and 65 words.

Every expectation is the oracle's or a host twin's (cig.standardize_batch, npore_bam_format_bam, npore_bam_write_file,
npore_debug_deflate_member_mode); bytes and strings are compared exactly."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest

import oracle
import output_edge_cases as oc
from npore_amd import aln, bam, cfg, cig
from conftest import REPO
from test_bam_deflate import host_member
from test_bam_out import Hdr, check_index, make_bam, members
from test_gpu_bam_match import device_members, mixed_buffer, want_member
from test_gpu_bam_out import record_stream, sam_records

pytestmark = pytest.mark.gpu
P = oc.P


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


class _Args:
    """cfg.args as the library's file entries expect them, for the time of a test"""

    def __init__(self, regions):
        self.regions = regions

    def __enter__(self):
        self.old = cfg.args
        cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=self.regions, max_reads=0)

    def __exit__(self, *exc):
        cfg.args = self.old


def _same_files(out, want):
    assert open(out, "rb").read() == open(want, "rb").read(), out
    assert open(out + ".bai", "rb").read() == open(want + ".bai", "rb").read(), out


def _finals_of(sam_path, st):
    it = iter(sam_records(sam_path))
    return ["" if s_ & 32 else next(it).split("\t")[5] for s_ in st]


# ---- 1. slides of 64 positions and more ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _slide_cases():
    return oc.slide_cases()


_oracle_strings = {}


def _oracle(tables, r, mbr):
    """(raw strings, status bits, final CIGARs by the Python statement) of the oracle for every slide case: computed once"""
    if (r, mbr) not in _oracle_strings:
        sub, nps = tables
        refs, seqs, cigs, _ = _slide_cases()
        res = [oracle.align(refs[k], seqs[k], cigs[k], sub, nps, r=r, max_b_rows=mbr, return_status=True) for k in range(len(refs))]
        finals = ["".join(f"{n}{c}" for c, n in cig.standardize_runs(raw, refs[k], seqs[k])) for k, (raw, _) in enumerate(res)]
        _oracle_strings[(r, mbr)] = [raw for raw, _ in res], np.array([s_ for _, s_ in res], np.int32), finals
    return _oracle_strings[(r, mbr)]


@pytest.mark.parametrize("r,mbr", oc.SLIDE_CONTEXTS)
def test_final_cigars_of_long_slides(ctx, tables, r, mbr):
    """standardize_kernel: one align_batch call per context; the texts equal the host glue on the same context's raw strings
    and the Python statement on the oracle's, read by read"""
    refs, seqs, cigs, labels = _slide_cases()
    raw, st = ctx.align_batch(refs, seqs, cigs, r=r, max_b_rows=mbr, return_status=True)
    fin, st2 = ctx.align_batch(refs, seqs, cigs, r=r, max_b_rows=mbr, return_status=True, final_cigars=True)
    want_raw, want_st, want_fin = _oracle(tables, r, mbr)
    assert np.array_equal(st, st2) and np.array_equal(st, want_st), (r, mbr)
    host = cig.standardize_batch(raw, refs, seqs)
    for k in range(len(refs)):
        assert raw[k] == want_raw[k], (r, mbr, labels[k])
        assert fin[k] == host[k] == want_fin[k], (r, mbr, labels[k], want_raw[k])


@pytest.fixture(scope="module")
def slide_files(tmp_path_factory):
    """the slide cases as a BAM on one contig (each read's reference between gaps of 10 bases) and its FASTA"""
    refs, seqs, cigs, labels = _slide_cases()
    rng = np.random.default_rng(7)
    contig, recs = [], []
    for k, (ref, seq, ops) in enumerate(zip(refs, seqs, cigs)):
        contig.append(rng.integers(1, 5, 10).astype(np.uint8))
        pos = sum(map(len, contig))
        contig.append(ref)
        runs = [("=ID".index(c), n) for n, c in cig.collapse_cigar(ops, return_groups=True)]
        recs.append(dict(name=f"s{k}", flag=0, ref_id=0, pos=pos, mapq=60, cigar=[((7, 1, 2)[op], n) for op, n in runs],
                         seq="".join("NACGT"[x] for x in seq), qual=bytes([30 + k % 10]) * len(seq), hp=k % 3))
    contig.append(rng.integers(1, 5, 40).astype(np.uint8))
    text = "".join("NACGT"[x] for x in np.concatenate(contig))
    d = tmp_path_factory.mktemp("slides")
    (d / "c.fa").write_text(">ctg\n" + text + "\n")
    make_bam(str(d / "s.bam"), [("ctg", len(text))], recs)
    return d, str(d / "s.bam"), str(d / "c.fa"), len(text), len(recs)


def test_cigar_words_of_long_slides(ctx, tables, slide_files):
    """standardize_words_kernel: the same reads through the file pipeline at r = 30, max_b_rows = 333.  The SAM route's CIGAR
    column is align_batch's and the oracle's final text; the BAM route's record stream is the host twin's of those."""
    d, bp, fa, clen, n = slide_files
    refs, seqs, cigs, labels = _slide_cases()
    regions = [("ctg", 0, clen - 1)]
    with _Args(regions):
        nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
        idx = nb.select(regions)
        assert len(idx) == n == len(refs)
        sam = str(d / "route.sam")
        st = nb.realign_file(ctx, nf, idx, sam, batch_reads=400, r=30, max_b_rows=333)
        finals = _finals_of(sam, st)
        fin, st_b = ctx.align_batch(refs, seqs, cigs, r=30, max_b_rows=333, return_status=True, final_cigars=True)
        want_raw, want_st, want_fin = _oracle(tables, 30, 333)
        assert np.array_equal(st, st_b) and np.array_equal(st, want_st) and not (st & 32).any()
        assert finals == fin == want_fin
        out = str(d / "dev.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        stb = nb.realign_file(ctx, nf, idx, out, batch_reads=400, r=30, max_b_rows=333, out_format="bam", bai=out + ".bai")
        assert np.array_equal(stb, st)
        assert record_stream(out) == nb.format_bam(idx, finals, st)
        check_index(out, out + ".bai")
        nb.close(); nf.close()


# ---- 2. more than 256 members ----------------------------------------------------------------------------------------------
_huffman = {}


@functools.lru_cache(maxsize=None)
def _buffer(n):
    return mixed_buffer(n)


def _twin(payload, mode):
    if mode == 2:
        return want_member(payload)
    if payload not in _huffman:
        _huffman[payload] = host_member(payload)
    return _huffman[payload]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,phase,n_members", [c[:3] for c in oc.MEMBER_CASES])
def test_more_members_than_threads_place_them(ctx, n, phase, n_members, mode):
    """257, 513 and 599 members of every form side by side: count, fragments, stream position, and every member byte for
    byte against the host twin (its place follows from the sizes of all members before it: device_members cuts the
    output by the sizes, and asserts that they sum to info[1])"""
    data = _buffer(n)
    mem, head, tail, pos = device_members(ctx, data, phase, mode=mode)
    want_head, want_n, want_tail = oc.member_cuts(n, phase)
    assert (len(head), len(mem), len(tail)) == (want_head, want_n, want_tail) and want_n == n_members
    assert head == data[:want_head] and tail == data[n - want_tail:]
    assert pos == phase + n
    forms = set()
    for k, m in enumerate(mem):
        payload = data[want_head + k * P:want_head + (k + 1) * P]
        want = _twin(payload, mode)
        assert m == want, (k, len(m), len(want))
        forms.add("stored" if len(m) == P + 31 else "coded")
    assert forms == {"stored", "coded"}


@pytest.fixture(scope="module")
def reads_1200(tmp_path_factory):
    """PIPELINE_READS reads of 10 kb on one contig (the benchmark's generator): about 18 MB of records"""
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import bench_realign
    tmp = tmp_path_factory.mktemp("members")
    bp, fa, clen = bench_realign.build_inputs(str(tmp), oc.PIPELINE_READS, 0, 10000, 37, procs=4)
    bam.write_bai(bp)
    return tmp, bp, fa, clen


def test_file_pipeline_with_more_than_256_members_in_a_batch(ctx, reads_1200):
    """1 200 reads of 10 kb in ONE batch with --bam_compress huffman: the batch's members are more than the placement's
    threads (the input builds in one to three seconds with four worker processes, so the count is not reduced)"""
    tmp, src, fa, clen = reads_1200
    n = oc.PIPELINE_READS
    regions = [("ctg", 0, clen - 1)]
    with _Args(regions):
        nb, nf = bam.NativeBam(src), bam.NativeFasta(fa)
        idx = nb.select(regions)
        assert len(idx) == n
        sam = str(tmp / "route.sam")
        st = nb.realign_file(ctx, nf, idx, sam, batch_reads=n, r=30)
        finals = _finals_of(sam, st)
        want = str(tmp / "want.bam")
        bam.create_bam_header(want, Hdr(nb.references, nb.lengths))
        nb.write_file(idx, finals, st, want, batch_reads=n, bai=want + ".bai", compress="huffman")
        coded = sum(1 for m in members(want) if len(m[1]) == P and not m[2])
        assert coded > oc.PLACE_THREADS, coded
        out = str(tmp / "dev.bam")
        bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
        stb = nb.realign_file(ctx, nf, idx, out, batch_reads=n, r=30, out_format="bam", bai=out + ".bai", compress="huffman")
        assert np.array_equal(stb, st)
        _same_files(out, want)
        nb.close(); nf.close()


# ---- 3. wave_copy by alignment and length class -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def copy_files(tmp_path_factory):
    references, contig, records, pairs = oc.copy_records()
    d = tmp_path_factory.mktemp("copies")
    (d / "c.fa").write_text(">" + oc.COPY_CONTIG + "\n" + contig + "\n")
    make_bam(str(d / "s.bam"), references, records)
    return d, str(d / "s.bam"), str(d / "c.fa"), len(contig), records, pairs


def test_records_of_every_copy_alignment(ctx, tables, copy_files):
    """reads of 1 ... 521 bases behind names of 1 ... 4 letters and clips of 0 ... 7 bases: the file equals the host twin's of
    the SAM route's final CIGARs (which are the oracle's), in batches of 5 and in one batch, and with Huffman-coded members,
    whose fragments go through wave_copy too"""
    d, bp, fa, clen, records, pairs = copy_files
    sub, nps = tables
    regions = [(oc.COPY_CONTIG, 0, clen - 1)]
    with _Args(regions):
        nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
        idx = nb.select(regions)
        assert len(idx) == len(records)
        sam = str(d / "route.sam")
        st = nb.realign_file(ctx, nf, idx, sam, batch_reads=5, r=30)
        assert not st.any()
        finals = _finals_of(sam, st)
        for k, (ref, seq, ops) in enumerate(pairs):
            raw = oracle.align(ref, seq, ops, sub, nps, r=30)
            assert finals[k] == cig.collapse_cigar(cig.standardize(raw, ref, seq)), (k, records[k]["name"])
        want, want_h = str(d / "want.bam"), str(d / "want_h.bam")
        for path, mode in ((want, "none"), (want_h, "huffman")):
            bam.create_bam_header(path, Hdr(nb.references, nb.lengths))
            nb.write_file(idx, finals, st, path, batch_reads=5, bai=path + ".bai", compress=mode)
        assert record_stream(want) == record_stream(want_h) == nb.format_bam(idx, finals, st)
        for name, batch_reads, mode, path in (("b5.bam", 5, "none", want), ("b1000.bam", 1000, "none", want), ("h5.bam", 5, "huffman", want_h)):
            out = str(d / name)
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            stb = nb.realign_file(ctx, nf, idx, out, batch_reads=batch_reads, r=30, out_format="bam", bai=out + ".bai", compress=mode)
            assert np.array_equal(stb, st), name
            _same_files(out, path)
        check_index(str(d / "b5.bam"), str(d / "b5.bam.bai"))
        nb.close(); nf.close()
