"""Pass-through (--pass_through) on the GPU, on the file of tests/bam_pass_cases.py: the device side of a record that passes
(csrc/bam_emit_kernels.hpp: skipped by the unpack and tag kernels, placed by its own size, copied by one wave) against the host
twin npore_bam_format_bam_full_pass; then file to file through the one-pass pipeline, the indexed reader and the host-pack /
host-glue route -- their record streams equal to each other and to the composition the rule owes (the input's bytes for a
record that passes, the host twin's FULL record for a read), at batch_reads 4 (a batch with no read to align) and 4 000, with
stored, Huffman-coded and match-coded members; the written index, the status bits, the ranks' shares and mask 0.
"""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

from npore_amd import aln, bam, cfg
from test_bam_out import Hdr, check_index, header_len, members, split_records
import bam_full_cases as fc
import bam_pass_cases as pc
import long_cigar_cases as lc
from full_record_driver import device_full

pytestmark = pytest.mark.gpu
MASK = 0x904
TAGS = dict(md=True, cs="short", de=True)


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


def record_stream(path, header=True):
    if os.path.getsize(path) == 0:
        return b""
    data = bam._bgzf_decompress(path)
    return data[header_len(data):] if header else data


@pytest.fixture(scope="module")
def case(ctx, tmp_path_factory):
    """The file, its handles, and ONE reference for every test: the reads' final CIGARs and status from a SAM run of the reads
    alone, the host twin's FULL records of them (MD, cs, de), and the stream a pass-through run owes."""
    tmp = tmp_path_factory.mktemp("gpu_pass")
    references, refs, records = pc.pass_file()
    bp, fa = str(tmp / "p.bam"), str(tmp / "p.fa")
    pc.write_bam(bp, references, records)
    lc.write_fasta(fa, refs)
    bam.write_bai(bp)
    raws, flags = fc.input_records(bp), [r["flag"] for r in records]
    regions = [(n, 0, l) for n, l in references]
    old = cfg.args
    cfg.args = argparse.Namespace(max_n=6, max_l=100, regions=regions, max_reads=0)
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    reads = nb.select(regions)
    assert reads.tolist() == [k for k in range(40) if not pc.passes(flags[k], MASK)]
    sam = tmp / "reads.sam"
    st = nb.realign_file(ctx, nf, reads, str(sam), batch_reads=7, r=30)
    assert [int(reads[k]) for k in np.nonzero(st)[0]] == [12] and st[np.nonzero(st)[0][0]] == 32
    it = iter(sam.read_text().splitlines())
    finals = ["" if s & 32 else next(it).split("\t")[5] for s in st]
    rest = [r for _, r in split_records(nb.format_bam_full(nf, reads, finals, st, **TAGS))]
    idx = nb.select(regions, pass_mask=MASK)
    assert idx.tolist() == list(range(40))
    want = b"".join(pc.compose(raws, flags, MASK, idx.tolist(), {12}, rest))
    want_st = np.full(40, pc.ST_PASSED, np.int32)
    want_st[reads] = st
    yield dict(tmp=tmp, references=references, records=records, raws=raws, flags=flags, regions=regions, nb=nb, nf=nf, bp=bp, reads=reads,
               st=st, finals=finals, idx=idx, want=want, want_st=want_st)
    nb.close(); nf.close()
    cfg.args = old


# ---- 1. the device against the host twin -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [0x904, 0x100, 0x800, 0x4, 0])
def test_device_equals_host_twin(ctx, case, mask):
    nb, nf, flags = case["nb"], case["nf"], case["flags"]
    idx = np.array(pc.py_select(case["raws"], [(0, 0, 1 << 28), (1, 0, 1 << 28)], 0, mask), np.int64)
    final_of = dict(zip(case["reads"].tolist(), case["finals"]))
    st_of = dict(zip(case["reads"].tolist(), case["st"].tolist()))
    finals = [final_of.get(int(k), "") for k in idx]
    status = np.array([st_of.get(int(k), 0) for k in idx], np.int32)
    for kw in (dict(), dict(md=True), TAGS):
        want = nb.format_bam_full(nf, idx, finals, status, pass_mask=mask, **kw)
        got, nm, mdl = device_full(ctx, nb, nf, idx, finals, status, mask=mask, **kw)
        assert got == want, (mask, kw)
        for k, i in enumerate(idx):
            if pc.passes(flags[i], mask):
                assert nm[k] == 0 and (not kw.get("md") or mdl[k] == 0), (mask, i)
        if mask == 0:
            assert got == nb.format_bam_full(nf, idx, finals, status, **kw)
    if mask == MASK:
        assert nb.format_bam_full(nf, idx, finals, status, pass_mask=mask, **TAGS) == case["want"]


# ---- 2. file to file: three routes, one stream ---------------------------------------------------------------------------------
def run_routes(ctx, case, tag, batch_reads, compress, mask=MASK):
    """{route: (path, status or None)}: the one-pass device pipeline, the indexed reader, the host-pack / host-glue route"""
    nb, nf, tmp = case["nb"], case["nf"], case["tmp"]
    kw = dict(batch_reads=batch_reads, r=30, out_format="bam", records="full", compress=compress, pass_mask=mask, **TAGS)
    out = {}

    def fresh(name):
        path = str(tmp / f"{tag}_{name}.bam")
        bam.create_bam_header(path, Hdr(nb.references, nb.lengths))
        return path

    one = bam.NativeBam(case["bp"], one_pass=True, share=False)
    path = fresh("onepass")
    out["onepass"] = (path, one.realign_sequential(ctx, nf, case["regions"], path, bai=path + ".bai", **kw))
    one.close()
    idx = nb.select(case["regions"], pass_mask=mask)
    path = fresh("indexed")
    out["indexed"] = (path, nb.realign_file(ctx, nf, idx, path, bai=path + ".bai", **kw))
    ctx.set("device_pack", 0)
    ctx.set("device_glue", 0)
    try:
        path = fresh("host")
        out["host"] = (path, nb.realign_file(ctx, nf, idx, path, bai=path + ".bai", **kw))
    finally:
        ctx.set("device_pack", 1)
        ctx.set("device_glue", 1)
    return out


@pytest.mark.parametrize("compress", ["none", "huffman", "match"])
@pytest.mark.parametrize("batch_reads", [4, 4000])
def test_file_to_file(ctx, case, batch_reads, compress):
    routes = run_routes(ctx, case, f"f{batch_reads}{compress}", batch_reads, compress)
    streams = {k: record_stream(p) for k, (p, _) in routes.items()}
    assert streams["onepass"] == streams["indexed"] == streams["host"]
    got, want = [r for _, r in split_records(streams["onepass"])], [r for _, r in split_records(case["want"])]
    assert len(got) == len(want) == 39
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, k
    # status: 128 exactly at the records that passed, the reads' bits as without the flag; the refused read reported, not written
    n, bad, (refused, inconsistent) = routes["onepass"][1]
    assert (n, bad, refused, inconsistent) == (40, [(12, 32)], 1, 0)
    for name in ("indexed", "host"):
        assert np.array_equal(routes[name][1], case["want_st"]), name
    assert [k for k in range(40) if case["want_st"][k] & pc.ST_PASSED] == [k for k in range(40) if pc.passes(case["flags"][k], MASK)]
    # index: every record reachable at its own bin and linear window
    for name, (path, _) in routes.items():
        members(path)
        check_index(path, path + ".bai")
    if compress == "none":
        files = {k: (open(p, "rb").read(), open(p + ".bai", "rb").read()) for k, (p, _) in routes.items()}
        assert files["onepass"] == files["indexed"] == files["host"]
        assert sum(1 for m in members(routes["onepass"][0]) if len(m[1]) == 65280) >= 2       # (the 70 000-byte array spans a cut)


# ---- 3. the ranks' shares ------------------------------------------------------------------------------------------------------
def test_shares_concatenate(ctx, case):
    nf, tmp = case["nf"], case["tmp"]
    kw = dict(batch_reads=4, r=30, out_format="bam", records="full", pass_mask=MASK, eof=False, **TAGS)
    split = 0
    for world in (2, 3):
        parts, total = [], 0
        for rank in range(world):
            h = bam.NativeBam(case["bp"], one_pass=True, share=False)
            assert h.set_share(rank, world)[0] == 1
            path = str(tmp / f"w{world}_r{rank}.bam")
            open(path, "wb").close()
            n, bad, _ = h.realign_sequential(ctx, nf, case["regions"], path, bai=path + ".bai", **kw)
            h.close()
            parts.append(record_stream(path, header=False))
            total += n
        assert total == 40 and b"".join(parts) == case["want"], world
        split = max(split, sum(1 for p in parts if p))
    assert split >= 2            # (the file is four BGZF blocks: of two shares the second may be empty, of three two are not)


# ---- 4. mask 0 is no mask --------------------------------------------------------------------------------------------------------
def test_mask_zero_changes_nothing(ctx, case):
    nb, nf, tmp, reads = case["nb"], case["nf"], case["tmp"], case["reads"]
    never = str(tmp / "never.bam")
    bam.create_bam_header(never, Hdr(nb.references, nb.lengths))
    st0 = nb.realign_file(ctx, nf, reads, never, batch_reads=4, r=30, out_format="bam", bai=never + ".bai", records="full", **TAGS)
    zero = str(tmp / "zero.bam")
    bam.create_bam_header(zero, Hdr(nb.references, nb.lengths))
    nb.set_output("bam", zero + ".bai", True, "none", "full", **TAGS)
    assert nb._lib.npore_bam_set_output_pass(nb.handle, 0) == 0
    st1 = np.zeros(len(reads), np.int32)
    fmap = nb.fasta_map(nf)
    nb._check(nb._lib.npore_bam_realign_file(ctx.handle, nb.handle, nf.handle, fmap.ctypes.data, reads.ctypes.data, len(reads), 4, 5.0, 1.0, 20000, 30,
                                             0, os.fsencode(zero), st1.ctypes.data))
    assert np.array_equal(st0, st1) and np.array_equal(st0, case["st"])
    assert open(never, "rb").read() == open(zero, "rb").read() and open(never + ".bai", "rb").read() == open(zero + ".bai", "rb").read()
    # ... and the mask held for one run: the next run on a handle that passed records drops them again
    one = bam.NativeBam(case["bp"], one_pass=True, share=False)
    for mask, n_want in ((MASK, 40), (0, 30)):
        path = str(tmp / f"again{mask}.bam")
        bam.create_bam_header(path, Hdr(nb.references, nb.lengths))
        n, _, _ = one.realign_sequential(ctx, nf, case["regions"], path, batch_reads=4000, r=30, out_format="bam", records="full", pass_mask=mask, **TAGS)
        assert n == n_want
    assert record_stream(path) == record_stream(never)
    one.close()


# ---- 5. the tool ---------------------------------------------------------------------------------------------------------------
def test_cli_pass_through(case):
    """`realign --records full --pass_through` through both readers: the stream the rule owes, indexed; without the flag, the reads alone"""
    import subprocess
    import sys
    from conftest import REPO
    tmp = case["tmp"]
    common = [sys.executable, "-m", "npore_amd.realign", "--bam", case["bp"], "--ref", str(tmp / "p.fa"), "--out_format", "bam", "--records", "full",
              "--md", "--cs", "short", "--de", "--batch_reads", "4"]
    for name, env in (("cli_one", None), ("cli_ix", dict(os.environ, NPORE_BAM_ONE_PASS="0"))):
        prefix = str(tmp / name)
        out = subprocess.run(common + ["--out_prefix", prefix, "--pass_through"], cwd=REPO, capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        assert out.stdout.count("ERROR") == 1 and "CIGAR does not match" in out.stdout            # the refused read, and nothing about the passed ones
        assert record_stream(prefix + ".bam") == case["want"], name
        check_index(prefix + ".bam", prefix + ".bam.bai")
    prefix = str(tmp / "cli_off")
    out = subprocess.run(common + ["--out_prefix", prefix], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert record_stream(prefix + ".bam") == case["nb"].format_bam_full(case["nf"], case["reads"], case["finals"], case["st"], **TAGS)


# ---- the debug ladder: the narrow entries are the widest with zeros (one record spec behind all four) ---------------------------
def test_device_ladder_forwards_agree(ctx, case):
    """npore_debug_format_bam_full{,_md,_tags,_pass}_device on the file: every entry that can say the options equals the widest at
    zero-extended arguments, and both equal the host twin -- with everything off, with MD, with MD + cs long + de, and (the widest
    alone can say it) those with mask 0x904."""
    nb, nf, lib = case["nb"], case["nf"], case["nb"]._lib
    final_of, st_of = dict(zip(case["reads"].tolist(), case["finals"])), dict(zip(case["reads"].tolist(), case["st"].tolist()))
    cap = sum(len(r) for r in case["raws"]) * 3 + (1 << 16)
    fmap = nb.fasta_map(nf)
    for mask, md, cs, de in ((0, False, None, False), (0, True, None, False), (0, True, "long", True), (MASK, True, "long", True)):
        idx = np.array(pc.py_select(case["raws"], [(0, 0, 1 << 28), (1, 0, 1 << 28)], 0, mask), np.int64)
        finals = [final_of.get(int(k), "") for k in idx]
        status = np.array([st_of.get(int(k), 0) for k in idx], np.int32)
        n, flags, tags = len(idx), bam.OUT_MD if md else 0, bam.output_tags(cs, de)
        _keep, reads = bam.marshal_finals(idx, finals, status)
        want = nb.format_bam_full(nf, idx, finals, status, md=md, cs=cs, de=de, pass_mask=mask)
        assert len(split_records(want)) == n - 1

        def run(entry, *more):
            recs, nm, mdl, got = np.zeros(cap, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32), C.c_int64()
            more = tuple(mdl.ctypes.data if m is Ellipsis else m for m in more)
            nb._check(getattr(lib, entry)(ctx.handle, nb.handle, nf.handle, fmap.ctypes.data, *reads, recs.ctypes.data, cap, C.byref(got),
                                          nm.ctypes.data, *more))
            return recs[:got.value].tobytes(), nm.tolist(), mdl.tolist() if md else None

        wide = run("npore_debug_format_bam_full_pass_device", flags, ..., tags, mask)
        assert wide[0] == want, (mask, md, cs, de)
        if mask == 0:
            assert run("npore_debug_format_bam_full_tags_device", flags, ..., tags) == wide
        if mask == 0 and tags == 0:
            assert run("npore_debug_format_bam_full_md_device", flags, ...) == wide
        if mask == 0 and tags == 0 and not md:
            assert run("npore_debug_format_bam_full_device") == wide
