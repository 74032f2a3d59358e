"""Random input and final CIGARs through the DEVICE record chain of --records full (csrc/bam_emit_kernels.hpp: nm_count_kernel, the
size kernels of MD, cs / de, the =/X form and OC, the placement, the emit kernels): the reads of bam_fuzz_cases -- about 100 a
seed, three seeds picked so that every seam the walks carry something over is hit (tests/test_bam_fuzz.py asserts that and holds
the host twin to the Python statement on the same reads) -- through npore_debug_format_bam_full_pass_device under all 48 option
sets md x cs {none, short, long} x de x eqx x oc against the host twin's bytes; the empty and the full set against the statement
itself; pass masks; the reads handed in one by one, seven at a time and in another order; a small call before a large one on a
context of its own; and one crafted read that is long only through the =/X split, changed, with OC and CG in that order.
"""
import numpy as np
import pytest

from npore_amd import aln, bam
from test_bam_out import split_records
import bam_eqx_cases as ec
import bam_full_cases as fc
import bam_fuzz_cases as fz
import bam_oc_cases as oc
import long_cigar_cases as lc
from full_record_driver import device_full

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


class Seed:
    """one seed's files, opened once; the host twin's bytes per option set and mask, made when first asked for"""
    def __init__(self, tmp, seed):
        self.seed = seed
        references, refs, self.records, self.finals, self.status = fz.fuzz_reads(seed)
        self.bp, self.fa = fc.write_inputs(tmp, references, refs, self.records, f"s{seed}")
        self.nb, self.nf = bam.NativeBam(self.bp, stream=False), bam.NativeFasta(self.fa)
        self.idx = self.nb.select([(n, 0, l) for n, l in references], pass_mask=bam.PASS_FLAGS)      # (the records that would pass too)
        assert len(self.idx) == len(self.records)
        self._host = {}

    def host(self, kw, mask=0):
        key = (fz.set_name(kw), mask)
        if key not in self._host:
            self._host[key] = self.nb.format_bam_full(self.nf, self.idx, self.finals, self.status, pass_mask=mask, **kw)
        return self._host[key]

    def device(self, ctx, kw, mask=0, pick=None, room=None):
        pick = np.arange(len(self.idx)) if pick is None else np.asarray(pick)
        return device_full(ctx, self.nb, self.nf, self.idx[pick], [self.finals[k] for k in pick], self.status[pick],
                           cap=(len(self.host(kw, mask)) if room is None else room) + 4096, mask=mask, **kw)[0]

    def describe(self, got, want, kw, mask=0):
        return dict(options=fz.set_name(kw), mask=hex(mask), **fz.describe_difference(got, want, self.records, self.finals, self.status))

    def close(self):
        self.nb.close(); self.nf.close()


@pytest.fixture(scope="module")
def seeds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gpu_bam_fuzz")
    out = {seed: Seed(tmp, seed) for seed in fz.SEEDS}
    yield out
    for s in out.values():
        s.close()


# ---- 1. all 48 option sets: the device's bytes are the host twin's --------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.SEEDS)
def test_device_equals_host_twin_under_every_option_set(ctx, seeds, seed):
    s = seeds[seed]
    sizes = set()
    for kw in fz.OPTION_SETS:
        want = s.host(kw)
        got = s.device(ctx, kw)
        assert got == want, s.describe(got, want, kw)
        sizes.add(len(got))
    assert len(sizes) == 48 and len(split_records(got)) == len(s.records) - 3


# ---- 2. the empty and the full set against the statement itself ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.SEEDS)
def test_device_equals_statement(ctx, seeds, seed):
    s = seeds[seed]
    raws, packs = fc.input_records(s.bp), fz.fuzz_packs(seed)
    for kw in (fz.EMPTY_SET, fz.FULL_SET):
        want = fz.statement_stream(raws, s.records, packs, s.finals, s.status, **kw)
        got = s.device(ctx, kw, room=len(want))
        assert got == want, s.describe(got, want, kw)
    # which reads carry OC, and with which text, is the statement's answer read by read
    kept = [(r, f) for r, f, st in zip(s.records, s.finals, s.status) if not st & 32]
    with_tag = 0
    for (_, rec), (r, fin) in zip(split_records(got), kept):
        changed = bam.cigar_changed(oc.inner(r["cigar"]), fin)
        assert oc.oc_of_record(rec)[0] == ([oc.text_of(r["cigar"])] if changed else []), r["name"]
        with_tag += changed
    assert 0 < with_tag < len(kept)


# ---- 3. pass masks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [0x904, 0x100])
def test_device_with_a_pass_mask(ctx, seeds, mask):
    s = seeds[fz.SEEDS[0]]
    raws = fc.input_records(s.bp)
    for kw in fz.MASK_SETS:
        want = s.host(kw, mask)
        got = s.device(ctx, kw, mask)
        assert got == want, s.describe(got, want, kw, mask)
    passed = [raw for raw, r, st in zip(raws, s.records, s.status) if r["flag"] & mask and not st & 32]
    assert passed and all(raw in got for raw in passed) and got != s.host(kw)


# ---- 4. however the reads are handed in, the records are those of the one call ----------------------------------------------------------
@pytest.mark.parametrize("name", ["full", "md_oc"])
def test_slicing_does_not_matter(ctx, seeds, name):
    s = seeds[fz.SEEDS[1]]
    kw = fz.FULL_SET if name == "full" else dict(md=True, cs=None, de=False, eqx=False, oc=True)
    whole = s.host(kw)
    by_read, it = [], iter(split_records(whole))
    for st in s.status:                                          # the one call's record of every read (None: refused)
        by_read.append(None if st & 32 else next(it)[1])
    n = len(s.idx)
    for size in (1, 7):
        for lo in range(0, n, size):
            pick = np.arange(lo, min(n, lo + size))
            got = s.device(ctx, kw, pick=pick, room=len(whole))
            assert got == b"".join(by_read[k] for k in pick if by_read[k] is not None), (fz.set_name(kw), size, lo, [s.records[k]["name"] for k in pick])
    pick = np.random.default_rng(7).permutation(n)
    got = s.device(ctx, kw, pick=pick, room=len(whole))
    want = b"".join(by_read[k] for k in pick if by_read[k] is not None)
    assert got == want and got != whole, fz.set_name(kw)


# ---- 5. a small call, then a large one, on a context that has seen neither ----------------------------------------------------------------
def test_buffers_grow_between_calls(tables, seeds):
    sub, nps = tables
    own = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    try:
        s = seeds[fz.SEEDS[2]]
        whole = s.host(fz.FULL_SET)
        first = [k for k, st in enumerate(s.status) if not st & 32][:3]
        small = s.device(own, fz.FULL_SET, pick=first, room=len(whole))
        assert small == b"".join(rec for _, rec in split_records(whole)[:3])
        got = s.device(own, fz.FULL_SET)
        assert got == whole, s.describe(got, whole, fz.FULL_SET)
        assert s.device(own, fz.FULL_SET, pick=first, room=len(whole)) == small      # ... and small again behind it
    finally:
        own.close()


# ---- 6. one crafted read: long only through the split, changed, OC in front of CG -------------------------------------------------------
def test_split_long_read_with_oc_and_cg(ctx, tmp_path):
    references, refs, records, finals = fz.split_long_read()
    bp, fa = fc.write_inputs(tmp_path, references, refs, records, "split")
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    idx = nb.select([(n, 0, l) for n, l in references])
    assert len(idx) == 1
    st = np.zeros(1, np.int32)
    rc, sc, _ = lc.expected_pack(records[0], records[0]["cigar"], refs["ctg"])
    raw, = fc.input_records(bp)
    want = bam.full_record(raw, rc, sc, finals[0], **fz.FULL_SET)
    got = device_full(ctx, nb, nf, idx, finals, st, cap=len(want) + 4096, **fz.FULL_SET)[0]
    assert got == want, fz.describe_difference(got, want, records, finals, st)
    assert nb.format_bam_full(nf, idx, finals, st, **fz.FULL_SET) == want
    text, n_cigar_op = ec.record_cigar_text(got)
    assert n_cigar_op == 2 and text == "1S" + "1=1X" * 32766 + "1=" + "1I" + "2S" and text.count("=") + text.count("X") + 3 == 65536
    texts, tags = oc.oc_of_record(got)
    assert texts == ["1S30000M0I35534M2S"] and tags == [b"RG", b"NM", b"MD", b"cs", b"de", b"OC", b"CG"]
    # without the split the same read is a plain record of four words, its OC in the same place
    kw = dict(fz.FULL_SET, eqx=False)
    plain = device_full(ctx, nb, nf, idx, finals, st, cap=len(want) + 4096, **kw)[0]
    assert plain == bam.full_record(raw, rc, sc, finals[0], **kw) and ec.record_cigar_text(plain) == ("1S65533M1I2S", 4)
    assert oc.oc_of_record(plain) == (texts, tags[:-1])
    nb.close(); nf.close()
