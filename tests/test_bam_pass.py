"""Pass-through (--pass_through, npore_bam_set_output_pass), host side: the setter, the selection npore_bam_select_pass and the
host twin npore_bam_format_bam_full_pass on the file of tests/bam_pass_cases.py -- against the rule of
npore_amd/csrc/staged_head.hpp (a record PASSES iff flag & mask != 0) restated there in Python: a record that passes is the
input's bytes, cut from the inflated input here; every other record is what npore_bam_format_bam_full_tags makes of the reads
alone.  No GPU: the final CIGARs are the input's own.
"""
import numpy as np
import pytest

from npore_amd import _lib, bam
from test_bam_out import split_records
import bam_full_cases as fc
import bam_pass_cases as pc
import long_cigar_cases as lc
from full_record_driver import host_full

MASKS = (0x904, 0x100, 0x800, 0x4, 0x900, 0x104)
EOF, PART, DEFLATE, MATCH, FULL, MD = bam.OUT_EOF, bam.OUT_PART, bam.OUT_DEFLATE, bam.OUT_MATCH, bam.OUT_FULL, bam.OUT_MD      # npore_bam_set_output's flags
ALL_FLAGS = EOF | PART | DEFLATE | MATCH | FULL | MD
CS, CS_LONG, DE = bam.TAG_CS, bam.TAG_CS_LONG, bam.TAG_DE                  # npore_bam_set_output_tags' word


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pass")
    references, refs, records = pc.pass_file()
    bp, fa = str(tmp / "p.bam"), str(tmp / "p.fa")
    pc.write_bam(bp, references, records)
    lc.write_fasta(fa, refs)
    raws = fc.input_records(bp)
    assert len(raws) == len(records) == 40
    nb, nf = bam.NativeBam(bp, stream=False), bam.NativeFasta(fa)
    yield dict(references=references, refs=refs, records=records, raws=raws, flags=[r["flag"] for r in records], nb=nb, nf=nf, bp=bp, fa=fa,
               finals=pc.finals_of(records), status=np.array([32 if r["_kind"] == "refused" else 0 for r in records], np.int32))
    nb.close(); nf.close()


def test_the_file_is_what_the_issue_asks_for(case):
    records, raws = case["records"], case["raws"]
    kinds = [r["_kind"] for r in records]
    assert kinds[0] != "primary" and kinds[-1] != "primary" and all(k != "primary" for k in kinds[16:20]) and 16 % 4 == 0
    assert records[0]["seq"] == "" and len(records[4]["seq"]) % 2 == 1 and records[4]["cigar"][0][0] == pc.H == records[4]["cigar"][-1][0]
    assert records[7]["flag"] == 4 and records[7]["cigar"] == [] and records[7]["ref_id"] >= 0
    assert len(raws[11]) > 65280 + 4000 and all(t in raws[11] for t in (b"NMS", b"MDZ", b"csZ", b"MLBC"))
    assert records[12]["_kind"] == "refused"
    rid, pos, flag, rl = pc.parse(raws[30])                      # the placeholder: two words, the real three in the tag
    assert raws[30][16:18] == b"\x02\x00" and b"CGBI\x03\x00\x00\x00" in raws[30] and rl == 102
    assert {r[12] for r in raws} == set(range(1, 9))             # l_read_name 1 ... 8
    assert {len(b"".join(raws[:k])) % 4 for k in range(40)} == {0, 1, 2, 3}
    assert all(200 <= lc.ref_len(r["cigar"]) <= 2010 for r in records if r["_kind"] == "primary")
    for r in records:
        if r["_kind"] == "primary":
            ops = [op for op, _ in r["cigar"] if op != pc.H]
            assert ops[0] == pc.S == ops[-1]


def test_setter(case):
    nb, lib = case["nb"], case["nb"]._lib
    assert lib.npore_abi_version() == 2
    assert lib.npore_bam_set_output_pass(nb.handle, 0x904) != 0                      # (a fresh handle writes SAM)
    for fmt, flags in ((0, 0), (1, EOF), (1, PART), (1, EOF | DEFLATE), (1, EOF | DEFLATE | MATCH)):      # no FULL set_output in front
        assert lib.npore_bam_set_output(nb.handle, fmt, None, flags) == 0
        assert lib.npore_bam_set_output_pass(nb.handle, 0x100) != 0, (fmt, flags)
        assert lib.npore_bam_set_output_pass(nb.handle, 0) != 0, (fmt, flags)
    for flags in (EOF | FULL, PART | FULL, EOF | FULL | MD, EOF | DEFLATE | FULL):
        assert lib.npore_bam_set_output(nb.handle, 1, None, flags) == 0
        for bit in range(31):
            mask = 1 << bit
            assert (lib.npore_bam_set_output_pass(nb.handle, mask) == 0) == (mask in (0x4, 0x100, 0x800)), (flags, bit)
        for mask in (0x904 | 1, 0x904 | 0x400, 0x1904, -1):
            assert lib.npore_bam_set_output_pass(nb.handle, mask) != 0, mask
        for mask in (0, 0x904, 0x900, 0x104):
            assert lib.npore_bam_set_output_pass(nb.handle, mask) == 0, mask
    # every set_output clears the mask: a run behind it passes nothing (the host's view of the mask: npore_bam_pack_sizes)
    idx = np.arange(40, dtype=np.int64)
    sizes = lambda: [np.diff(a) for a in nb.pack(case["nf"], idx)[1::2]]
    assert lib.npore_bam_set_output(nb.handle, 1, None, EOF | FULL) == 0 and lib.npore_bam_set_output_pass(nb.handle, 0x904) == 0
    with_mask = sizes()
    assert lib.npore_bam_set_output(nb.handle, 1, None, EOF | FULL) == 0
    without = sizes()
    for k in range(40):
        if pc.passes(case["flags"][k], 0x904):
            assert [int(a[k]) for a in with_mask] == [0, 0, 0], k
        else:
            assert [int(a[k]) for a in with_mask] == [int(a[k]) for a in without], k
    assert any(int(a[4]) > 0 for a in without)                                      # (without the mask a supplementary is a read like any other)
    # what the other setters refuse stays refused
    assert lib.npore_bam_set_output(nb.handle, 1, None, 64 | FULL | EOF) != 0
    assert lib.npore_bam_set_output(nb.handle, 0, None, 0) == 0
    # the ABI lists the four new symbols with the arguments of their parents plus the mask
    for name in ("npore_bam_set_output_pass", "npore_bam_select_pass", "npore_bam_format_bam_full_pass", "npore_debug_format_bam_full_pass_device"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["npore_bam_select_pass"][1]) == len(_lib.SIGNATURES["npore_bam_select"][1]) + 1
    assert len(_lib.SIGNATURES["npore_bam_format_bam_full_pass"][1]) == len(_lib.SIGNATURES["npore_bam_format_bam_full_tags"][1]) + 1
    assert len(_lib.SIGNATURES["npore_debug_format_bam_full_pass_device"][1]) == len(_lib.SIGNATURES["npore_debug_format_bam_full_tags_device"][1]) + 1


def select_pass_raw(nb, regions, max_reads, mask):
    """npore_bam_select_pass as it is (mask 0 too, which NativeBam.select hands to npore_bam_select)"""
    rid = np.array([r for r, _, _ in regions], np.int32)
    beg = np.array([s for _, s, _ in regions], np.int64)
    end = np.array([e for _, _, e in regions], np.int64)
    out = np.zeros(200, np.int64)
    k = nb._lib.npore_bam_select_pass(nb.handle, len(regions), rid.ctypes.data, beg.ctypes.data, end.ctypes.data, max_reads, mask, out.ctypes.data, len(out))
    assert 0 <= k <= len(out)
    return out[:k].tolist()


def test_selection(case):
    nb, raws, references, records = case["nb"], case["raws"], case["references"], case["records"]
    at = records[pc.UNMAPPED_AT]["pos"]
    whole = [(0, 0, references[0][1]), (1, 0, references[1][1])]
    region_sets = [whole, [(0, at, at + 3000)], [(0, at + 1, at + 3000)], [(0, 0, at)], [(0, 0, at + 1)], [(1, 500, 9000), (0, 100, 4000)],
                   [(0, records[3]["pos"] + 50, records[17]["pos"] + 1)]]
    names = lambda regs: [(references[r][0], s, e) for r, s, e in regs]
    for regs in region_sets:
        for max_reads in (0, 1, 5, 8, 17, 18, 19, 20, 39):         # (8, 17 - 20: the cap lands on a passed record with the whole mask)
            assert select_pass_raw(nb, regs, max_reads, 0) == nb.select(names(regs), max_reads).tolist() == pc.py_select(raws, regs, max_reads, 0)
            for mask in MASKS:
                want = pc.py_select(raws, regs, max_reads, mask)
                assert select_pass_raw(nb, regs, max_reads, mask) == want, (regs, max_reads, mask)
                assert nb.select(names(regs), max_reads, pass_mask=mask).tolist() == want
    assert pc.py_select(raws, whole, 0, 0x904) == list(range(40))
    assert pc.py_select(raws, whole, 8, 0x904)[-1] == 7 and pc.py_select(raws, whole, 20, 0x904)[-1] == 19
    # the record without a CIGAR, exactly at a region's start: in with its bit (as if its length were 1), never without; one base on, out
    assert pc.UNMAPPED_AT in pc.py_select(raws, [(0, at, at + 3000)], 0, 0x4) and pc.UNMAPPED_AT in pc.py_select(raws, [(0, at, at + 3000)], 0, 0x904)
    assert pc.UNMAPPED_AT not in pc.py_select(raws, [(0, at, at + 3000)], 0, 0x900)
    assert pc.UNMAPPED_AT not in pc.py_select(raws, [(0, at + 1, at + 3000)], 0, 0x904)
    assert pc.UNMAPPED_AT not in pc.py_select(raws, [(0, 0, at)], 0, 0x904) and pc.UNMAPPED_AT in pc.py_select(raws, [(0, 0, at + 1)], 0, 0x904)
    for bad in (1, 0x400, 0x1000, -1):
        assert nb._lib.npore_bam_select_pass(nb.handle, 0, None, None, None, 0, bad, None, 0) < 0


@pytest.mark.parametrize("md,cs,de", [(False, None, False), (True, None, False), (False, "short", True), (True, "long", True)])
def test_record_bytes(case, md, cs, de):
    nb, nf, raws, flags, finals, status = (case[k] for k in ("nb", "nf", "raws", "flags", "finals", "status"))
    all_idx = np.arange(40, dtype=np.int64)
    kw = dict(md=md, cs=cs, de=de)
    # mask 0: the bytes of npore_bam_format_bam_full_tags, for the reads npore_bam_select keeps
    reads = np.array(pc.py_select(raws, [(0, 0, 1 << 28), (1, 0, 1 << 28)], 0, 0), np.int64)
    plain = nb.format_bam_full(nf, reads, [finals[k] for k in reads], status[reads], **kw)
    assert host_full(nb, nf, reads, [finals[k] for k in reads], status[reads], flags=MD if md else 0, tags=bam.output_tags(cs, de)) == (0, plain)
    assert len(split_records(plain)) == len(reads) - 1            # the refused read is absent
    for mask in MASKS:
        idx = np.array(pc.py_select(raws, [(0, 0, 1 << 28), (1, 0, 1 << 28)], 0, mask), np.int64)
        rest = np.array([k for k in idx if not pc.passes(flags[k], mask)], np.int64)
        assert set(rest) == set(reads.tolist())
        want = pc.compose(raws, flags, mask, idx.tolist(), {12}, [r for _, r in split_records(plain)])
        got = nb.format_bam_full(nf, idx, [finals[k] for k in idx], status[idx], pass_mask=mask, **kw)
        got_recs = [r for _, r in split_records(got)]
        assert len(got_recs) == len(want) == len(idx) - 1
        for k, (g, w) in enumerate(zip(got_recs, want)):
            assert g == w, (mask, k)
        assert got == b"".join(want)
    # in file order with the whole mask: every passing index is the input's record
    got_recs = [r for _, r in split_records(nb.format_bam_full(nf, all_idx, finals, status, pass_mask=0x904, **kw))]
    order = [k for k in range(40) if k != 12]
    for g, k in zip(got_recs, order):
        if pc.passes(flags[k], 0x904):
            assert g == raws[k], k
            assert g[14:16] == (k).to_bytes(2, "little")         # (the input's bin, whatever it says)
    assert sum(pc.passes(f, 0x904) for f in flags) == 10
    # a bit outside 0x904 is refused
    assert host_full(nb, nf, reads, [finals[k] for k in reads], status[reads], mask=0x904 | 2)[0] != 0


def test_cli_refuses_pass_through_without_full_records(case, tmp_path):
    """`realign --pass_through` needs --out_format bam --records full: one ERROR line, exit 1, nothing written (no GPU is touched)"""
    import os
    import subprocess
    import sys
    from conftest import REPO
    for extra in ([], ["--out_format", "bam"], ["--out_format", "bam", "--records", "reference"]):
        prefix = str(tmp_path / "bad")
        out = subprocess.run([sys.executable, "-m", "npore_amd.realign", "--bam", case["bp"], "--ref", case["fa"], "--out_prefix", prefix,
                              "--pass_through"] + extra, cwd=REPO, capture_output=True, text=True, timeout=120)
        assert out.returncode == 1, out.stdout[-2000:] + out.stderr[-2000:]
        errors = [l for l in out.stdout.splitlines() if l.startswith("ERROR")]
        assert len(errors) == 1 and "--pass_through" in errors[0] and "--records full" in errors[0], out.stdout
        assert not os.path.exists(prefix + ".bam") and not os.path.exists(prefix + ".sam")
    text = subprocess.run([sys.executable, "-m", "npore_amd.realign", "--help"], cwd=REPO, capture_output=True, text=True, timeout=120).stdout
    flat = " ".join(text.split())
    assert "--pass_through" in flat and "unplaced" in flat and "0x100" in flat and "0x800" in flat and "0x4" in flat


# ---- the record spec (csrc/hostio.hpp RecSpec, rec_spec_of): one statement of the output options' rules behind every entry ------
def ladder_args(case, idx):
    """the arguments the four host entries share, and where they leave the records"""
    import ctypes as C
    nb = case["nb"]
    keep, reads = bam.marshal_finals(idx, [case["finals"][k] for k in idx], case["status"][idx])
    fmap, recs, n = nb.fasta_map(case["nf"]), C.c_void_p(), C.c_int64()
    args = (nb.handle, case["nf"].handle, fmap.ctypes.data, *reads, 0, C.byref(recs), C.byref(n))
    return args, (lambda: C.string_at(recs.value, n.value)), (keep, fmap)


@pytest.mark.parametrize("mask", [0, 0x4, 0x100, 0x800, 0x904])
def test_the_ladder_forwards_agree(case, mask):
    """All twelve (md, cs, de) combinations: every entry of npore_bam_format_bam_full{,_md,_tags,_pass} that can say the combination
    -- a narrower one where the options it lacks are zero, the widest always -- returns the same bytes, NativeBam.format_bam_full's."""
    nb, lib = case["nb"], case["nb"]._lib
    idx = np.array(pc.py_select(case["raws"], [(0, 0, 1 << 28), (1, 0, 1 << 28)], 0, mask), np.int64)
    args, got, _keep = ladder_args(case, idx)
    combos = [(md, cs, de) for md in (False, True) for cs in (None, "short", "long") for de in (False, True)]
    assert len(combos) == 12
    for md, cs, de in combos:
        flags, tags = MD if md else 0, bam.output_tags(cs, de)
        want = nb.format_bam_full(case["nf"], idx, [case["finals"][k] for k in idx], case["status"][idx], md=md, cs=cs, de=de, pass_mask=mask)
        assert len(split_records(want)) == len(idx) - 1            # (the refused read is absent)
        calls = [lambda: lib.npore_bam_format_bam_full_pass(*args, flags, tags, mask)]
        if mask == 0:
            calls.append(lambda: lib.npore_bam_format_bam_full_tags(*args, flags, tags))
        if mask == 0 and tags == 0:
            calls.append(lambda: lib.npore_bam_format_bam_full_md(*args, flags))
        if mask == 0 and tags == 0 and not md:
            calls.append(lambda: lib.npore_bam_format_bam_full(*args))
        for k, call in enumerate(calls):
            assert call() == 0 and got() == want, (mask, md, cs, de, k)


def spec_ok(fmt, flags, tags, pas):
    """csrc/hostio.hpp rec_spec_of restated: defined bits only, CS_LONG beside CS, md / tags / pass on FULL records, FULL records in BAM"""
    full = bool(flags & FULL)
    return not (flags & ~ALL_FLAGS or tags & ~(CS | CS_LONG | DE) or pas & ~0x904 or (tags & CS_LONG and not tags & CS)
                or (not full and (flags & MD or tags or pas)) or (full and fmt != 1))


def set_output_ok(fmt, flags):
    """... and npore_bam_set_output's own: a known format, DEFLATE in BAM, MATCH beside DEFLATE, a FULL run ends a file or writes a part"""
    return fmt in (0, 1) and not (flags & DEFLATE and fmt != 1) and not (flags & MATCH and not flags & DEFLATE) and not (flags & FULL and not flags & (EOF | PART)) and spec_ok(fmt, flags, 0, 0)


def test_the_rule_table(case):
    """Every (format, flags, tags, pass) over the defined bits and one undefined bit each, through npore_bam_set_output, _pass and
    _tags in that order on a fresh handle: accepted and refused as the rules above say.  And the host entry accepts (flags, tags,
    pass) exactly when the setters accept them for a FULL BAM run."""
    lib = case["nb"]._lib
    flag_sets = list(range(ALL_FLAGS + 1)) + [64, 64 | FULL | EOF]
    tag_sets, pass_sets = list(range((CS | CS_LONG | DE) + 1)) + [8], [a | b | c for a in (0, 4) for b in (0, 0x100) for c in (0, 0x800)] + [0x400]
    for fmt in (0, 1, 2):
        for flags in flag_sets:
            e1 = set_output_ok(fmt, flags)
            if not e1:                                           # nothing is held: every option is refused (one handle serves them all)
                nb = bam.NativeBam(case["bp"], stream=False)
                assert lib.npore_bam_set_output(nb.handle, fmt, None, flags) != 0, (fmt, flags)
                for tags in tag_sets:
                    assert lib.npore_bam_set_output_tags(nb.handle, tags) != 0, (fmt, flags, tags)
                for pas in pass_sets:
                    assert lib.npore_bam_set_output_pass(nb.handle, pas) != 0, (fmt, flags, pas)
                nb.close()
                continue
            for tags in tag_sets:
                for pas in pass_sets:
                    nb = bam.NativeBam(case["bp"], stream=False)
                    held = bool(flags & FULL)
                    e2 = held and spec_ok(fmt, flags, 0, pas)
                    e3 = held and spec_ok(fmt, flags, tags, pas if e2 else 0)
                    got = (lib.npore_bam_set_output(nb.handle, fmt, None, flags) == 0, lib.npore_bam_set_output_pass(nb.handle, pas) == 0,
                           lib.npore_bam_set_output_tags(nb.handle, tags) == 0)
                    nb.close()
                    assert got == (True, e2, e3), (fmt, flags, tags, pas)
    nb = case["nb"]
    args, _got, _keep = ladder_args(case, np.zeros(0, np.int64))
    for flags in (0, MD, 64, MD | 64, FULL, EOF):                  # (the entry's flags know NPORE_OUT_MD alone: FULL and the writer's bits are not its to take)
        for tags in tag_sets:
            for pas in pass_sets:
                assert lib.npore_bam_set_output(nb.handle, 1, None, FULL | EOF) == 0
                setters = flags in (0, MD) and lib.npore_bam_set_output(nb.handle, 1, None, FULL | EOF | flags) == 0 and \
                    lib.npore_bam_set_output_pass(nb.handle, pas) == 0 and lib.npore_bam_set_output_tags(nb.handle, tags) == 0
                assert setters == (flags in (0, MD) and spec_ok(1, FULL | EOF | flags, tags, pas))
                assert (lib.npore_bam_format_bam_full_pass(*args, flags, tags, pas) == 0) == setters, (flags, tags, pas)
    assert lib.npore_bam_set_output(nb.handle, 0, None, 0) == 0


def test_the_setting_is_spent_once(case, tmp_path):
    """A run takes the setting and leaves the default: npore_bam_write_file, which refuses FULL records, is such a run -- behind it
    the handle writes SAM again, _pass and _tags are refused as on a fresh handle, and the mask npore_bam_pack_sizes sees is gone."""
    nb, lib = case["nb"], case["nb"]._lib
    idx = np.arange(40, dtype=np.int64)
    sizes = lambda: [np.diff(a).tolist() for a in nb.pack(case["nf"], idx)[1::2]]
    without = sizes()
    assert lib.npore_bam_set_output(nb.handle, 1, None, FULL | MD | EOF) == 0
    assert lib.npore_bam_set_output_pass(nb.handle, 0x904) == 0 and lib.npore_bam_set_output_tags(nb.handle, CS | CS_LONG | DE) == 0
    assert sizes() != without
    out = tmp_path / "never.bam"
    assert lib.npore_bam_write_file(nb.handle, None, 0, 1, None, None, None, None, 0, str(out).encode()) != 0
    assert b"FULL records" in lib.npore_last_error() and not out.exists()      # (refused for what the setting said, which it thereby took)
    assert sizes() == without
    for mask in (0, 0x4, 0x904):
        assert lib.npore_bam_set_output_pass(nb.handle, mask) != 0, mask
    for tags in (0, CS, DE, CS | CS_LONG | DE):
        assert lib.npore_bam_set_output_tags(nb.handle, tags) != 0, tags
    assert lib.npore_bam_write_file(nb.handle, None, 0, 1, None, None, None, None, 0, str(out).encode()) != 0      # (SAM again: no BAM run)
    assert b"npore_bam_set_output first" in lib.npore_last_error() and not out.exists()
