"""What a one-pass handle takes from the .bai beside the BAM -- the ranks' cuts (npore_bam_set_share) and which contigs
have reads (the default regions) -- under an index that is stale, somebody else's, bent or no index at all: decided on the
host before any kernel runs, and it decides which records reach the GPU.  CPU tests over tests/bai_trust_cases.py, whose
`expected` states the rule; the reader is the product's, built with plain g++ (tests/model/bam_walk.cpp).  With the
device behind it: tests/test_gpu_bai_trust.py."""
import argparse
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bai_trust_cases as btc
from model import bam_walk
from npore_amd import bam, cfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -5


class Family:
    pass


@pytest.fixture(scope="module")
def fam(tmp_path_factory):
    """the file, its index family as files (in a directory of their own: nothing lies beside the BAM), the single walk"""
    tmp = tmp_path_factory.mktemp("bai_trust")
    f = Family()
    f.tmp = tmp
    f.path, f.recs = btc.share_test_bam(tmp)
    f.raw = open(f.path, "rb").read()
    f.stream = btc.Stream(f.raw)
    f.bytes = btc.index_family(tmp, f.path, f.recs)
    os.mkdir(tmp / "idx")
    f.file = {}
    for name, raw in f.bytes.items():
        f.file[name] = str(tmp / "idx" / (name.replace("=", "_") + ".bai"))
        with open(f.file[name], "wb") as fh:
            fh.write(raw)
    assert bam.NativeBam.bai_path(f.path) is None
    f.whole = bam_walk.one_pass(f.path, btc.REGIONS)
    assert np.array_equal(f.whole, f.stream.starts) and len(f.whole) == 400
    return f


def _decision(f, name, world):
    """(accepted by every rank?, [(begin, end)] of the ranks as expected() writes them) -- asserting that the ranks agree"""
    rc, spans = bam_walk.shares(f.path, f.file[name], world)
    assert set(rc) in ({0}, {UNSUPPORTED}), (name, world, rc)
    n, first = len(f.stream.data), f.stream.first_record
    norm = [(n if b == -1 else first if b == 0 else b, n if e == -1 else e) for b, e in spans]
    return rc[0] == 0, norm


def test_the_family_is_what_it_says(fam):
    """The cases themselves: the file has several BGZF members and about 17 linear offsets; the stale indexes come from
    files with the same header; the straddling cuts do straddle; expected() accepts the file's own index at every world
    with cuts that are record starts, ascending."""
    s = fam.stream
    assert sum(1 for m in s.members if m[4]) >= 5 and 12 <= len(btc.linear_offsets(fam.bytes["true"])) <= 24
    for name in fam.bytes:
        assert btc.parse_bai(fam.bytes[name]) is not None and len(btc.parse_bai(fam.bytes[name])) == 2, name
    assert btc.parse_bai(fam.bytes["samtools-like"])[0][0] > 0 and btc.parse_bai(fam.bytes["true"])[0][0] == 0
    for world in btc.WORLDS:
        cuts = btc.expected(fam.raw, fam.bytes["true"], world, s)
        assert cuts != btc.REFUSE and len(cuts) == world + 1 and cuts == sorted(cuts) and cuts[0] == s.starts[0] and cuts[-1] == len(s.data)
        assert all(c in s.starts or c == len(s.data) for c in cuts) and len(set(cuts)) >= min(world, 4)
        cuts = btc.expected(fam.raw, fam.bytes["straddle"], world, s)
        assert cuts != btc.REFUSE and any(btc.straddles(s, c) for c in cuts[1:-1] if c < len(s.data)), world
    # an offset mutant changes offsets and nothing else
    assert [n for n, _ in btc.parse_bai(fam.bytes["uoff+1"])] == [n for n, _ in btc.parse_bai(fam.bytes["true"])]
    assert btc.linear_offsets(fam.bytes["uoff+1"]) == [v + 1 for v in btc.linear_offsets(fam.bytes["true"])]
    assert btc.linear_offsets(fam.bytes["coff+18"]) == [v + (18 << 16) for v in btc.linear_offsets(fam.bytes["true"])]


@pytest.mark.parametrize("world", btc.WORLDS)
def test_every_rank_makes_one_decision(fam, world):
    """For every index of the family: every rank refuses at set_share or every rank accepts -- no rank walks anything
    while another rank errors --, the outcome and the cuts are expected()'s, and where the ranks accept, their kept
    offsets one after the other are the single walk's 400."""
    for name in fam.bytes:
        want = btc.expected(fam.raw, fam.bytes[name], world, fam.stream)
        accepted, spans = _decision(fam, name, world)
        assert accepted == (want != btc.REFUSE), (name, world)
        parts, errors = [], []
        for rank in range(world):
            try:
                parts.append(bam_walk.one_pass(fam.path, btc.REGIONS, 0, rank, world, fam.file[name]))
            except bam_walk.WalkError as e:
                errors.append(str(e))
        if not accepted:
            assert not parts and len(errors) == world and all(e.startswith(f"{UNSUPPORTED}:") for e in errors), (name, world, errors[:2])
            assert all(fam.file[name] in e for e in errors), errors[0]                 # the message names the index
            continue
        assert not errors, (name, world, errors[:2])
        n = len(fam.stream.data)
        assert spans == [(want[r], want[r + 1]) if want[r] < n else (n, n) for r in range(world)], (name, world)
        assert np.array_equal(np.concatenate(parts), fam.whole), (name, world)
        for rank in range(world):
            assert all(want[rank] <= o < want[rank + 1] for o in parts[rank]), (name, world, rank)


def test_named_outcomes(fam):
    """What expected() must say for the family, by name, at EVERY world -- also at one whose own cuts all happen to be
    good (at world 2 the one cut lies below the offsets that past-eof and plus-7000 move)."""
    for world in btc.WORLDS:
        for name in btc.ACCEPTED:
            assert btc.expected(fam.raw, fam.bytes[name], world, fam.stream) != btc.REFUSE, (name, world)
            assert _decision(fam, name, world)[0], (name, world)
        for name in btc.REFUSED:
            assert btc.expected(fam.raw, fam.bytes[name], world, fam.stream) == btc.REFUSE, (name, world)
            assert not _decision(fam, name, world)[0], (name, world)
    # the premise of the docstring: at world 2 the cut that the file's own index gives is one that those two leave alone
    cut2 = btc.expected(fam.raw, fam.bytes["true"], 2, fam.stream)[1]
    for name in ("past-eof", "plus-7000"):
        assert fam.stream.voff(cut2) in btc.linear_offsets(fam.bytes[name]), name


def _regions_of(path, names):
    """the default regions get_bam_regions makes from a one-pass handle on `path`, as (ref_id, start, stop)"""
    h = bam.NativeBam(path, one_pass=True, share=False)
    old = cfg.args
    cfg.args = argparse.Namespace(contig=None, contigs=None, bed=None, contig_beg=None, contig_end=None, bam=path, ref="ref.fa")
    try:
        regions = bam.get_bam_regions(h, {n: None for n in names})
        assert h.refs_with_reads() == bam_walk.refs_with_reads(path)              # (the g++ twin opens the file the same way)
    finally:
        cfg.args = old
        h.close()
    ids = {n: k for k, n in enumerate(names)}
    return [(ids[c], s, e) for c, s, e in regions]


def test_contigs_the_index_declares_empty(fam, tmp_path):
    """With a stale index beside the file as x.bam.bai, a one-pass walk over the default regions yields exactly what it
    yields with no index, or fails with a message that names the index: never fewer records without an error.  The
    contig declared empty lies behind the last region, before the first, and between two."""
    three = btc.three_contig_records(fam.recs)
    files = []                                                   # (BAM, references, {index name: bytes}, the ones that must fail)
    p2 = str(tmp_path / "two.bam")
    shutil.copy(fam.path, p2)
    files.append((p2, btc.REFS, {n: fam.bytes[n] for n in ("stale-first-250", "stale-contig-a", "stale-every-other", "true")},
                  {"stale-first-250", "stale-contig-a"}))       # (both declare contig b empty: behind the last region)
    p3 = str(tmp_path / "three.bam")
    bam.write_bam(p3, btc.REFS3, three, level=1)
    stale3 = {"no-c": [r for r in three if r["ref_id"] != 2],    # behind the last region
              "no-a": [r for r in three if r["ref_id"] != 0],    # before the first
              "no-b": [r for r in three if r["ref_id"] != 1],    # between two
              "only-b": [r for r in three if r["ref_id"] == 1],
              "none": [],                                        # every contig declared empty: no region at all
              "all": three}
    idx3 = {n: btc._index_of(tmp_path, n, btc.REFS3, recs) for n, recs in stale3.items()}
    files.append((p3, btc.REFS3, idx3, {"no-c", "no-a", "no-b", "only-b", "none"}))
    for path, refs, indexes, must_fail in files:
        names = [n for n, _ in refs]
        bai = path + ".bai"
        assert not os.path.exists(bai)
        all_regions = [(k, 0, l - 1) for k, (_, l) in enumerate(refs)]
        assert _regions_of(path, names) == all_regions           # no index: every contig is assumed to have reads
        whole = bam_walk.one_pass(path, all_regions)
        assert len(whole) == 400
        for name, raw in indexes.items():
            with open(bai, "wb") as fh:
                fh.write(raw)
            declared = btc.declared_with_reads(raw, len(refs))
            regions = _regions_of(path, names)
            assert regions == [all_regions[k] for k in sorted(declared)], name
            try:
                got = bam_walk.one_pass(path, regions)
            except bam_walk.WalkError as e:
                assert bai in str(e) and "stale" in str(e), (name, str(e))
                assert name in must_fail, name
            else:
                assert np.array_equal(got, whole), name          # never fewer records without an error
                assert name not in must_fail, name
            os.remove(bai)


def test_malformed_indexes_are_no_indexes(fam, tmp_path):
    """Files that are no .bai -- every proper prefix of the file's own index, counts of 0x7fffffff, a wrong magic, an n_ref
    that is not the header's: set_share says unsupported on every rank and refs_with_reads() is every contig."""
    true = fam.bytes["true"]
    cases = dict(btc.malformed(true, 2))
    cases.update({f"prefix-{n}": true[:n] for n in (0, 3, 4, 7, 8, 11, 12, 16, len(true) // 2, len(true) - 8, len(true) - 1)})
    p = str(tmp_path / "m.bam")
    shutil.copy(fam.path, p)
    for name, raw in cases.items():
        assert btc.expected(fam.raw, raw, 2, fam.stream) == btc.REFUSE and btc.declared_with_reads(raw, 2) == {0, 1}, name
        with open(p + ".bai", "wb") as fh:
            fh.write(raw)
        rc, _ = bam_walk.shares(p, p + ".bai", 3)
        assert rc == [UNSUPPORTED] * 3, (name, rc)
        assert bam_walk.refs_with_reads(p) == {0, 1}, name
    assert all(btc.parse_bai(true[:n]) is None for n in range(len(true))) and btc.parse_bai(true) is not None


def test_bai_reader_under_sanitizers(fam, tmp_path):
    """The same, every proper prefix included, by a stand-alone program (tests/model/bai_sanitize.cpp) under
    AddressSanitizer and UBSan with no allocation above 64 MB: a vector sized by an unchecked n_ref is an error there."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = os.path.join(REPO, "tests", "model", "bai_sanitize.cpp")
    exe = str(tmp_path / "bai_sanitize")
    # (the runtimes linked statically: the program needs nothing preloaded and does not mind what is)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + san + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is missing")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + san + ["-o", exe, src, "-lz", "-lpthread"])
    true = fam.bytes["true"]
    cases = list(btc.malformed(true, 2).values()) + [true[:n] for n in range(len(true))]
    blob = str(tmp_path / "cases.bin")
    with open(blob, "wb") as fh:
        fh.write(b"".join(struct.pack("<i", len(c)) + c for c in cases))
    p = str(tmp_path / "m.bam")
    shutil.copy(fam.path, p)
    out = subprocess.run([exe, p, blob], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="max_allocation_size_mb=64"))
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]
    assert out.stdout.split() == [str(len(cases))]
