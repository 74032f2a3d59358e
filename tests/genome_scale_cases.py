"""Inputs shared by tests/test_genome_scale_cases.py and tests/test_gpu_genome_scale.py: reads at genome coordinates on
several contigs -- a BAM header of four contigs, one of them of 2^26 + 8192 bases, a FASTA that holds three of them in
another order, reads on both sides of every border of the BAI bin scheme (2^14, 2^17, 2^20, 2^23, 2^26), mates on other
contigs and beyond 2^26, reads that run past their contig's end, and the range sets of the pileup counts.  Every
expectation is written down from the rule (bam_reader.hpp, unpack_kernels.hpp, SAM specification 5.3), not from a run."""
import functools

import numpy as np

from npore_amd import bam, synth
import bam_full_cases as fc

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
BIG = "chrBig"
BIG_LEN = (1 << 26) + 8192
HEADER = [("alpha", 5000), (BIG, BIG_LEN), ("decoy", 300), ("zeta", 5000)]       # the BAM header's order
FASTA_ORDER = ["zeta", BIG, "alpha"]                                             # the FASTA's: another order, no decoy
FASTA_MAP = [2, 1, -1, 0]                                                        # index of each BAM reference in the FASTA
BORDERS = tuple(1 << k for k in (14, 17, 20, 23, 26))                            # level 4 ... level 0 of the bin scheme
HALF = 2000                                                                      # chrBig is N but for [b - HALF, b + HALF) and its end
PLACEMENTS = "abcdef"
BATCH = 5


def placement(b, which, length):
    """[start, stop) on chrBig of the read of `length` reference bases placed `which` way at border b"""
    start = {"a": b - 150, "b": b - length, "c": b + 1 - length, "d": b - 1, "e": b, "f": b + 7}[which]
    return start, start + length


def _letters(codes):
    return np.frombuffer(b"NACGT", np.uint8)[np.asarray(codes)].tobytes().decode()


def _runs(cg):
    """[(op, length)] of make_read's edit script over '=XID'"""
    a = np.frombuffer(bytes(cg), np.uint8)
    cut = np.flatnonzero(np.diff(a)) + 1
    starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(a)]])
    return [("MIDNSHP=X".index(chr(a[s])), int(e - s)) for s, e in zip(starts, ends)] if len(a) else []


@functools.lru_cache(maxsize=None)
def case(seed=23):
    """(references, refs, records, decoy_records): the header's [(name, length)], {contig: str} of the FASTA's three contigs,
    the records of the main BAM in coordinate order (keys with `_` are notes for the tests: `_hp`, `_place` = (border,
    letter) or None, `_bad`, `_over` = reference bases past the contig's end) and the one record of the second BAM.
    The result is shared: do not change it."""
    rng = np.random.default_rng(seed)
    windows = {}                                              # (contig, start of the window) -> make_ref's (codes, np_starts, np_period)
    big = np.full(BIG_LEN, ord("N"), np.uint8)
    for b in BORDERS:
        windows[(BIG, b - HALF)] = synth.make_ref(rng, 2 * HALF, 0.1)
    windows[(BIG, BIG_LEN - HALF)] = synth.make_ref(rng, HALF, 0.1)
    for (_, w0), (codes, _, _) in windows.items():
        big[w0:w0 + len(codes)] = np.frombuffer(_letters(codes).encode(), np.uint8)
    refs = {BIG: big.tobytes().decode()}
    for name in ("alpha", "zeta"):
        windows[(name, 0)] = synth.make_ref(rng, 5000, 0.1)
        refs[name] = _letters(windows[(name, 0)][0])
    ref_id = {n: k for k, (n, _) in enumerate(HEADER)}
    records = []

    def add(contig, w0, start, length, over=0, bad=False, place=None, clips=None):
        """a read by synth.make_read on [start, start + length) of the window that begins at w0: the window's n-polymers that
        begin in the slice, shifted to it; `over`: that many more bases of read and '=' behind the slice -- past the contig"""
        k = len(records)
        codes, np_starts, np_period = windows[(contig, w0)]
        lo = start - w0
        assert 0 <= lo and lo + length <= len(codes)
        keep = (np_starts >= lo) & (np_starts < lo + length)
        sq, cg = synth.make_read(rng, codes[lo:lo + length], np_starts[keep] - lo, np_period[keep], 0.3)
        runs, body = _runs(cg), _letters(sq)
        if over:
            assert start + length == len(refs[contig])
            runs, body = runs + [(7, over)], body + _letters(rng.integers(1, 5, over))
        if k % 7 == 3:
            body = body[:11] + "N" + body[12:40] + "R" + body[41:]
        lead, trail = fc.CLIPS[k % len(fc.CLIPS)] if clips is None else clips
        nl, nt = sum(n for op, n in lead if op == S), sum(n for op, n in trail if op == S)
        n = nl + len(body) + nt
        hp = fc.HP_TAGS[k % len(fc.HP_TAGS)]
        rec = dict(name=f"g{k}", flag=16 if k % 4 == 1 else 0, ref_id=ref_id[contig], pos=start, mapq=k % 61,
                   cigar=lead + runs + ([(M, 5)] if bad else []) + trail, seq="A" * nl + body + "C" * nt,
                   qual=None if k % 5 == 0 else bytes(rng.integers(0, 60, n).tolist()),
                   tags=fc.FRONT_TAGS[k % 4] + (hp or b"") + fc.BACK_TAGS[(k // 2) % 4], _hp=fc.HP_VALUES[k % len(fc.HP_TAGS)],
                   _place=place, _bad=bad, _over=over)
        # the mate: none, on the same contig (beyond 2^26 for the reads there), on another contig, unmapped with a distance kept
        if k % 4 == 1:
            rec.update(next_ref_id=ref_id[contig], next_pos=start + 100 + k, tlen=500 + k)
        elif k % 4 == 2:
            rec.update(next_ref_id=3 if contig == BIG else 1, next_pos=17 + k if contig == BIG else (1 << 26) + 1000 + k, tlen=0)
        elif k % 4 == 3:
            rec.update(next_ref_id=-1, next_pos=-1, tlen=-(300 + k))
        records.append(rec)

    lengths = {"a": 300, "b": 100, "c": 173, "d": 256, "e": 131, "f": 211}
    for j, b in enumerate(BORDERS):
        for which in PLACEMENTS:
            start, stop = placement(b, which, lengths[which] + 7 * j if which != "a" else 300)
            add(BIG, b - HALF, start, stop - start, place=(b, which))
    add(BIG, (1 << 20) - HALF, (1 << 20) + 700, 150, bad=True, clips=([], []))      # its CIGAR claims 5 bases more than it has
    add(BIG, BIG_LEN - HALF, BIG_LEN - 120, 120, over=25)
    add(BIG, BIG_LEN - HALF, BIG_LEN - 1500, 222)
    for name in ("alpha", "zeta"):
        for start, length in ((40, 180), (1234, 300), (4000, 100)):
            add(name, 0, start, length)
    add("alpha", 0, 4900, 100, over=30)
    records.sort(key=lambda r: (r["ref_id"], r["pos"]))
    w = windows[("alpha", 0)][0]
    decoy = [dict(name="onDecoy", flag=0, ref_id=2, pos=20, mapq=30, cigar=[(M, 100)], seq=_letters(w[:100]), qual=bytes(range(100)))]
    return HEADER, refs, records, decoy


def write_fasta(path, refs, order=FASTA_ORDER, width=80):
    """the contigs in `order`, lines of `width` bases (numpy: no loop over bases)"""
    with open(path, "wb") as fh:
        for name in order:
            a = np.frombuffer(refs[name].encode(), np.uint8)
            fh.write(b">" + name.encode() + b"\n")
            full = len(a) // width * width
            lines = np.empty((full // width, width + 1), np.uint8)
            lines[:, :width] = a[:full].reshape(-1, width)
            lines[:, width] = 10
            fh.write(lines.tobytes())
            if full < len(a):
                fh.write(a[full:].tobytes() + b"\n")
    return path


def plain(records):
    return [{k: v for k, v in r.items() if not k.startswith("_")} for r in records]


def write_inputs(tmp):
    """(main BAM, decoy BAM, FASTA) written under `tmp`, the main BAM with its .bai"""
    references, refs, records, decoy = case()
    bp, dp, fa = str(tmp / "genome.bam"), str(tmp / "decoy.bam"), str(tmp / "genome.fa")
    bam.write_bam(bp, references, plain(records))
    bam.write_bai(bp)
    bam.write_bam(dp, references, decoy)
    write_fasta(fa, refs)
    return bp, dp, fa


def whole_regions():
    """one region per contig of the FASTA, in header order"""
    return [(n, 0, l) for n, l in HEADER if n != "decoy"]


def ref_len(rec):
    return sum(n for op, n in rec["cigar"] if op in (M, D, N, 7, 8))


def overlapping(records, regions):
    """The overlap rule (bam.get_read_data; reference src/bam.pyx:18-47): region by region, in file order, the primary mapped
    reads with pos < stop and pos + reference length > start -- their indices in `records`."""
    ids = {n: k for k, (n, _) in enumerate(HEADER)}
    out = []
    for c, start, stop in regions:
        for k, r in enumerate(records):
            if r["ref_id"] == ids[c] and not r["flag"] & 0x904 and r["pos"] < stop and r["pos"] + ref_len(r) > start:
                out.append(k)
    return out


def region_sets():
    """[(what, [(contig, start, stop)])], each one region per contig in header order (what realign_sequential takes)"""
    return [("starts above 2^26", [(BIG, (1 << 26) + 1, BIG_LEN - 1)]),
            ("ends on 2^20, skips alpha", [(BIG, 0, 1 << 20), ("zeta", 0, 4999)]),
            ("from 2^23 to 2^26", [(BIG, 1 << 23, 1 << 26)]),
            ("alpha and the end of chrBig", [("alpha", 100, 4950), (BIG, BIG_LEN - 130, BIG_LEN + 100)])]


def range_sets(seed=3):
    """The range sets of the pileup counts: {name: [(contig, start, stop)]}.  `borders`: 1 500 positions on either side of every
    border in shuffled order, the whole of zeta, a range that leaves chrBig's end; `halves`: the same cut at the borders, so
    that ranges end and begin exactly there, and alpha from its middle past its end."""
    rng = np.random.default_rng(seed)
    around = [(BIG, b - 1500, b + 1500) for b in BORDERS]
    around = [around[k] for k in rng.permutation(len(around))]
    end = (BIG, BIG_LEN - 1700, BIG_LEN + 500)
    halves = [x for b in BORDERS for x in ((BIG, b, b + 1500), (BIG, b - 1500, b))]
    return {"borders": around + [("zeta", 0, 5000), end], "halves": [("alpha", 2500, 5100)] + halves + [end]}


# one range of 6.6e7 dense positions, for purity only (purity_window = 1 << 22, no per-position rows) ...
LONG_RANGE = (BIG, (1 << 20) - 1000, (1 << 26) + 1000)


def long_range_pieces():
    """... and the pieces of it that a read can touch: chrBig's reads lie inside the windows around the borders, so a position
    of LONG_RANGE outside them has no entry, and a position without an entry adds nothing to a histogram or a tally
    (purity_rec.hpp).  The pileup model is run on these 10 000 positions, not on 6.6e7 empty Python lists."""
    _, lo, hi = LONG_RANGE
    return [(BIG, max(lo, b - HALF), min(hi, b + HALF)) for b in BORDERS if b + HALF > lo and b - HALF < hi]

