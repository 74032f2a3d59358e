"""Inputs shared by tests/test_bam_oc.py and tests/test_gpu_bam_oc.py (--records full --oc, NPORE_TAG_OC): the table of the rule's
examples, crafted records with their finals at which the device's decision and walk (csrc/bam_emit_kernels.hpp oc_changed,
oc_walk: tiles of 64 words of the read's real CIGAR, word c in lane c % 64 of tile c // 64) can go wrong, the reads with more than
65 535 words on either side, a file of short reads for the pipeline, and the statement's record stream.  Every expectation
-- changed or not, the OC text -- is written down from the rule (csrc/oc_rec.hpp), not from a run."""
import re

import numpy as np

from npore_amd import bam
import long_cigar_cases as lc

M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
OPS = "MIDNSHP=X"
OC = 256                                                         # NPORE_TAG_OC

# (the input's CIGAR, its final CIGAR, changed?, the OC text a changed read gets) -- pinned by hand
TABLE = [
    ("10M2I10M", "10M2I10M", False, None),                                              # equal
    ("5=1X4=2I0D3M2M", "10M2I5M", False, None),                                         # equal up to =/X form, 0-length and split words
    ("3M2M", "5M", False, None),
    ("3M0I2M", "5M", False, None),
    ("3=2X", "5M", False, None),
    ("10M1I1D10M", "21M", True, "10M1I1D10M"),                                          # an input 1I1D where the final has M
    ("10M1I1D10M", "10M1I1D10M", False, None),                                          # ... and where it has not
    ("10M2I10M", "10M2I11M", True, "10M2I10M"),                                         # the last word's length only
    ("10M2I10M", "10M2I", True, "10M2I10M"),                                            # the final one word shorter, equal prefix
    ("10M2I10M", "10M2I10M1I", True, "10M2I10M"),                                       # ... one word longer
    ("10M2I10M", "10M2D10M", True, "10M2I10M"),                                         # an op
    ("2H3S5M0I5=1S4H", "10M", False, None),                                             # clips of both kinds on either end are no part of it
    ("2H3S5M0I5=1S4H", "4M1I5M", True, "2H3S5M0I5=1S4H"),                               # ... but of the text, as is the word of length 0
    ("3S7M", "3S7M", True, "3S7M"),                                                     # (a final is taken as it stands: it has no clips)
    ("5M", "2M3M", True, "5M"),                                                         # (... and is no canonical form when it is split)
    ("0M", "", False, None),                                                            # nothing against nothing
    ("", "", False, None),
    ("5M", "", True, "5M"),
    ("268435455H1M1P1N1M", "1M1P1N1M", False, None),                                    # P and N are words like any other
    ("268435455H1M1P1N1M", "2M", True, "268435455H1M1P1N1M"),
]


def runs_of(text):
    """[(op, len)] of a CIGAR text"""
    return [(OPS.index(op), int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def text_of(runs):
    return "".join(f"{n}{OPS[op]}" for op, n in runs)


def clip_range(cigar):
    """(i, j): the clip words are [0, i) and [j, n) -- lead H? S?, trail S? H? over what the lead left (csrc/bam_reader.hpp
    full_clip_words)"""
    i, j = 0, len(cigar)
    if i < j and cigar[i][0] == H:
        i += 1
    if i < j and cigar[i][0] == S:
        i += 1
    if j > i and cigar[j - 1][0] == H:
        j -= 1
    if j > i and cigar[j - 1][0] == S:
        j -= 1
    return i, j


def inner(cigar):
    """the words between the clip words"""
    i, j = clip_range(cigar)
    return cigar[i:j]


def parse_tags(aux):
    """[(tag, type, value bytes)] of a record's aux bytes"""
    import bam_md_cases as mc
    return mc.parse_tags(aux)


def oc_of_record(rec):
    """(the texts of the record's OC tags, the names of all its tags in order)"""
    import bam_full_cases as fc
    tags = parse_tags(fc.parse_full(rec)[4])
    return [v[:-1].decode() for t, _, v in tags if t == b"OC"], [t for t, _, _ in tags]


def alternating(n, first=M):
    """n words M 2 / I 1 in turn: no two neighbours merge, so the canonical form is the words themselves"""
    ops = (first, I if first == M else M)
    return [(ops[k % 2], 2 if ops[k % 2] == M else 1) for k in range(n)]


_READS = {}


def oc_reads(seed=41):
    """(references, refs, records, finals, {name: changed?}, {name: OC text pinned by hand}).  Computed once, shared, never
    changed.  A record's `cigar` is its input CIGAR; without clip words, word c lies in lane c % 64 of tile c // 64."""
    if seed in _READS:
        return _READS[seed]
    rng = np.random.default_rng(seed)
    contig = lc.random_contig(rng, 60000)
    records, finals, changed, pinned = [], [], {}, {}
    state = dict(pos=100)

    def add(name, cigar, final, is_changed, text=None, tags=b"", status=0, flag=0):
        """cigar: the INPUT CIGAR [(op, len)], clip words included; final: its final CIGAR as text or as [(op, len)]; the read is
        the contig under the input CIGAR"""
        pos, at, seq = state["pos"], state["pos"], []
        for op, ln in cigar:
            if op in (M, EQ, X):
                seq += list(contig[at:at + ln])
            elif op in (I, S):
                seq += list(lc.random_contig(rng, ln))
            if op in (M, EQ, X, D, N):
                at += ln
        records.append(dict(name=name, flag=flag, ref_id=0, pos=pos, mapq=30, seq="".join(seq), cigar=list(cigar),
                            qual=bytes(rng.integers(0, 50, len(seq)).tolist()) if seq else None, tags=tags, _status=status, _ctg="ctg"))
        finals.append(final if isinstance(final, str) else text_of(final))
        changed[name] = is_changed
        if text is not None:
            pinned[name] = text
        state["pos"] = at + 20

    # ---- the table's rows as records: those a file can hold as reads -- some bases, no N or P in the input, no clip in the final
    for k, (cig, fin, chg, text) in enumerate(TABLE):
        if re.search(r"[1-9]\d*[MI=X]", cig) and not re.search(r"[NP]", cig) and not re.search(r"[SH]", fin):
            add(f"t{k}", runs_of(cig), fin, chg, text)
    # ---- tile edges: 1, 63, 64, 65, 128 and 129 words, equal, and different in the last word's length only
    for n in (1, 63, 64, 65, 128, 129):
        w = alternating(n)
        add(f"n{n}_same", w, w, False)
        add(f"n{n}_last", w, w[:-1] + [(w[-1][0], w[-1][1] + 1)], True)
    # the final one word shorter / longer than the input with an equal prefix, across the first tile's end
    w = alternating(65)
    add("shorter_64", w, w[:64], True)
    add("longer_66", w, w + [(I, 3)], True)
    w = alternating(64)
    add("longer_65", w, w + [(M, 3)], True)
    add("shorter_63", w, w[:63], True)
    # a merged run that straddles a tile edge: M in lane 63, = in lane 0 of the next tile
    w = alternating(63, first=I) + [(M, 3), (EQ, 4), (I, 2)] + alternating(30)      # (word 62 is I)
    canon = w[:63] + [(M, 7)] + w[65:]
    add("straddle", w, canon, False)
    add("straddle_off", w, w[:63] + [(M, 6)] + w[65:], True)     # different only in what the second tile adds to the run
    add("straddle_split", w, w[:63] + [(M, 3), (M, 4)] + w[65:], True)
    # a word of length 0 in lanes 0 and 63
    w = [(I, 0)] + alternating(62) + [(D, 0)] + alternating(10)      # (word 62 is I, word 64 M)
    add("zero_edges", w, [x for x in w if x[1]], False)
    add("zero_edges_off", w, [x for x in w if x[1]][:-1] + [(I, 7)], True)
    # a whole tile of words of length 0 between an M in lane 63 and an M in lane 0: ONE run through it
    w = alternating(64, first=I) + [((0, 1, 2, 3, 6, 7, 8)[k % 7], 0) for k in range(64)] + [(M, 5), (I, 1), (M, 2)]
    add("zero_tile", w, w[:63] + [(M, 7), (I, 1), (M, 2)], False)
    add("zero_tile_off", w, w[:63] + [(M, 2), (M, 5), (I, 1), (M, 2)], True)
    # a run merged across three tiles: words 62 ... 192 are M = X of length 1 with words of length 0 among them
    run = [((M, EQ, X)[k % 3], 1) if k % 5 else (I, 0) for k in range(131)]
    n_run = sum(ln for _, ln in run)
    w = alternating(62, first=I) + run + [(I, 1), (M, 2)]
    add("three_tiles", w, w[:61] + [(M, 2 + n_run), (I, 1), (M, 2)], False)
    add("three_tiles_off", w, w[:61] + [(M, 1 + n_run), (I, 1), (M, 2)], True)
    # different only in the second tile
    w = alternating(100)
    add("second_tile", w, w[:80] + [(M, 3)] + w[81:], True)
    add("second_tile_op", w, w[:81] + [(D, 1)] + w[82:], True)
    # ---- clips of every kind on either end, changed and unchanged in turn
    k = 0
    for lead in ([], [(H, 2)], [(S, 3)], [(H, 2), (S, 3)]):
        for trail in ([], [(H, 5)], [(S, 1)], [(S, 1), (H, 5)]):
            body = [(M, 10), (I, 1), (D, 1), (EQ, 12)]
            chg = k % 2 == 0
            add(f"clip{k}", lead + body + trail, "23M" if chg else "10M1I1D12M", chg, text_of(lead + body + trail) if chg else None)
            k += 1
    # ---- decimal widths: 1 ... 9 digits, up to a hard clip of 2^28 - 1 (H consumes nothing)
    widths = [1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, (1 << 28) - 1]
    for a, b in zip(widths[0::2], widths[1::2]):
        cig = [(H, a), (M, 10), (I, 1), (D, 1), (M, 10), (H, b)]
        add(f"d{a}", cig, "21M", True, f"{a}H10M1I1D10M{b}H")
    add("d_inner", [(M, 9), (I, 10), (M, 99), (D, 100), (M, 101)], "9M10I200M100D", True, "9M10I99M100D101M")
    # ---- an input that carries OC already, once changed and once unchanged; another tag on either side of it
    own = b"XAZbefore\0" + b"OCZ7M7I\0" + b"XBi" + (5).to_bytes(4, "little")
    add("has_oc_changed", [(M, 10), (I, 2), (M, 10)], "10M2I11M", True, "10M2I10M", tags=own)
    add("has_oc_same", [(M, 10), (I, 2), (M, 10)], "10M2I10M", False, tags=own)
    # ---- a refused read between two good ones
    add("refused_before", [(M, 30)], "29M1I", True, "30M")
    add("refused", [(M, 30)], "30M", False, status=32)
    add("refused_after", [(S, 1), (M, 30)], "15M1I14M", True, "1S30M")
    # ---- a record that passes under a mask (secondary) and has an OC of its own; without a mask it is a read like any other
    add("secondary", [(M, 20)], "19M1I", True, "20M", tags=b"OCZ3M17I\0", flag=0x100)
    # ---- names of 1 ... 8 bytes: the tag at every alignment
    for n in range(1, 9):
        add("abcdefgh"[:n], [(S, n % 3)] * (n % 3 > 0) + [(M, 12)], "6M1I5M", True, (f"{n % 3}S" if n % 3 else "") + "12M")
    out = ([("ctg", len(contig))], {"ctg": contig}, records, finals, changed, pinned)
    _READS[seed] = out
    return out


_LONG = {}


def long_reads(seed=43, units=33000):
    """(references, refs, records, finals, {name: changed?}): inputs of 2 * units > 65 535 words, (1M 1I) x units, which lie in the
    file as placeholder + CG tag -- `cg_in`, whose final is short, so its OC text comes from the CG tag's words and the record is
    plain; `cg_same`, whose final is its input (no OC; CG out); `cg_both`, whose final differs in the last word only: OC and CG,
    in that order.  Computed once, shared, never changed."""
    if seed in _LONG:
        return _LONG[seed]
    rng = np.random.default_rng(seed)
    contig = lc.random_contig(rng, 3 * units + 1000)
    cigar = [(M, 1), (I, 1)] * units
    records, finals, changed = [], [], {}
    for k, (name, fin, chg) in enumerate((("cg_in", f"{units}M{units}I", True), ("cg_same", text_of(cigar), False),
                                          ("cg_both", text_of(cigar[:-1] + [(I, 2)]), True))):
        pos = 100 + k * units
        seq = np.empty(2 * units, "U1")
        seq[0::2] = list(contig[pos:pos + units])
        seq[1::2] = list(lc.random_contig(rng, units))
        records.append(dict(name=name, flag=0, ref_id=0, pos=pos, mapq=40, seq="".join(seq), cigar=list(cigar), qual=None, tags=b"RGZgrp\0",
                            _status=0, _ctg="ctg"))
        finals.append(fin)
        changed[name] = chg
    out = ([("ctg", len(contig))], {"ctg": contig}, records, finals, changed)
    _LONG[seed] = out
    return out


_PIPE = {}


def pipeline_reads(seed=47, n_reads=40):
    """(references, refs, records): about 40 reads of 100 - 160 bases for the file pipeline -- every other one matches the
    contig base for base under `nM`; the others have lost one base of a homopolymer of five, and their input CIGAR places the
    deletion at the run's RIGHT end, which the standardisation moves to its left end.  Four of them carry flags that
    --pass_through passes (with an OC of their own), two an OC that a changed read replaces and an unchanged one loses."""
    if seed in _PIPE:
        return _PIPE[seed]
    rng = np.random.default_rng(seed)
    contig, at_runs = [], []
    for k in range(n_reads):
        contig += list(lc.random_contig(rng, 100))
        base = "ACGT"[k % 4]
        while contig[-1] == base:
            contig.pop()
        at_runs.append(len(contig))
        contig += [base] * 5
        nxt = lc.random_contig(rng, 100)
        while nxt[0] == base:
            nxt = nxt[1:]
        contig += list(nxt)
    contig = "".join(contig)
    records = []
    for k in range(n_reads):
        run = at_runs[k]
        pos, a, b = run - 50 - k % 7, 50 + k % 7, 40 + k % 11      # a bases in front of the homopolymer, b behind it
        if k % 2 == 0:
            seq, cigar = contig[pos:pos + a + 5 + b], [(M, a + 5 + b)]
        else:
            seq, cigar = contig[pos:pos + a + 4] + contig[run + 5:run + 5 + b], [(M, a + 4), (D, 1), (M, b)]
        if k % 5 == 0:
            cigar = [(S, 2)] + cigar
            seq = "GG" + seq
        tags = b"OCZ1M\0" if k in (2, 3) else b""
        flag = 0
        if k in (10, 11, 20, 21):
            flag, tags = (0x100 if k < 20 else 0x800), b"OCZ9M9I\0" + b"NMC\x01"
        records.append(dict(name=f"p{k}", flag=flag, ref_id=0, pos=pos, mapq=50, seq=seq, cigar=cigar, qual=bytes(rng.integers(5, 45, len(seq)).tolist()),
                            tags=tags, _ctg="ctg"))
    out = ([("ctg", len(contig))], {"ctg": contig}, records)
    _PIPE[seed] = out
    return out


def oracle_finals(records, refs, tables, r=30, max_b_rows=20000):
    """the reference's final CIGARs of the records: its align() through the oracle, its standardisation and collapse"""
    import oracle
    from npore_amd import cig
    sub, nps = tables
    out = []
    for rec in records:
        rc, sc, ops = lc.expected_pack(rec, rec["cigar"], refs[rec["_ctg"]])
        raw = oracle.align(rc, sc, ops.decode(), sub, nps, r=r, max_b_rows=max_b_rows)
        out.append(cig.collapse_cigar(cig.standardize(raw, rc, sc)))
    return out


def want_stream(raws, records, contigs, finals, status, mask=0, oc=True, **kw):
    """bam.full_record(oc=, ...) of every kept read, a record that passes under `mask` as it came, one after the other"""
    out = []
    for raw, rec, fin, st in zip(raws, records, finals, status):
        if st & 32:
            continue
        if rec["flag"] & mask:
            out.append(raw)
            continue
        rc, sc, _ = lc.expected_pack(rec, rec["cigar"], contigs[rec.get("_ctg", "ctg")])
        out.append(bam.full_record(raw, rc, sc, fin, oc=oc, **kw))
    return b"".join(out)
