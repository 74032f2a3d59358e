"""Inputs shared by tests/test_bam_eqx.py and tests/test_gpu_bam_eqx.py (--records full --eqx, NPORE_CIGAR_EQX): the table of the
rule's examples on raw code arrays, the readers the identities need, the crafted reads at which the device walk can go wrong --
besides those of bam_cs_cases, bam_md_cases and bam_full_cases, which the tests run as well --, the two reads on either side of
the CG threshold, and the statement's record stream.  Every expectation is written down from the rule (csrc/eqx_rec.hpp), not
from a run."""
import re

import numpy as np

from npore_amd import bam
import bam_cs_cases as cc
import bam_md_cases as mc
import long_cigar_cases as lc

M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
OPS = "MIDNSHP=X"

# (reference codes, read codes, final CIGAR, its =/X form) -- 'NACGT-' are the codes 0 ... 5; pinned by hand
TABLE = [
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 1, 2, 3, 4], "8M", "8="),                                        # all equal
    ([1, 2, 3, 4, 1, 2, 3, 4], [2, 2, 3, 4, 1, 2, 3, 4], "8M", "1X7="),                                      # a difference first
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 1, 2, 3, 1], "8M", "7=1X"),                                      # ... last
    ([1], [3], "1M", "1X"),                                                                                  # ... alone
    ([1, 2, 3, 4], [2, 3, 4, 1], "4M", "4X"),                                                                # ... everywhere
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 1, 2, 3, 4], "3=2X3M", "8="),                                    # one run through three words: the input's op is ignored
    ([1, 2, 3, 4], [1, 2, 4, 4], "2X2=", "2=1X1="),                                                          # ... either way
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 3, 4], "4M2N2M", "4=2N2="),                                      # N ends the stretch and is copied
    ([1, 2], [1, 2], "0M2M0I0D", "2="),                                                                      # words of length 0 are left out
    ([1, 2, 3, 4], [1, 2, 3, 4], "2M0I2M", "4="),                                                            # ... and end no stretch
    ([1, 2, 3], [4], "2D1I1D", "2D1I1D"),                                                                    # neighbouring I / D copied in order
    ([1, 2, 3, 4, 1, 2, 3, 4, 1, 2], [1, 2, 3, 4, 2, 4, 1, 2], "4M2D4M", "4=2D1X3="),
    ([1, 2, 3, 4, 1, 2, 3, 4], [1, 2, 3, 4, 4, 4, 1, 2, 3, 4], "4M2I4M", "4=2I4="),
    ([1, 2, 3, 4, 1, 2], [1, 2, 3, 1, 3, 2], "3M1I1D2M", "3=1I1D1X1="),                                         # the run on either side of a gap has its own class
    ([1, 0, 3, 5], [1, 0, 3, 5], "4M", "1=1X2="),                                                            # code 0 on 0 is X, code 5 on 5 is =
    ([0, 2, 5], [1, 2, 3], "3M", "1X1=1X"),                                                                  # code 0 in the reference
    ([1, 2, 3], [0, 2, 5], "3M", "1X1=1X"),                                                                  # ... in the read
    ([1, 2], [1, 2], "2M1D2M1I", "2=1D2X1I"),                                                                # positions beyond both arrays are X
    ([], [], "3M", "3X"),
    ([1, 2], [4, 4, 1, 2, 4], "1H2S1M1P1M1S", "1H2S1=1P1=1S"),                                               # S H P: copied, each ends the stretch
    ([], [1, 2, 3], "3I", "3I"),
    ([], [], "", ""),                                                                                        # the empty CIGAR
]


def runs_of(text):
    """[(op letter, len)] of a CIGAR text"""
    return [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def canonical_m(text):
    """the canonical M form: words of length 0 left out, = and X as M, neighbouring M words merged"""
    out = []
    for op, n in runs_of(text):
        if n == 0:
            continue
        op = "M" if op in "=X" else op
        if op == "M" and out and out[-1][0] == "M":
            out[-1][1] += n
        else:
            out.append([op, n])
    return "".join(f"{n}{op}" for op, n in out)


def eqx_identities(eqx, final, nm, cs_short=None):
    """The identities of the rule on one read's =/X form `eqx` of `final`"""
    got, src = runs_of(eqx), runs_of(final)
    assert "".join(f"{n}{op}" for op, n in got) == eqx and not any(op == "M" or n == 0 for op, n in got), eqx
    assert canonical_m(eqx) == canonical_m(final), (eqx, final)
    total = lambda runs, ops: sum(n for op, n in runs if op in ops)
    assert total(got, "ID") + total(got, "X") == nm, (eqx, nm)
    assert total(got, "=XDN") == total(src, "M=XDN") and total(got, "=XIS") == total(src, "M=XIS")      # reference and query consumed
    for (a, _), (b, _) in zip(got, got[1:]):
        assert not (a == b and a in "=X"), eqx                                                           # a run is maximal
    if cs_short is not None:
        toks = cc.parse_cs(cs_short)
        assert total(got, "=") == sum(int(p) for s, p in toks if s == ":") and total(got, "X") == sum(1 for s, _ in toks if s == "*"), (eqx, cs_short)


def record_cigar_text(rec):
    """(CIGAR text of a FULL record -- the CG tag's words where the record is long --, n_cigar_op as the record says it)"""
    import bam_full_cases as fc
    f, _, words, _, aux = fc.parse_full(rec)
    if f[5] == 2 and words[0] == (f[7] << 4 | S) and (words[1] & 15) == N:
        cg = [v for t, ty, v in mc.parse_tags(aux) if t == b"CG"]
        if cg:
            assert cg[0][:1] == b"I"
            words = list(np.frombuffer(cg[0][5:], "<u4"))
    return "".join(f"{int(w) >> 4}{OPS[int(w) & 15]}" for w in words), f[5]


def split_clips(text):
    """(the input's leading clip words H? S?, the words between, its trailing clip words S? H?) of a FULL record's CIGAR text"""
    return re.fullmatch(r"((?:\d+H)?(?:\d+S)?)(.*?)((?:\d+S)?(?:\d+H)?)", text).groups()


def without_outer_clips(text):
    return split_clips(text)[1]


_READS = {}


def eqx_reads(seed=31):
    """(references, refs, records, finals, {name: the =/X form pinned by hand}).  Computed once, shared, never changed.  The
    smallest shapes at which the device walk (csrc/bam_emit_kernels.hpp eqx_walk: tiles of 64 words, rounds of 64 positions) can
    go wrong: compared words of 1, 63, 64, 65, 128 and 129 positions with the class changing at the in-round offsets 0 and 63
    and at the first position of the next round; a run that crosses two round seams unbroken, one that ends exactly on a seam
    inside a word and one that ends on it with the word; 64 and 129 alternating positions (64 words out of one round); a
    stretch through three compared words, without and with changes; an I, a D and an N as the first word of a tile behind an
    open X run; (1M1I) x 150; names of 1 ... 4 letters; a refused read between two good ones; a read with no words; code 0 in
    the reference and in the read; a final past both arrays; clips H S ... S H."""
    if seed in _READS:
        return _READS[seed]
    rng = np.random.default_rng(seed)
    contig = list(lc.random_contig(rng, 30000))
    for p in (20003, 20007):
        contig[p] = "N"
    contig = "".join(contig)
    records, finals, pinned = [], [], {}

    def add(name, pos, runs, edits=(), clips=([], []), seq_sub=None, status=0, rec_cigar=None, final=None, tags=b""):
        """runs: the FINAL CIGAR as [(op, len)]; the read is the contig under it with `edits` (query offsets) substituted; the
        record's own CIGAR is the final one with = and X as M unless rec_cigar says otherwise"""
        seq, at = [], pos
        for op, ln in runs:
            if op in (M, EQ, X):
                seq += list(contig[at:at + ln])
            elif op == I:
                seq += list(lc.random_contig(rng, ln))
            if op in (M, EQ, X, D, N):
                at += ln
        for e in edits:
            seq[e] = mc.other(seq[e])
        for e, c in (seq_sub or {}).items():
            seq[e] = c
        nl, nt = sum(n for op, n in clips[0] if op == S), sum(n for op, n in clips[1] if op == S)
        own = rec_cigar if rec_cigar is not None else [(M if op in (EQ, X) else op, ln) for op, ln in runs]
        records.append(dict(name=name, flag=0, ref_id=0, pos=pos, mapq=40, seq="G" * nl + "".join(seq) + "T" * nt, cigar=clips[0] + list(own) + clips[1],
                            qual=bytes(rng.integers(0, 50, nl + len(seq) + nt).tolist()) if seq or nl or nt else None, tags=tags,
                            _status=status, _ctg="ctg"))
        finals.append(final if final is not None else "".join(f"{ln}{OPS[op]}" for op, ln in runs))

    def coded(classes):
        """the run-length code of a string over = and X"""
        return "".join(f"{len(m.group(0))}{m.group(0)[0]}" for m in re.finditer(r"=+|X+", classes))

    pos = 100
    for ln in (1, 63, 64, 65, 128, 129):                          # one compared word between two short ones
        offs = [o for o in (0, 63, 64, 127, 128) if o < ln]
        add(f"w{ln}", pos, [(M, 3), (I, 1), (M, ln), (D, 2), (M, 4)], edits=tuple(4 + o for o in offs), clips=([(S, 2)], []) if ln % 2 else ([], []))
        pinned[f"w{ln}"] = "3=1I" + coded("".join("X" if o in offs else "=" for o in range(ln))) + "2D4="
        pos += 300
    assert pinned["w129"] == "3=1I1X62=2X62=2X2D4=" and pinned["w64"] == "3=1I1X62=1X2D4=" and pinned["w1"] == "3=1I1X2D4="
    add("cross", pos, [(M, 200)], edits=(10, 150))               # the = run from 11 to 149 crosses the seams at 64 and 128
    pinned["cross"] = "10=1X139=1X49="
    add("on_seam", pos + 300, [(M, 130)], edits=(64,))           # the = run ends with the first round, inside the word
    pinned["on_seam"] = "64=1X65="
    add("on_seam_word", pos + 500, [(M, 128), (I, 1), (M, 2)])   # ... with the second round and the word
    pinned["on_seam_word"] = "128=1I2="
    add("x_over_seam", pos + 700, [(M, 70)], edits=tuple(range(60, 68)))      # an X run over the seam
    pinned["x_over_seam"] = "60=8X2="
    pos += 900
    add("alt64", pos, [(M, 64)], edits=tuple(range(0, 64, 2)))   # 64 words out of one round
    pinned["alt64"] = "1X1=" * 32
    add("alt129", pos + 100, [(EQ, 129)], edits=tuple(range(1, 129, 2)), clips=([(H, 1)], [(S, 3)]))
    pinned["alt129"] = "1=1X" * 64 + "1="
    add("three_words", pos + 300, [(EQ, 70), (X, 64), (M, 5)])
    pinned["three_words"] = "139="
    add("three_changes", pos + 500, [(EQ, 40), (X, 30), (M, 30)], edits=(39, 40, 70))
    pinned["three_changes"] = "39=2X29=1X29="
    pos += 700
    # words 1 ... 64: (2M 1I) x 31, 1M, 1X, whose last position differs -- an X run is open where the tile ends; word 65 is copied
    front = [(M, 2), (I, 1)] * 31 + [(M, 1), (X, 1)]
    for k, nxt in enumerate(((I, 3), (D, 3), (N, 4))):
        runs = front + [nxt, (M, 5)]
        nq, nr = 3 * 31 + 2 + (3 if nxt[0] == I else 0) + 5, 2 * 31 + 2 + (0 if nxt[0] == I else nxt[1]) + 5
        add(f"tile_{OPS[nxt[0]]}", pos, runs, edits=(3 * 31 + 1,), rec_cigar=[(M, nr), (I, nq - nr)] if nxt[0] == N else None)
        pinned[f"tile_{OPS[nxt[0]]}"] = "2=1I" * 31 + f"1=1X{nxt[1]}{OPS[nxt[0]]}5="
        pos += 200
    add("mi150", pos, [(M, 1), (I, 1)] * 150)
    pinned["mi150"] = "1=1I" * 150
    pos += 300
    for k, name in enumerate(("e", "eq", "eqx", "eqx4")):        # the CIGAR field at every byte alignment
        add(name, pos, [(M, 9)], edits=(4,), clips=([(S, 1)], []))
        pinned[name] = "4=1X4="
        pos += 50
    add("refused_before", pos, [(M, 30)], edits=(3,))
    add("refused", pos + 10, [(M, 30)], status=32)
    add("refused_after", pos + 20, [(M, 30)], edits=(4,))
    pinned["refused_before"], pinned["refused_after"] = "3=1X26=", "4=1X25="
    add("no_words", pos + 100, [(M, 10)], final="", clips=([(S, 2)], []))
    pinned["no_words"] = ""
    add("clips", pos + 200, [(M, 10), (I, 2), (M, 10)], edits=(0, 21), clips=([(H, 3), (S, 2)], [(S, 4), (H, 1)]))
    pinned["clips"] = "1X9=2I9=1X"
    add("n_in_ref", 20000, [(M, 5), (D, 4), (M, 6)])             # contig N at 20003 (under M) and 20007 (under D)
    pinned["n_in_ref"] = "3=1X1=4D6="
    add("n_in_read", 20100, [(M, 6), (I, 3), (M, 6)], seq_sub={2: "N", 7: "R", 11: "N"})      # (7: under I)
    pinned["n_in_read"] = "2=1X3=3I2=1X3="
    # the record covers 20 reference bases and has 20 read bases; the final names 27 and 33
    add("past_end", 20200, [(M, 20)], final="18M3I4M2D1M5I")
    pinned["past_end"] = "18=3I4X2D1X5I"
    both = sorted(zip(records, finals), key=lambda rf: rf[0]["pos"])
    out = ([("ctg", len(contig))], {"ctg": contig}, [r for r, _ in both], [f for _, f in both], pinned)
    _READS[seed] = out
    return out


_CG = {}


def cg_reads(seed=37):
    """(references, refs, records, finals): two reads whose M form is ONE word and whose every second base differs, between two
    clip words -- 65 533 positions: 65 535 operations, the most n_cigar_op holds; 65 534 positions: 65 536, the first CIGAR
    that goes to the CG tag.  Computed once, shared, never changed."""
    if seed in _CG:
        return _CG[seed]
    rng = np.random.default_rng(seed)
    contig = lc.random_contig(rng, 140000)
    records, finals = [], []
    for name, pos, ln in (("cg65535", 100, 65533), ("cg65536", 70000, 65534)):
        seq = list(contig[pos:pos + ln])
        for e in range(1, ln, 2):
            seq[e] = mc.other(seq[e])
        records.append(dict(name=name, flag=0, ref_id=0, pos=pos, mapq=40, seq="G" + "".join(seq) + "TT", cigar=[(S, 1), (M, ln), (S, 2)], qual=None,
                            tags=b"RGZgrp\0", _status=0, _ctg="ctg"))
        finals.append(f"{ln}M")
    out = ([("ctg", len(contig))], {"ctg": contig}, records, finals)
    _CG[seed] = out
    return out


def want_stream(raws, records, contigs, finals, status, md=False, cs=None, de=False, eqx=True):
    """bam.full_record(md=, cs=, de=, eqx=) of every kept read, one after the other"""
    out = []
    for raw, rec, fin, st in zip(raws, records, finals, status):
        if st & 32:
            continue
        rc, sc, _ = lc.expected_pack(rec, rec["cigar"], contigs[rec.get("_ctg", "ctg")])
        out.append(bam.full_record(raw, rc, sc, fin, md=md, cs=cs, de=de, eqx=eqx))
    return b"".join(out)
