"""Inputs shared by tests/test_bam_fuzz.py and tests/test_gpu_bam_fuzz.py: reads whose input AND final CIGARs are random, for the
whole record chain of --records full (csrc/bam_emit_kernels.hpp: NM, MD, cs / de, the =/X form, OC) under every option set; a
report of which reads hit which seam of the device walks, computed from the inputs alone; the tag texts of a read computed once
and records assembled from them as bam.full_record assembles them; and one crafted read that is long only through the =/X split.

What the walks carry, and where (bam_emit_kernels.hpp): a FINAL CIGAR is walked in tiles of 64 words, word c in lane c % 64 of
tile c // 64, a compared word in rounds of 64 positions from the word's first position; md_walk and cs_walk carry the count `u`,
eqx_walk the open run (`run`, `cls`).  oc_changed walks the INPUT's real CIGAR in tiles of 64 words, the clip words counted (word
c of the record in lane c % 64), and carries the open run (`rop`, `rlen`, `runs`).

The seeds in SEEDS were picked on the CPU so that every situation of SITUATIONS occurs at least once in each of them
(tests/test_bam_fuzz.py asserts it)."""
import struct

import numpy as np

from npore_amd import bam
import bam_full_cases as fc
import bam_md_cases as mc
import bam_oc_cases as oc
import long_cigar_cases as lc

M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
OPS = "MIDNSHP=X"
COMPARED = (M, EQ, X)
SEEDS = (101, 104, 108)
N_READS = 100
WORD_COUNTS = (1, 2, 5, 63, 64, 65, 127, 128, 129, 200)
EDGE_LENS = (63, 64, 65, 127, 128, 129)
# the 48 option sets, md slowest, oc fastest (tests/model/record_bounds.cpp prints its sums in this order)
OPTION_SETS = [dict(md=md, cs=cs, de=de, eqx=eqx, oc=o) for md in (False, True) for cs in (None, "short", "long") for de in (False, True)
               for eqx in (False, True) for o in (False, True)]
EMPTY_SET = OPTION_SETS[0]
FULL_SET = dict(md=True, cs="long", de=True, eqx=True, oc=True)
# six sets for the runs under a pass mask: every option is on in at least two of them and off in at least two
MASK_SETS = [dict(md=True, cs=None, de=False, eqx=False, oc=True), dict(md=False, cs="short", de=True, eqx=True, oc=False),
             dict(md=True, cs="long", de=True, eqx=True, oc=True), dict(md=False, cs=None, de=False, eqx=False, oc=False),
             dict(md=False, cs="long", de=False, eqx=True, oc=True), dict(md=True, cs="short", de=True, eqx=False, oc=False)]


def set_name(kw):
    return "+".join(([("md")] if kw["md"] else []) + ([f"cs_{kw['cs']}"] if kw["cs"] else []) + [k for k in ("de", "eqx", "oc") if kw[k]]) or "none"


def canonical(words):
    """the canonical form of input words [(op, len)] (csrc/oc_rec.hpp): words of length 0 dropped, = and X read as M, neighbours of
    equal op merged"""
    out = []
    for op, n in words:
        if n == 0:
            continue
        op = M if op in (EQ, X) else op
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + n)
        else:
            out.append((op, n))
    return out


def _lengths(rng, n, cap):
    """n lengths, log-uniform in 1 ... cap; about 15 % set to a round's edges, about 8 % to 0"""
    ln = np.minimum(cap, np.exp(rng.uniform(0, np.log(cap + 1), n)).astype(np.int64))
    u = rng.random(n)
    ln[u < 0.15] = rng.choice(EDGE_LENS, int((u < 0.15).sum()))
    ln[(u >= 0.15) & (u < 0.23)] = 0
    return ln.tolist()


def _n_words(rng):
    return int(rng.choice(WORD_COUNTS)) if rng.random() < 0.5 else int(rng.integers(1, 261))


def _words(rng, n, ops):
    return list(zip(rng.choice(ops, n).tolist(), _lengths(rng, n, 40 if n > 60 else 200))) if n else []


def _near_miss(rng, canon):
    """`canon` with one near miss: a length + 1, an op changed, a word removed or a word of length 1 put in -- at the last word, the
    first word, the first word of a tile or anywhere"""
    w = list(canon)
    n, u = len(w), rng.random()
    tiles = list(range(64, n, 64))
    at = n - 1 if u < 0.3 else 0 if u < 0.45 else int(rng.choice(tiles)) if u < 0.75 and tiles else int(rng.integers(n))
    how = int(rng.integers(4))
    if how == 0:
        w[at] = (w[at][0], w[at][1] + 1)
    elif how == 1:
        w[at] = (int(rng.choice([o for o in (M, I, D) if o != w[at][0]])), w[at][1])
    elif how == 2:
        del w[at]
    else:
        w.insert(at + int(rng.integers(2)), (int(rng.choice((M, I, D))), 1))
    return w


def _relettered(rng, words):
    """the words with every op replaced by one that consumes the same: the walk stays in register with the bases"""
    same = {M: (M, EQ, X), EQ: (M, EQ, X), X: (M, EQ, X), I: (I, S), D: (D, N), P: (P, H)}
    return [(int(rng.choice(same[op])), n) for op, n in words]


_READS = {}


def fuzz_reads(seed):
    """(references, refs, records, finals, status): about 100 reads in coordinate order on one contig with a few dozen N bases.
    Computed once per seed, shared, never changed.  A record's `cigar` is its INPUT CIGAR.  Read k's final is of kind k % 4:
    0 the input's canonical form (unchanged); 1 that form with one near miss; 2 the input's words as they stand, = / X and words of
    length 0 included; 3 unrelated words over all nine ops, or (every other time) the input's words re-lettered -- D as N, I as S,
    P as H, M as = or X -- with the tail cut or unrelated words behind them, so that a final runs past either array or stops
    short of it."""
    if seed in _READS:
        return _READS[seed]
    rng = np.random.default_rng(seed)
    shapes, pos = [], 50
    for k in range(N_READS):
        n = _n_words(rng)
        words = _words(rng, n, (M, I, D, EQ, X, P))
        lead, trail = fc.CLIPS[int(rng.integers(len(fc.CLIPS)))]
        ci = len(lead)
        marked = set()                                           # compared words whose last base differs
        if n > 64 and rng.random() < 0.5:                        # a compared word in lane 63 of the final, an I or a D in lane 0 behind it
            for s in range(64, n, 64):
                if rng.random() < 0.5:
                    marked.add(ci + s - 1)
                words[s - 1] = (int(rng.choice(COMPARED)), max(1, words[s - 1][1]))
                words[s] = (int(rng.choice((I, D))), max(1, words[s][1]))
        if n >= 70 and rng.random() < 0.3:                       # a word of length 0 in lane 63 or lane 0 of the input
            c = 63 - ci + int(rng.integers(2))
            words[c] = (words[c][0], 0)
        if n >= 129 and rng.random() < 0.3:                      # a whole tile of the input, words 64 ... 127 of the record, of length 0
            for c in range(64 - ci, 128 - ci):
                words[c] = (words[c][0], 0)
        if not any(ln for op, ln in words if op in (M, I, EQ, X)):
            words[0] = (M, 7)                                    # (a read has bases)
        shapes.append((words, lead, trail, pos, marked))
        pos += int(rng.integers(0, 300))
    end = max(p + lc.ref_len(w) for w, _, _, p, _ in shapes)
    arr = rng.integers(1, 5, end + 100).astype(np.uint8)
    arr[rng.integers(50, end, 40)] = 0                           # N
    contig = "".join("NACGT"[x] for x in arr)
    records, finals = [], []
    for k, (words, lead, trail, pos, marked) in enumerate(shapes):
        sub = 0.5 if k % 5 == 0 else 0.05
        seq, at = [], pos
        for c, (op, ln) in enumerate(lead + words + trail):
            if op in COMPARED:
                piece = arr[at:at + ln].copy()
                hit = rng.random(ln) < sub
                if c in marked and ln:
                    hit[-1] = True
                piece[hit] = (piece[hit] + rng.integers(0, 3, int(hit.sum()))) % 4 + 1      # (another letter)
                seq.append(piece)
            elif op in (I, S):
                seq.append(rng.integers(1, 5, ln).astype(np.uint8))
            if op in lc.CONSUMES_REF:
                at += ln
        seq = "".join("NACGT"[x] for x in np.concatenate(seq))
        tags = fc.FRONT_TAGS[k % 4] + (b"OCZ5M1I\0" if k % 6 == 0 else b"") + fc.BACK_TAGS[(k // 2) % 4]
        rec = dict(name="q" * (k % 6) + str(k), flag={3: 16, 5: 0x100, 6: 0x800, 8: 0x4, 9: 16}.get(k % 10, 0), ref_id=0, pos=pos,
                   mapq=int(rng.integers(0, 61)), seq=seq, cigar=lead + words + trail,
                   qual=None if k % 7 == 2 else bytes(rng.integers(0, 50, len(seq)).tolist()), tags=tags,
                   _status=32 if k in (11, 37, 70) else 0, _ctg="ctg")
        if k % 3 == 1:
            rec.update(next_ref_id=0, next_pos=pos + 100 + k, tlen=500 + k)
        records.append(rec)
        canon = canonical(words)
        if k % 4 == 0:
            fin = canon
        elif k % 4 == 1:
            fin = _near_miss(rng, canon)
        elif k % 4 == 2:
            fin = words
        elif k % 8 == 3:
            fin = _words(rng, 0 if k % 40 == 3 else _n_words(rng), tuple(range(9)))
            if rng.random() < 0.5:                               # an I, a D or an N in lane 0 behind a compared word in lane 63
                for s in range(64, len(fin), 64):
                    fin[s - 1] = (int(rng.choice(COMPARED)), max(1, fin[s - 1][1]))
                    fin[s] = (int(rng.choice((I, D, N))), max(1, fin[s][1]))
        else:
            fin, u = _relettered(rng, words), rng.random()
            if u < 1 / 3:
                fin = fin[:int(rng.integers(len(fin) + 1))]
            elif u < 2 / 3:
                fin = fin + _words(rng, int(rng.integers(1, 11)), tuple(range(9)))
        finals.append(oc.text_of(fin))
    out = ([("ctg", len(contig))], {"ctg": contig}, records, finals, np.array([r["_status"] for r in records], np.int32))
    _READS[seed] = out
    return out


_PACKS = {}


def fuzz_packs(seed):
    """[(reference codes, read codes)] of the seed's reads, as the pack makes them (lc.expected_pack); computed once"""
    if seed not in _PACKS:
        _, refs, records, _, _ = fuzz_reads(seed)
        _PACKS[seed] = [lc.expected_pack(r, r["cigar"], refs["ctg"])[:2] for r in records]
    return _PACKS[seed]


# ---- which reads hit which seam: from the inputs alone, no library call, no output ----------------------------------------------------
SITUATIONS = (["compared_run_over_tile_seam"] + [f"tile_first_{o}_behind_open_{c}" for o in "IDN" for c in ("X", "EQ")] +
              ["zero_word_final_lane0", "zero_word_final_lane63", "zero_word_input_lane0", "zero_word_input_lane63", "zero_tile_of_input",
               "input_run_merges_over_tile_seam", "near_miss_last_word", "near_miss_first_word", "near_miss_first_word_of_a_tile",
               "final_fewer_words", "final_more_words", "unchanged", "changed", "md_count_10_over_round_seam", "md_count_100_over_round_seam",
               "cs_count_10_over_round_seam", "cs_count_100_over_round_seam", "nm_one_byte", "nm_two_bytes", "final_past_reference",
               "final_past_read", "final_short_of_reference", "final_short_of_read", "empty_final", "refused", "passes_under_0x904",
               "own_oc_tag", "no_qualities"] + [f"clip_shape_{j}" for j in range(len(fc.CLIPS))] + [f"head_offset_mod8_{j}" for j in range(8)])


def _differs(rc, sc, a, b, n):
    """which of n compared positions from (a, b) differ (csrc/nm_rec.hpp nm_differs: a position beyond an array has code 0)"""
    r, s = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    k = max(0, min(n, len(rc) - a))
    r[:k] = rc[a:a + k]
    k = max(0, min(n, len(sc) - b))
    s[:k] = sc[b:b + k]
    return (r != s) | (r == 0) | (s == 0)


def _count_seams(fin, rc, sc, closers):
    """(a count of 10 or more, a count of 100 or more) written from a stretch that was below it where a round of 64 positions of a
    compared word ended: the carried count changes its number of digits.  closers: the ops that end a stretch besides a
    differing position (MD: D; cs: I, D, N)."""
    hit, u, carried, a, b = [False, False], 0, [], 0, 0

    def close(c):
        for lim, j in ((10, 0), (100, 1)):
            hit[j] = hit[j] or any(0 < v < lim <= c for v in carried)
        carried.clear()
    for op, ln in fin:
        if op in COMPARED and ln:
            d = _differs(rc, sc, a, b, ln)
            for q0 in range(0, ln, 64):
                ev = np.flatnonzero(d[q0:q0 + 64])
                n_round = min(64, ln - q0)
                if len(ev):
                    close(u + int(ev[0]))
                    u = n_round - 1 - int(ev[-1])
                else:
                    u += n_round
                carried.append(u)
        elif op in closers and ln:
            close(u)
            u = 0
        if op in (M, EQ, X, D, N):
            a += ln
        if op in (M, EQ, X, I, S):
            b += ln
    close(u)
    return hit


def staged_full_head_bytes(rec):
    """the bytes of a read's staged FULL head (csrc/hostio.hpp staged heads: block_size word, fixed fields, name with its NUL, CIGAR
    words, 4-bit bases, qualities, the kept aux bytes) under no option oc; a CIGAR of more than 65 535 words is not modelled"""
    l_seq = sum(n for op, n in rec["cigar"] if op in lc.CONSUMES_QUERY)      # (the bases the CIGAR consumes: a record's l_seq)
    return 4 + 32 + len(rec["name"]) + 1 + 4 * len(rec["cigar"]) + (l_seq + 1) // 2 + l_seq + len(bam.filter_aux(rec["tags"]))


def situations(records, finals, packs):
    """{situation: how many reads hit it} of reads, their final CIGARs and their code arrays [(reference codes, read codes)].
    head_offset_mod8_j: the reads, refused ones too, whose staged FULL head starts at j modulo 8 where the heads of the whole
    batch lie one after the other in this order, as the file pipeline and the debug entry stage them
    (csrc/file_pipeline.hpp plan_staged_heads): the unpack and emit kernels read a head from any alignment."""
    count = {s: 0 for s in SITUATIONS}

    def seen(name, yes=True):
        count[name] += bool(yes)
    head = 0                                                     # where the read's staged head starts (below)
    for rec, final, (rc, sc) in zip(records, finals, packs):
        seen(f"head_offset_mod8_{head % 8}")                     # (a refused read's head is staged and unpacked like any other)
        head += staged_full_head_bytes(rec)
        if rec["_status"] & 32:
            seen("refused")
            continue
        fin, cig = oc.runs_of(final), rec["cigar"]
        n = len(fin)
        ci, cj = oc.clip_range(cig)
        canon = canonical(cig[ci:cj])
        # ---- the final's tiles
        starts, a, b, nm = [], 0, 0, 0
        for op, ln in fin:
            starts.append((a, b))
            nm += int(_differs(rc, sc, a, b, ln).sum()) if op in COMPARED else ln if op in (I, D) else 0
            a += ln if op in (M, EQ, X, D, N) else 0
            b += ln if op in (M, EQ, X, I, S) else 0
        seams = range(64, n, 64)
        seen("compared_run_over_tile_seam", any(fin[s - 1][0] in COMPARED and fin[s][0] in COMPARED and fin[s - 1][1] and fin[s][1] for s in seams))
        behind = set()
        for s in seams:
            live = [c for c in range(s) if fin[c][1]]
            if fin[s][0] in (I, D, N) and fin[s][1] and live and fin[live[-1]][0] in COMPARED:
                c = live[-1]
                last = _differs(rc, sc, starts[c][0] + fin[c][1] - 1, starts[c][1] + fin[c][1] - 1, 1)[0]
                behind.add(f"tile_first_{OPS[fin[s][0]]}_behind_open_{'X' if last else 'EQ'}")
        for name in behind:
            seen(name)
        seen("zero_word_final_lane0", any(fin[c][1] == 0 for c in range(0, n, 64)))
        seen("zero_word_final_lane63", any(fin[c][1] == 0 for c in range(63, n, 64)))
        md10, md100 = _count_seams(fin, rc, sc, (D,))
        cs10, cs100 = _count_seams(fin, rc, sc, (I, D, N))
        seen("md_count_10_over_round_seam", md10), seen("md_count_100_over_round_seam", md100)
        seen("cs_count_10_over_round_seam", cs10), seen("cs_count_100_over_round_seam", cs100)
        seen("nm_one_byte", nm <= 0xFF), seen("nm_two_bytes", 0xFF < nm <= 0xFFFF)
        seen("final_past_reference", a > len(rc)), seen("final_past_read", b > len(sc))
        seen("final_short_of_reference", a < len(rc)), seen("final_short_of_read", b < len(sc))
        seen("empty_final", n == 0)
        # ---- the input's tiles: word c of the record, the clip words counted, lies in lane c % 64
        seen("zero_word_input_lane0", any(cig[c][1] == 0 for c in range(ci, cj) if c % 64 == 0))
        seen("zero_word_input_lane63", any(cig[c][1] == 0 for c in range(ci, cj) if c % 64 == 63))
        seen("zero_tile_of_input", any(all(cig[c][1] == 0 for c in range(max(ci, t), min(cj, t + 64))) for t in range(0, cj, 64) if max(ci, t) < min(cj, t + 64)))
        cop = lambda c: M if cig[c][0] in (EQ, X) else cig[c][0]
        merges = False
        for s in range(64, cj, 64):
            lo, hi = [c for c in range(ci, min(s, cj)) if cig[c][1]], [c for c in range(max(s, ci), cj) if cig[c][1]]
            merges = merges or bool(lo and hi and cop(lo[-1]) == cop(hi[0]))
        seen("input_run_merges_over_tile_seam", merges)
        # ---- the final against the input's canonical form
        same = [x == y for x, y in zip(canon, fin)]
        prefix = same.index(False) if False in same else len(same)
        back = [x == y for x, y in zip(canon[::-1], fin[::-1])]
        suffix = back.index(False) if False in back else len(back)
        longest = max(len(canon), n)
        seen("unchanged", canon == fin), seen("changed", canon != fin)
        seen("near_miss_last_word", canon != fin and prefix >= longest - 1)
        seen("near_miss_first_word", canon != fin and suffix >= longest - 1)
        seen("near_miss_first_word_of_a_tile", canon != fin and prefix >= 64 and prefix % 64 == 0 and prefix + suffix >= longest - 1)
        seen("final_fewer_words", n < len(canon)), seen("final_more_words", n > len(canon))
        seen("passes_under_0x904", rec["flag"] & 0x904), seen("own_oc_tag", b"OCZ" in rec["tags"]), seen("no_qualities", rec["qual"] is None)
        if (cig[:ci], cig[cj:]) in fc.CLIPS:
            seen(f"clip_shape_{fc.CLIPS.index((cig[:ci], cig[cj:]))}")
    return count


# ---- the statement, with a read's tag texts computed once -----------------------------------------------------------------------------
def read_texts(raw, rc, sc, final):
    """everything bam.full_record computes from the bases of one read, under any option set: the input record taken apart as
    full_record takes it apart, and the statement's NM, MD, cs in both forms, de, =/X form, changed flag and OC text"""
    raw = bytes(raw)
    ref_id, pos, l_rn, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", raw, 4)
    q = 36 + l_rn
    cigar = [(c & 15, c >> 4) for c in struct.unpack_from(f"<{n_cig}I", raw, q)]
    q += 4 * n_cig
    body = raw[q:q + (l_seq + 1) // 2 + l_seq]
    aux = raw[q + len(body):4 + struct.unpack_from("<i", raw, 0)[0]]
    cigar = bam.resolve_long_cigar(cigar, l_seq, ref_id, pos, aux)
    i, j = oc.clip_range(cigar)
    return dict(fixed=(ref_id, pos, l_rn, mapq, flag, l_seq, nref, npos, tlen), name=raw[36:36 + l_rn], lead=cigar[:i], trail=cigar[j:], body=body, aux=aux,
                reflen=sum(n for op, n in cigar if op in (0, 2, 3, 7, 8)), final=final, nm=bam.nm_of(rc, sc, final), md=bam.md_of(rc, sc, final),
                cs={"short": bam.cs_of(rc, sc, final), "long": bam.cs_of(rc, sc, final, long=True)}, de=bam.de_of(rc, sc, final),
                eqx=bam.eqx_of(rc, sc, final), changed=bam.cigar_changed(cigar[i:j], final), oc=bam.oc_of(cigar))


def assemble(t, md=False, cs=None, de=False, eqx=False, oc=False):
    """the FULL record of read_texts' dict under one option set: bam.full_record's assembly (tests/test_bam_fuzz.py holds it to
    bam.full_record itself on one seed, over all option sets)"""
    ref_id, pos, l_rn, mapq, flag, l_seq, nref, npos, tlen = t["fixed"]
    fin = oc_runs(t["eqx"] if eqx else t["final"])
    words = b"".join(struct.pack("<I", (n << 4) | op) for op, n in t["lead"] + fin + t["trail"])
    nm = t["nm"]
    tags = bam.filter_aux(t["aux"], oc) + fc.nm_tag(nm)
    if md:
        tags += b"MDZ" + t["md"].encode() + b"\0"
    if cs:
        tags += b"csZ" + t["cs"][cs].encode() + b"\0"
    if de:
        tags += b"def" + struct.pack("<f", t["de"])
    if oc and t["changed"]:
        tags += b"OCZ" + t["oc"].encode() + b"\0"
    if len(words) // 4 > 0xFFFF:
        tags += b"CGBI" + struct.pack("<I", len(words) // 4) + words
        words = struct.pack("<II", (l_seq << 4) | 4, (t["reflen"] << 4) | 3)
    out = (struct.pack("<iiBBHHHiiii", ref_id, pos, l_rn, mapq, bam.reg2bin(pos, pos + max(1, t["reflen"])), len(words) // 4, flag, l_seq, nref, npos, tlen) +
           t["name"] + words + t["body"] + tags)
    return struct.pack("<i", len(out)) + out


oc_runs = oc.runs_of


def assembled_stream(texts, raws, records, status, mask=0, **kw):
    """assemble() of every kept read, a record that passes under `mask` as it came, one after the other"""
    return b"".join(raw if rec["flag"] & mask else assemble(t, **kw) for t, raw, rec, st in zip(texts, raws, records, status) if not st & 32)


def statement_stream(raws, records, packs, finals, status, mask=0, **kw):
    """the same through bam.full_record itself"""
    return b"".join(raw if rec["flag"] & mask else bam.full_record(raw, rc, sc, fin, **kw)
                    for raw, rec, (rc, sc), fin, st in zip(raws, records, packs, finals, status) if not st & 32)


def describe_difference(got, want, records, finals, status, mask=0):
    """the first record that differs: the read's name, its input CIGAR and its final, each cut to 120 characters"""
    from test_bam_out import split_records
    kept = [(r, f) for r, f, st in zip(records, finals, status) if not st & 32]
    a, b = split_records(got), split_records(want)
    for k, ((_, x), (_, y)) in enumerate(zip(a, b)):
        if x != y:
            rec, fin = kept[k]
            at = next((q for q in range(min(len(x), len(y))) if x[q] != y[q]), min(len(x), len(y)))
            return dict(read=rec["name"], input=oc.text_of(rec["cigar"])[:120], final=fin[:120], sizes=(len(x), len(y)), first_byte=at)
    return dict(records=(len(a), len(b)), bytes=(len(got), len(want)))


# ---- reads of the worst density, written by hand, for the record buffer's bound (csrc/hostio.hpp) ------------------------------------------
_DENSE = {}


def dense_reads(seed=59, n=300):
    """(references, refs, records, finals): the reads that make a tag longest for the reference positions and bases they cover --
    `md`: (1M 1D) x n with every M position differing, MD `0A0^C` per pair; `alt`: ONE M word of 2 n positions that differ and do
    not in turn, cs `*ag:1` / `*ag=C` per pair and two =/X words per pair; `all_x`: one M word whose every position differs, cs
    `*ag` per position; `mi`: (1M 1I) x n; `oc`: an input of 2 n words between two hard clips of 2^28 - 1 whose final is the same
    alignment in two words, so the read changed and carries all of them in OC.  Finals are M / I / D and cover the read exactly,
    as the file pipeline's do."""
    if seed in _DENSE:
        return _DENSE[seed]
    rng = np.random.default_rng(seed)
    contig = lc.random_contig(rng, 12 * n + 1000)
    records, finals = [], []

    def add(name, cigar, final, differ):
        """differ(q): whether compared position q of the read differs"""
        pos = 100 + 2 * n * len(records) + 50 * len(records)
        seq, at, q = [], pos, 0
        for op, ln in cigar:
            if op == M:
                for c in contig[at:at + ln]:
                    seq.append(mc.other(c) if differ(q) else c)
                    q += 1
            elif op == I:
                seq += list(lc.random_contig(rng, ln))
            if op in (M, D):
                at += ln
        records.append(dict(name=name, flag=0, ref_id=0, pos=pos, mapq=60, seq="".join(seq), cigar=list(cigar), qual=bytes(len(seq)), tags=b"",
                            _status=0, _ctg="ctg"))
        finals.append(final)
    add("md", [(M, 1), (D, 1)] * n, "1M1D" * n, lambda q: True)
    add("alt", [(M, 2 * n)], f"{2 * n}M", lambda q: q % 2 == 0)
    add("all_x", [(M, 2 * n)], f"{2 * n}M", lambda q: True)
    add("mi", [(M, 1), (I, 1)] * n, "1M1I" * n, lambda q: False)
    big = (1 << 28) - 1
    add("oc", [(H, big)] + [(M, 1), (I, 1)] * n + [(H, big)], f"{n}M{n}I", lambda q: q % 2 == 0)
    out = ([("ctg", len(contig))], {"ctg": contig}, records, finals)
    _DENSE[seed] = out
    return out


# ---- one crafted read: long only through the split, and changed ------------------------------------------------------------------------
_SPLIT = {}


def split_long_read(seed=53):
    """(references, refs, records, finals): one read whose M form is 1S <65534>M 2S with every second base differing, as
    bam_eqx_cases.cg_reads' -- but its input CIGAR has the M word in two with a `0I` between, and its final is 65533M1I: the read
    CHANGED.  In M form the record has 4 words; in =/X form 65 533 + 1 + 2 = 65 536, so its CIGAR goes to the CG tag, behind OC."""
    if seed in _SPLIT:
        return _SPLIT[seed]
    rng = np.random.default_rng(seed)
    ln = 65534
    contig = lc.random_contig(rng, ln + 300)
    seq = list(contig[100:100 + ln])
    for e in range(1, ln, 2):
        seq[e] = mc.other(seq[e])
    rec = dict(name="split_long", flag=0, ref_id=0, pos=100, mapq=40, seq="G" + "".join(seq) + "TT", cigar=[(S, 1), (M, 30000), (I, 0), (M, ln - 30000), (S, 2)],
               qual=None, tags=b"RGZgrp\0", _status=0, _ctg="ctg")
    out = ([("ctg", len(contig))], {"ctg": contig}, [rec], [f"{ln - 1}M1I"])
    _SPLIT[seed] = out
    return out
