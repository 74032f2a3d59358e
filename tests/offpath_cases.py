"""Inputs of tests/test_gpu_offpath.py: short reads on which the OUT-OF-LINE blocks of the fill step's text show (the LEN
loop and the two-candidate block of the SHR pass, npore_amd/csrc/gen_fill_asm.py), and what the host twin of the prep
kernels (tests/model) says about them.

Every read (at most 600 bases, cut into three or four chunks) is a chain of elements, 3 ... 11 random bases between them:
  * a repeat of a unit of 1, 2 or 3 bases, 4 ... 31 copies in the reference, with 1, 2 or 3 copies more in the read: an
    insertion at the END of the repeat (LEN candidates all along it, at the period of the unit).  The copy numbers come
    in turn from a list that holds 29, 30 and 31: a candidate there calls a length of 32 and more (L + copies inserted
    + 1), whose score is not in the LDS table (`big`: read from global memory);
  * homopolymers of different bases close to each other, and a homopolymer behind a dinucleotide repeat that ends in
    its base: cells whose reference column starts an n-polymer and whose read row lies in one, of ANOTHER unit -- the
    position is flagged, the n-mer filter fails;
  * four copies of a motif bbbbc with a copy more in the read (step_cache_cases.py): the columns of a copy carry TWO SHR
    candidates, periods 5 and 1, the second one starting a run (the copy's first column) or continuing one; the column
    where a copy starts is flagged for LEN at both periods in one lane;
  * now and then a homopolymer of 33 ... 36 bases (its columns are rare: compiled steps) right behind an insertion, so
    that the text is entered again inside the elements that follow.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from ref_queue_cases import chunks_of, plain_range
from step_cache_cases import DSC_HAS2, DSC_RARE, FLAG_SHIFT, MER_SHIFT, n_waves, role_of

_MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "model")
_TWIN = None


def build_twin(force=False):
    """tests/model/libshr2_twin.so: the host twin of the fill with the notes of the two-candidate block switched on"""
    so = os.path.join(_MODEL, "libshr2_twin.so")
    csrc = os.path.join(_MODEL, "..", "..", "npore_amd", "csrc")
    deps = [os.path.join(_MODEL, f) for f in ("shr2_twin.cpp", "pull_model.cpp", "host_prep.hpp")] + \
           [os.path.join(csrc, f) for f in ("cell.hpp", "layout.hpp")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, deps[0]])
    return so


def shr2_notes(ref, seq, cigar, sub, nps, indel_start, indel_extend, max_b_rows, r, max_n=6, max_l=100):
    """int32 [n, 6] of one read: see tests/model/shr2_twin.cpp"""
    global _TWIN
    if _TWIN is None:
        _TWIN = C.CDLL(build_twin())
        _TWIN.shr2_twin_notes.restype = C.c_int64
        _TWIN.shr2_twin_notes.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    ref, seq = np.ascontiguousarray(ref, np.uint8), np.ascontiguousarray(seq, np.uint8)
    sub, nps = np.ascontiguousarray(sub, np.float32), np.ascontiguousarray(nps, np.float32)
    cig = cigar.encode()
    cap = (len(ref) + len(seq) + 2) * (2 * r + 1)          # one note per cell at the most
    out = np.zeros(6 * cap, np.int32)
    n = _TWIN.shr2_twin_notes(ref.ctypes.data, len(ref), seq.ctypes.data, len(seq), cig, len(cig), sub.ctypes.data, nps.ctypes.data,
                              max_n, max_l, indel_start, indel_extend, max_b_rows, r, out.ctypes.data, cap)
    assert 0 <= n <= cap, n
    return out[:6 * n].reshape(-1, 6)


COPIES = (4, 29, 7, 30, 5, 31, 12, 6, 21, 9, 31, 4, 16, 30, 8, 29)
KEYS = ("text", "len_fail", "len_pass", "len_two_periods", "len_two_iter", "len_big", "len_lane0", "len_lane63",
        "two", "two_start", "two_cont")


def make_reads(seed, n_reads, t0, n_chunks):
    """-> refs, seqs, cigars, max_b_rows; every read has t0 or t0 + 1 anti-diagonals"""
    rng = np.random.default_rng(seed)
    mbr = (t0 - 40) // (n_chunks - 1) + 1
    refs, seqs, cigs = [], [], []
    e = 0
    for k in range(n_reads):
        ref, seq, cig = [], [], []

        def same(n):
            b = [int(x) for x in rng.integers(1, 5, max(n, 0))]
            ref.extend(b); seq.extend(b); cig.extend("=" * len(b))

        def unit(u):
            while True:
                b = [int(x) for x in rng.integers(1, 5, u)]
                if u == 1 or len(set(b)) > 1:
                    return b

        def repeat(u, copies, more):
            ref.extend(u * copies); seq.extend(u * (copies + more))
            cig.extend("=" * (len(u) * copies) + "I" * (len(u) * more))

        def element(e):
            kind = e % 6
            copies, more = COPIES[(e // 6 + e) % len(COPIES)], 1 + (e // 3) % 3
            if kind in (0, 3):                       # homopolymer, another one of a different base right behind it
                b = unit(1)
                repeat(b, copies, more)
                same(1 + e % 3)
                repeat([1 + b[0] % 4], 4 + e % 5, 1)
            elif kind == 1:                          # dinucleotide repeat, then a homopolymer of its last base
                u = unit(2)
                repeat(u, min(copies, 16), more)
                repeat([u[1]], 5, 1)
            elif kind == 2:                          # trinucleotide repeat
                repeat(unit(3), min(copies, 10), more)
            elif kind == 4:                          # the two-candidate motif, a copy more in the read
                b = int(rng.integers(1, 5))
                repeat([b, b, b, b, 1 + b % 4], 4, 1 + (e // 6) % 2)
            else:                                    # a rare run right behind an insertion (every other time: a long repeat)
                if (e // 6) % 2:
                    b = unit(1)
                    seq.extend(b * 3); cig.extend("III")
                    n = int(rng.integers(33, 37))
                    ref.extend(b * n); seq.extend(b * n); cig.extend("=" * n)
                else:
                    repeat(unit(1), 31, 1 + (e // 12) % 3)
            same(int(rng.integers(3, 12)))

        same(int(rng.integers(5, 30)))
        while len(ref) + len(seq) + 1 < t0 - 90:
            element(e)
            e += 1
        while len(ref) + len(seq) + 1 < t0:
            same(1)
        refs.append(np.array(ref, np.uint8)); seqs.append(np.array(seq, np.uint8)); cigs.append("".join(cig))
    return refs, seqs, cigs, mbr


def survey(prep, r):
    """Per wave role, over the plain ranges of one read's chunks, the steps that run in the text (step_cache_cases.survey
    says how they are told from the compiled ones) in which a band-interior lane
      len_fail         holds a flagged LEN period (cell.hpp: flagged in the column's reference word and in the row's read
                       word) whose n-mer does NOT match
      len_pass         holds one whose n-mer matches: the candidate is evaluated
      len_two_periods  holds two flagged periods at once
      len_two_iter     holds two flagged periods of which the LOWER one matches: the loop's second iteration evaluates
      len_big          holds a matching one whose reference repeat count L is 31 or more: the call length L + q + 1 is
                       at least 32, the score comes from global memory (L itself is capped at 32 columns later: a
                       column of L >= 32 is rare)
      len_lane0 / 63   holds a flagged period in lane 0 / lane 63 of the wave
      two              holds a column with two SHR candidates; two_start / two_cont: whose second candidate starts a
                       run / continues one
    Step b of a chunk computes, in lane l of wave w, the cell of row ins + r - (64 w + l) and column del + 64 w + l - r,
    (ins, del) = the path's position behind the step."""
    nw = n_waves(r)
    out = {role_of(w, nw): dict.fromkeys(KEYS + ("interior",), 0) for w in range(nw)}
    n_plain = 0
    seq_off = np.concatenate([[0], np.cumsum(prep["geom"][:, 4] + 1)])
    ref_off = 0
    for ch, (steps, refw, g) in enumerate(chunks_of(prep)):
        seqw = prep["seqw"][seq_off[ch]:seq_off[ch + 1]].astype(np.uint32)
        ncol = g["dcols"] + 1
        refl = prep["refl"][ref_off:ref_off + ncol]
        ref_off += ncol
        lo, hi, dl = plain_range(steps, g, r)
        lo = max(lo, 1)
        if lo >= hi:
            continue
        n_plain += 1
        pad = 64 * nw + 2
        rare = np.zeros(ncol + pad, bool); rare[:ncol] = (refw[:ncol, 2] & DSC_RARE) != 0
        b = np.arange(lo, hi)
        is_i = steps[b - 1] != 0
        before = dl[b - 1]
        for w in range(nw):
            role = out[role_of(w, nw)]
            tcol = 64 * w + np.arange(64)
            interior = (tcol >= 1) & (tcol <= 2 * r - 1)
            counted = interior if (w == 0 and nw > 1) else np.ones(64, bool)
            role["interior"] |= int(interior.any())
            if not interior.any():
                continue
            jb = before[:, None] + tcol[None, :] - r
            compiled = (rare[jb] & counted[None, :]).any(axis=1) | (~is_i & rare[before + 64 * w + 64 - r])
            text = ~compiled
            role["text"] += int(text.sum())
            row = np.clip((b - dl[b])[:, None] + r - tcol[None, :], 0, g["drows"])
            col = np.clip(dl[b][:, None] + tcol[None, :] - r, 0, ncol - 1)
            live = text[:, None] & interior[None, :]
            sw = seqw[row]
            rx = refw[:ncol, 0].astype(np.uint32)[col]
            flags = ((sw & rx) >> FLAG_SHIFT) & 63
            flags = np.where(live, flags, 0)
            match = np.zeros(flags.shape, np.uint32)
            big = np.zeros(flags.shape, bool)
            for n in range(1, 7):
                mer = np.uint32((1 << 3 * n) - 1)
                m = ((flags >> (n - 1)) & 1 != 0) & ((((sw >> np.uint32(32 - 3 * n)) ^ (rx >> MER_SHIFT)) & mer) == 0)
                match |= m.astype(np.uint32) << (n - 1)
                big |= m & (refl[col, n - 1] >= 31)
            pop = sum((flags >> n) & 1 for n in range(6))
            top = np.zeros(flags.shape, np.uint32)
            for n in range(6):
                top = np.where((flags >> n) & 1 != 0, np.uint32(1 << n), top)
            role["len_fail"] += int(((flags & ~match) != 0).any(axis=1).sum())
            role["len_pass"] += int((match != 0).any(axis=1).sum())
            role["len_two_periods"] += int((pop >= 2).any(axis=1).sum())
            role["len_two_iter"] += int(((match & ~top) != 0).any(axis=1).sum())
            role["len_big"] += int(big.any(axis=1).sum())
            role["len_lane0"] += int((flags[:, 0] != 0).sum())
            role["len_lane63"] += int((flags[:, 63] != 0).sum())
            z, wd = refw[:ncol, 2].astype(np.uint32)[col], refw[:ncol, 3].astype(np.uint32)[col]
            has2 = live & ((z & DSC_HAS2) != 0)
            role["two"] += int(has2.any(axis=1).sum())
            role["two_start"] += int((has2 & ((wd >> 31) != 0)).any(axis=1).sum())
            role["two_cont"] += int((has2 & ((wd >> 31) == 0)).any(axis=1).sum())
    return dict(roles=out, n_plain=n_plain, n_chunks=len(prep["geom"]))


def shr2_outcomes(notes, prep, r):
    """Per wave role, from the notes of tests/model/shr2_twin.cpp (one per cell whose column carries a second SHR
    candidate: chunk-local anti-diagonal, band column, local reference column, first taken, second taken, values equal)
    and the same read's annotation: the steps that run in the text (as in `survey`) in which a band-interior lane holds a
    column whose second candidate
      two_win   is taken (its value is strictly below the first's, or the first was not taken, and below 100 b)
      two_tie   has exactly the value of the first, which was taken: the first must stay
    The notes come chunk after chunk, row after row; a chunk's notes are told from the next one's by the anti-diagonal
    falling back, and checked against the chunk's own columns (the note's reference column is del - r + band column)."""
    nw = n_waves(r)
    out = {role_of(w, nw): dict(two_win=0, two_tie=0, two_cells=0) for w in range(nw)}
    chunks = chunks_of(prep)
    bounds = [0] + [k for k in range(1, len(notes)) if notes[k, 0] < notes[k - 1, 0]] + [len(notes)]
    groups = [notes[a:b] for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
    ch = 0
    for g_notes in groups:
        while True:                                    # (a chunk without a two-candidate cell has no group)
            assert ch < len(chunks), "notes that fit no chunk"
            steps, refw, g = chunks[ch]
            lo, hi, dl = plain_range(steps, g, r)
            ch += 1
            ok = g_notes[:, 0].max() < g["nrows"]
            ok = ok and bool((g_notes[:, 2] == dl[g_notes[:, 0]] - r + g_notes[:, 1]).all())
            ok = ok and bool((g_notes[:, 2] >= 0).all()) and int(g_notes[:, 2].max()) <= g["dcols"]
            ok = ok and bool(((refw[g_notes[:, 2], 2] & DSC_HAS2) != 0).all())
            if ok:
                break
        lo = max(lo, 1)
        if lo >= hi:
            continue
        ncol = g["dcols"] + 1
        rare = np.zeros(ncol + 64 * nw + 2, bool); rare[:ncol] = (refw[:ncol, 2] & DSC_RARE) != 0
        b = np.arange(lo, hi)
        is_i = steps[b - 1] != 0
        before = dl[b - 1]
        for w in range(nw):
            tcol = 64 * w + np.arange(64)
            interior = (tcol >= 1) & (tcol <= 2 * r - 1)
            counted = interior if (w == 0 and nw > 1) else np.ones(64, bool)
            jb = before[:, None] + tcol[None, :] - r
            compiled = (rare[jb] & counted[None, :]).any(axis=1) | (~is_i & rare[before + 64 * w + 64 - r])
            text = np.zeros(g["nrows"], bool); text[lo:hi] = ~compiled
            c = g_notes[:, 1]
            m = (c // 64 == w) & (c >= 1) & (c <= 2 * r - 1) & text[g_notes[:, 0]]
            role = out[role_of(w, nw)]
            role["two_cells"] += int(m.sum())
            role["two_win"] += len({int(x) for x in g_notes[m & (g_notes[:, 4] != 0), 0]})
            role["two_tie"] += len({int(x) for x in g_notes[m & (g_notes[:, 3] != 0) & (g_notes[:, 4] == 0) & (g_notes[:, 5] != 0), 0]})
    return out
