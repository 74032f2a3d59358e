"""Inputs of tests/test_gpu_step_cache.py: reads on which a stale or clobbered column cache of the fill step shows, and
what the host twin of the prep kernels (tests/model) says about them.

The hand-scheduled step loop (npore_amd/csrc/gen_fill_asm.py) derives the fields of a column descriptor in a 'D' step and
where the text is entered, and an 'I' step reads them from registers: the cache has to survive every run of 'I' steps and
everything that happens inside one (the end of a 64-step window, a block end, the refills of the word queues, the
out-of-line polls, the LEN variant of the hand-over), and it has to be rebuilt at every entry.

Every read:
  * n-polymers every 67 reference columns (67 is prime to 64: they pass every lane), by turns a homopolymer of 6 ... 9
    (ONE candidate period) and four copies of a motif bbbbc (a column per copy carries TWO: periods 5 and 1), with
    copy-number changes in the read;
  * events, one every ~100 anti-diagonals, by turns
      - an insertion in the middle of a two-candidate motif, of copies of the motif (LEN candidates all along it),
      - an insertion at the end of a homopolymer, of the same base,
      - a deletion of 65 ... 80 reference bases (it drains a reference-word queue: a refill) with an insertion right
        behind it,
      - a run of 33 ... 40 equal bases (L >= 32: a rare column, every wave that holds it runs compiled steps) and an
        insertion at the reference position where the run's last column leaves the lanes of one wave: that wave enters
        the text again with an 'I' step first.  The distance is drawn from those of the first, the second and the
        last wave of the band;
    with insertion lengths taken in turn from 1, 2, 63, 64, 65, 130: runs of 'I' steps that cross the end of a step
    window, a block end and a refill of the read words;
  * a length padded so that `max_b_rows` cuts it into `n_full` chunks with a plain range and a short tail.
"""
import numpy as np

from ref_queue_cases import chunks_of, plain_range

DSC_HAS2, DSC_RARE = 1 << 5, 1 << 7      # layout.hpp
MER_SHIFT, FLAG_SHIFT = 14, 8            # layout.hpp: the six bases and the six "n-polymer" flags of a read / reference word
INS_LENGTHS = (1, 2, 63, 64, 65, 130)


def n_waves(r):
    return (2 * r + 1 + 63) // 64


def role_of(w, nw):
    """gen_fill_asm.py: 0 = only wave of a chunk, 1 = first, 2 = middle, 3 = last of several"""
    return 0 if nw == 1 else 1 if w == 0 else 3 if w == nw - 1 else 2


def make_reads(seed, n_reads, t0, n_full, r):
    """-> refs, seqs, cigars, max_b_rows; every read has t0 or t0 + 1 anti-diagonals"""
    rng = np.random.default_rng(seed)
    mbr = (t0 - 40) // n_full + 1
    nw = n_waves(r)
    # reference distance from the last column of a rare run to the insertion that follows the step in which that column
    # leaves wave w: lane l of wave w holds reference index del + 64 w + l - r; the first wave of several counts its
    # band-interior lanes only (lane 0 is the band's edge)
    leave = sorted({r + 1 - 64 * w + (-1 if w == 0 and nw > 1 else 0) for w in {0, min(1, nw - 1), nw - 1}})
    refs, seqs, cigs = [], [], []
    ev = 0
    for k in range(n_reads):
        ref, seq, cig = [], [], []

        def same(n):
            b = [int(x) for x in rng.integers(1, 5, max(n, 0))]
            ref.extend(b); seq.extend(b); cig.extend("=" * len(b))

        def insert(bases):
            seq.extend(bases); cig.extend("I" * len(bases))

        def motif():
            b = int(rng.integers(1, 5))
            return [b, b, b, b, 1 + b % 4]

        def polymer(m):
            """one n-polymer, 67 columns with its filler; a copy more or fewer in the read now and then"""
            if m % 2:
                u, copies = motif(), 4
            else:
                u, copies = [int(rng.integers(1, 5))], int(rng.integers(6, 10))
            delta = int(rng.integers(-1, 2))
            ref.extend(u * copies); seq.extend(u * (copies + delta))
            cig.extend("=" * (len(u) * min(copies, copies + delta)) + ("I" if delta > 0 else "D") * (len(u) * abs(delta)))
            same(67 - len(u) * copies)

        def event(e):
            n = INS_LENGTHS[e % len(INS_LENGTHS)]
            kind = (e // len(INS_LENGTHS) + e) % 4
            if kind == 0:          # inside a two-candidate motif, copies of it
                u = motif()
                ref.extend(u * 4); seq.extend(u * 2); cig.extend("=" * 10)
                insert((u * (n // 5 + 1))[:n])
                seq.extend(u * 2); cig.extend("=" * 10)
            elif kind == 1:        # at the end of a homopolymer, the same base
                b = int(rng.integers(1, 5))
                ref.extend([b] * 7); seq.extend([b] * 7); cig.extend("=" * 7)
                insert([b] * n)
                same(1)
            elif kind == 2:        # a long deletion, the insertion right behind it
                gap = [int(x) for x in rng.integers(1, 5, int(rng.integers(65, 81)))]
                ref.extend(gap); cig.extend("D" * len(gap))
                insert([int(x) for x in rng.integers(1, 5, n)])
            else:                  # a rare run, the insertion where its last column leaves one wave
                dist = leave[(e // 4) % len(leave)]
                L, b = int(rng.integers(33, 41)), int(rng.integers(1, 5))
                if dist >= 1:
                    ref.extend([b] * L); seq.extend([b] * L); cig.extend("=" * L)
                    same(dist - 1)
                    insert([int(x) for x in rng.integers(1, 5, n)])
                else:              # the insertion lies -dist + 1 columns in front of the run's last column
                    insert([int(x) for x in rng.integers(1, 5, n)])
                    same(1 - dist - L)      # (nothing where the run is longer than that: the insertion then stands at its head)
                    ref.extend([b] * L); seq.extend([b] * L); cig.extend("=" * L)
            same(int(rng.integers(3, 12)))

        same(int(rng.integers(7, 74)))
        m = k
        while len(ref) + len(seq) + 1 < t0 - 330:
            polymer(m)
            m += 1
            if m % 2 == 0:
                event(ev)
                ev += 1
        while len(ref) + len(seq) + 1 < t0 - 150:
            polymer(m)
            m += 1
        while len(ref) + len(seq) + 1 < t0:
            same(1)
        refs.append(np.array(ref, np.uint8)); seqs.append(np.array(seq, np.uint8)); cigs.append("".join(cig))
    return refs, seqs, cigs, mbr


def survey(prep, r):
    """Per wave role, over the plain ranges of one read's chunks, what the step text meets -- from the annotation alone.
    Step b of a chunk (kind steps[b - 1]) finds reference index dl[b - 1] + 64 w + l - r in lane l of wave w.  A wave runs
    the step through the compiled body when a lane it counts holds a rare descriptor (kernels.hpp plain_span `rare_here`;
    the first wave of several counts its band-interior lanes) or, a 'D' step, when the descriptor that enters at its
    last lane is rare (the text's own test); the text is ENTERED at the first step of the plain range and behind every
    compiled step.  Counted per role:
      entry_i   entries whose first step is an 'I' step (the cache is built and used before any 'D' step has run)
      window_i  pairs of 'I' steps in the text on either side of the end of a 64-step window
      two_i     'I' steps in the text, behind an 'I' step in the text, with a two-candidate column in a band-interior lane
      len_i     'I' steps in the text, behind an 'I' step in the text, in which a band-interior lane holds a LEN candidate
                that passes the n-mer filter (cell.hpp: a period n flagged in the column's reference word -- position j
                starts an n-polymer -- and in the row's read word -- position i - n lies in one -- with the n most
                recent read bases equal to the next n reference bases; lane l of wave w holds row ins + r - (64 w + l)
                and column del + 64 w + l - r): the LEN variant of the hand-over runs between the cache's write and
                this step's use of it
      refill_i  (waves that hold band column 0) pairs of 'I' steps in the text with a refill of the read-word queue between
                them: the queue holds 64 words from the chunk's first step on and every 'I' step takes one
                (kernels.hpp sq_idx), so the refill stands in front of the chunk's 'I' step number 64 k + 1
      interior  whether the role holds a band-interior column at all (the last wave of r = 32, 64, 256 holds the edge only)
    Every window end is a block end (gen_fill_asm.py block_end: bend <= (bl | 63) + 1) and so is every refill, so
    window_i and refill_i count block ends inside runs of 'I' steps."""
    nw = n_waves(r)
    out = {role_of(w, nw): dict(entry_i=0, window_i=0, two_i=0, len_i=0, refill_i=0, interior=False, text=0) for w in range(nw)}
    n_plain, longest_i = 0, 0
    seq_off = np.concatenate([[0], np.cumsum(prep["geom"][:, 4] + 1)])
    assert seq_off[-1] == len(prep["seqw"])
    for ch, (steps, refw, g) in enumerate(chunks_of(prep)):
        seqw = prep["seqw"][seq_off[ch]:seq_off[ch + 1]].astype(np.uint32)
        lo, hi, dl = plain_range(steps, g, r)
        lo = max(lo, 1)
        if lo >= hi:
            continue
        n_plain += 1
        ncol = g["dcols"] + 1
        pad = 64 * nw + 2
        rare = np.zeros(ncol + pad, bool); rare[:ncol] = (refw[:ncol, 2] & DSC_RARE) != 0
        two = np.zeros(ncol + pad, bool); two[:ncol] = (refw[:ncol, 2] & DSC_HAS2) != 0
        b = np.arange(lo, hi)
        is_i = steps[b - 1] != 0
        before = dl[b - 1]
        run = 0
        for x in is_i.tolist():
            run = run + 1 if x else 0
            longest_i = max(longest_i, run)
        for w in range(nw):
            role = out[role_of(w, nw)]
            lanes = np.arange(64)
            tcol = 64 * w + lanes
            interior = (tcol >= 1) & (tcol <= 2 * r - 1)
            counted = interior if (w == 0 and nw > 1) else np.ones(64, bool)
            role["interior"] |= bool(interior.any())
            j = before[:, None] + tcol[None, :] - r
            assert j.min() >= 0
            compiled = (rare[j] & counted[None, :]).any(axis=1) | (~is_i & rare[before + 64 * w + 64 - r])
            text = ~compiled
            entered = text & np.concatenate([[True], compiled[:-1]])
            role["text"] += int(text.sum())
            role["entry_i"] += int((entered & is_i).sum())
            pair = text[:-1] & text[1:] & is_i[:-1] & is_i[1:]
            role["window_i"] += int((pair & (b[1:] % 64 == 0)).sum())
            has2 = (two[j] & interior[None, :]).any(axis=1)
            role["two_i"] += int((pair & has2[1:]).sum())
            # an 'I' step leaves the columns where they are: dl[b] = dl[b - 1] in every step counted here
            # (lanes beyond the band hold nothing that counts: their indices are clipped, their lanes masked below)
            row = (b - dl[b])[:, None] + r - tcol[None, :]
            col = dl[b][:, None] + tcol[None, :] - r
            if interior.any():
                assert row[:, interior].min() >= 0 and row[:, interior].max() <= g["drows"] and col[:, interior].max() < ncol
            sw = seqw[np.clip(row, 0, g["drows"])]
            rx = refw[:ncol, 0].astype(np.uint32)[np.clip(col, 0, ncol - 1)]
            flags = (sw & rx) >> FLAG_SHIFT
            good = np.zeros(row.shape, bool)
            for n in range(1, 7):
                mer = np.uint32((1 << 3 * n) - 1)
                good |= ((flags >> (n - 1)) & 1 != 0) & ((((sw >> np.uint32(32 - 3 * n)) ^ (rx >> MER_SHIFT)) & mer) == 0)
            role["len_i"] += int((pair & (good & interior[None, :]).any(axis=1)[1:]).sum())
            if w == 0:
                taken = b - dl[b]                    # 'I' steps of the chunk up to and including step b
                role["refill_i"] += int((pair & (taken[:-1] % 64 == 0) & (taken[:-1] > 0)).sum())
    return dict(roles=out, n_plain=n_plain, n_chunks=len(prep["geom"]), longest_i=longest_i)
