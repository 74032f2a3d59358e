"""Inputs of tests/test_gpu_ref_queue.py and tests/test_ref_queue_index.py: reads whose band crosses many refills of the
per-wave reference-word queues of fill_kernel (kernels.hpp ref_q: the 64 reference words that will enter at a wave's last
lane, one taken per 'D' step), and what the host twin of the prep kernels (tests/model) says about them.

Every read:
  * a reference of >= 10 x 64 columns, homopolymers of 6 ... 9 bases every 67 columns -- 67 is prime to 64, so they enter
    at every lane of the queue -- with copy-number changes in the read.  (Under the annotation's "longest" rule,
    annot_wave.hpp / host_prep.hpp np_info_compute, such a run is an n-polymer for period 1 alone: a third candidate
    period, DSC_MORE, takes a homopolymer of more than 200 bases.  What sends these reads down the rare path is:)
  * runs of 33 ... 55 bases (L >= 32: DSC_BIGL, hence DSC_RARE), one of >= 40 inside every plain range and more every
    five short ones, so that over a case rare descriptors lie at every lane of the queue and enter at many of them;
  * an input path that is deletion-heavy (even reads: deletions of 70 ... 90 bases drain a queue in consecutive steps,
    across a refill) or insertion-heavy (odd reads);
  * a length padded so that `max_b_rows` cuts it into `n_full` chunks that have a plain range (the hand-scheduled loop)
    and a tail of about 40 anti-diagonals that has none.
"""
import numpy as np

DSC_BIGL, DSC_MORE, DSC_RARE = 1 << 6, 1 << 7, 1 << 7      # layout.hpp: BIGL in either descriptor, MORE in the second, RARE in the first
REFW_SENTINEL = 0x36DB6 << 14                               # layout.hpp


def make_reads(seed, n_reads, t0, n_full, r, long_runs=True):
    """-> refs, seqs, cigars, max_b_rows.  Every read has t0 or t0 + 1 anti-diagonals; the long run and the long indel
    are placed where the chunks of that max_b_rows have their plain range at band half-width r.  long_runs=False leaves
    the runs of 33 ... 55 bases out: what remains are the homopolymers of 6 ... 9 (tests/test_ref_queue_index.py checks that
    those alone give no rare column)."""
    rng = np.random.default_rng(seed)
    mbr = (t0 - 40) // n_full + 1
    refs, seqs, cigs = [], [], []
    for k in range(n_reads):
        ref, seq, cig = [], [], []

        def same(n):
            b = [int(x) for x in rng.integers(1, 5, n)]
            ref.extend(b); seq.extend(b); cig.extend("=" * n)

        def long_run(lo):                         # a homopolymer of L >= 32, two copies fewer in the read
            n, base = int(rng.integers(lo, 56)), int(rng.integers(1, 5))
            ref.extend([base] * n); seq.extend([base] * (n - 2)); cig.extend("=" * (n - 2) + "DD")
            same(int(rng.integers(5, 30)))

        def long_indel():
            gap = [int(x) for x in rng.integers(1, 5, int(rng.integers(70, 91)))]
            if k % 2 == 0:
                ref.extend(gap); cig.extend("D" * len(gap))
            else:
                seq.extend(gap); cig.extend("I" * len(gap))

        events = []
        for c in range(n_full):                   # rows at which chunk c is well inside its plain range
            start = c * (mbr - 1) + 2 * r + 12 + 60
            events.append(start)
        same(int(rng.integers(7, 74)))
        m = 0
        while len(ref) + len(seq) + 1 < t0 - 150:
            base = int(rng.integers(1, 5))
            h = int(rng.integers(6, 10))
            delta = int(rng.integers(-2, 3))
            ref.extend([base] * h)
            seq.extend([base] * (h + delta))
            cig.extend("=" * min(h, h + delta) + ("I" * delta if delta > 0 else "D" * -delta))
            same(67 - h)
            m += 1
            if events and len(ref) + len(seq) + 1 >= events[0]:
                events.pop(0)
                if long_runs:
                    long_run(40)
                long_indel()
            elif long_runs and m % 5 == 4:
                long_run(33)
        while len(ref) + len(seq) + 1 < t0:
            same(1)
        refs.append(np.array(ref, np.uint8)); seqs.append(np.array(seq, np.uint8)); cigs.append("".join(cig))
    return refs, seqs, cigs, mbr


def chunks_of(prep):
    """per chunk of one read's model.prep(): (steps of the chunk, refw rows of the chunk, geometry dict)"""
    out, ro = [], 0
    for brk, nrows, row0, col0, drows, dcols, _ in prep["geom"].tolist():
        out.append((prep["steps"][brk:brk + nrows - 1], prep["refw"][ro:ro + dcols + 1],
                    dict(brk=brk, nrows=nrows, row0=row0, col0=col0, drows=drows, dcols=dcols)))
        ro += dcols + 1
    return out


def plain_range(steps, g, r):
    """[lo, hi) of the chunk's anti-diagonals that are plain (cell.hpp step_is_plain), and the local column of each"""
    ins = np.concatenate([[0], np.cumsum(steps != 0)])
    dl = np.arange(g["nrows"]) - ins
    plain = (ins - r >= 6) & (dl - r >= 6) & (ins + r <= g["drows"]) & (dl + r <= g["dcols"])
    idx = np.nonzero(plain)[0]
    return (int(idx[0]), int(idx[-1]) + 1, dl) if len(idx) else (0, 0, dl)


def survey(prep, r):
    """What the read's annotation holds for the queues, counted over the columns that lie in the band during a plain
    range: phases (chunk-local column mod 64) of the rare columns and of the first column of every rare stretch, columns with L >= 32,
    chunks away from column 0 that have a plain range, chunks that have none, 'D' steps of plain ranges, chunks in which the
    band runs past the reference's end (sentinel words from the queue)."""
    rare_phases, entry_phases, n_big, n_plain_inner, n_noplain, n_dsteps, longest_d = set(), set(), 0, 0, 0, 0, 0
    n_sentinel, nw = 0, (2 * r + 1 + 63) // 64
    for steps, refw, g in chunks_of(prep):
        n_sentinel += int((steps == 0).sum()) + 64 * nw - r > g["dcols"]      # the last wave's queue ran beyond the chunk's columns
        lo, hi, dl = plain_range(steps, g, r)
        if lo >= hi:
            n_noplain += 1
            continue
        n_plain_inner += g["col0"] != 0
        d = (steps[lo:hi - 1] == 0)
        n_dsteps += int(d.sum())
        run = 0
        for x in d.tolist():
            run = run + 1 if x else 0
            longest_d = max(longest_d, run)
        j0, j1 = int(dl[lo]), min(int(dl[hi - 1]) + r, g["dcols"])
        cols = np.arange(j0, j1 + 1)
        w = refw[j0:j1 + 1]
        assert ((w[:, 2] & DSC_RARE) != 0).tolist() == ((((w[:, 2] | w[:, 3]) & DSC_BIGL) != 0) | ((w[:, 3] & DSC_MORE) != 0)).tolist()
        rare = (w[:, 2] & DSC_RARE) != 0
        rare_phases |= set((cols[rare] % 64).tolist())
        entry_phases |= set((cols[1:][rare[1:] & ~rare[:-1]] % 64).tolist())      # first column of a rare stretch
        n_big += int((((w[:, 2] | w[:, 3]) & DSC_BIGL) != 0).sum())
    return dict(rare_phases=rare_phases, entry_phases=entry_phases, n_big=n_big, n_plain_inner=n_plain_inner, n_noplain=n_noplain,
                n_dsteps=n_dsteps, longest_d=longest_d, n_chunks=len(prep["geom"]), n_sentinel=n_sentinel)
