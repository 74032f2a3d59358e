"""The index identity behind the per-wave reference-word queues of fill_kernel (kernels.hpp ref_q, gen_fill_asm.py mode_d),
in plain Python on the host twin of the prep kernels (tests/model): no GPU.

A chunk's band is 2r + 1 columns on NW = ceil((2r + 1) / 64) waves; lane l of wave cw holds the reference words of local
column del_l + 64 cw + l - r, and a 'D' step moves them one lane down.  Every wave keeps the 64 words that enter next at its
lane 63 in a queue register: base 64 (cw + 1) - r, one word taken per 'D' step, the next 64 loaded when the 64 are used up.
Checked here, for every wave and every 'D' step of random input paths:
  * the k-th word a wave takes is refw[del_l + 64 cw + 63 - r] (del_l = k, the chunk's 'D' steps so far, this one
    included), the sentinel outside [0, dcols];
  * it is the word that lane 0 of the wave above held before the step -- what used to come through the exchange record;
  * every lane then holds the words of its column, and all waves refill at the same 'D' steps.
"""
import numpy as np
import pytest

from ref_queue_cases import DSC_BIGL, DSC_MORE, DSC_RARE, REFW_SENTINEL, chunks_of, make_reads

SENT = (REFW_SENTINEL, 0, 0)


def word(refw, j):
    return (int(refw[j, 0]), int(refw[j, 2]), int(refw[j, 3])) if 0 <= j < len(refw) else SENT


def check_chunk(steps, refw, dcols, r):
    assert len(refw) == dcols + 1
    nw = (2 * r + 1 + 63) // 64
    lanes = [[word(refw, 64 * cw + l - r) for l in range(64)] for cw in range(nw)]
    base = [64 * (cw + 1) - r for cw in range(nw)]
    idx = [0] * nw
    queue = [[word(refw, base[cw] + l) for l in range(64)] for cw in range(nw)]
    del_l, refills = 0, [[] for _ in range(nw)]
    for s in steps.tolist():
        if s != 0:
            continue
        del_l += 1
        below = [lanes[cw][0] for cw in range(nw)]          # lane 0 of every wave before the step
        for cw in range(nw):
            if idx[cw] >= 64:
                idx[cw] -= 64
                base[cw] += 64
                queue[cw] = [word(refw, base[cw] + l) for l in range(64)]
                refills[cw].append(del_l)
            w = queue[cw][idx[cw]]
            idx[cw] += 1
            assert w == word(refw, del_l + 64 * cw + 63 - r), (r, cw, del_l)
            if cw + 1 < nw:
                assert w == below[cw + 1], (r, cw, del_l)
            lanes[cw] = lanes[cw][1:] + [w]
    for cw in range(nw):
        assert lanes[cw] == [word(refw, del_l + 64 * cw + l - r) for l in range(64)], (r, cw)
        assert refills[cw] == refills[0] == list(range(65, del_l + 1, 64)), (r, cw)
    return del_l, nw


@pytest.mark.parametrize("r", [32, 64, 100, 200, 256])
def test_queue_word_is_the_column_entering_at_lane_63(r):
    from model import model
    refs, seqs, cigs, mbr = make_reads(500 + r, 2, 4600 if r == 256 else 2600, 3 if r == 256 else 2, r)
    rng = np.random.default_rng(r)
    # a random path as well: independent bases, a cigar of random runs
    ops = "".join(rng.choice(list("=ID"), p=[0.6, 0.2, 0.2]) * int(rng.integers(1, 40)) for _ in range(120))
    refs.append(rng.integers(1, 5, sum(c != "I" for c in ops)).astype(np.uint8))
    seqs.append(rng.integers(1, 5, sum(c != "D" for c in ops)).astype(np.uint8))
    cigs.append(ops)
    n_d = n_sent = 0
    for ref, seq, cig in zip(refs, seqs, cigs):
        for m in (mbr, 20000):
            for steps, refw, g in chunks_of(model.prep(ref, seq, cig, max_b_rows=m)):
                d, nw = check_chunk(steps, refw, g["dcols"], r)
                n_d += d
                n_sent += d + 64 * nw - r > g["dcols"]       # the last wave took words from beyond the chunk's columns
    assert n_d >= 10 * 64 and n_sent > 0


def test_homopolymers_of_six_to_nine_alone_give_no_rare_column():
    """Why tests/ref_queue_cases.py takes its rare columns from runs of 33 ... 55 bases: under np_info's "longest" rule a
    homopolymer of 6 ... 9 is an n-polymer for period 1 alone, so it sets neither DSC_MORE (a third candidate period) nor
    DSC_BIGL, and with them no DSC_RARE.  The same reads with the long runs left out: homopolymers of >= 6 in every
    reference, no rare descriptor in any column."""
    from model import model
    refs, seqs, cigs, mbr = make_reads(900, 4, 2600, 2, 100, long_runs=False)
    for ref, seq, cig in zip(refs, seqs, cigs):
        edges = np.flatnonzero(np.diff(ref.astype(np.int32)) != 0)
        runs = np.diff(np.concatenate([[-1], edges, [len(ref) - 1]]))
        assert (runs >= 6).sum() >= 10 and runs.max() < 32, runs.max()       # (equal neighbouring bases may lengthen a run; 32 is DSC_BIGL's)
        for steps, refw, g in chunks_of(model.prep(ref, seq, cig, max_b_rows=mbr)):
            assert not ((refw[:, 2] | refw[:, 3]) & DSC_BIGL).any()
            assert not (refw[:, 3] & DSC_MORE).any() and not (refw[:, 2] & DSC_RARE).any()
