"""fill_kernel's per-wave reference-word queues (kernels.hpp ref_q / gen_fill_asm.py mode_d: every wave of a chunk takes the
reference words that enter at its last lane from its own queue) against the oracle: every string and status, at the wave
counts where the roles differ, on reads built so that a wrong queue base, a wrong refill phase or a missed rare-path test
shows (tests/ref_queue_cases.py)."""
import pytest

import oracle
from npore_amd import aln
from ref_queue_cases import make_reads, survey

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


def check_inputs(refs, seqs, cigs, mbr, r, n_full, min_ref):
    """the properties the case is about, from the host twin's annotation: they cannot be absent without the test failing.
    Rare columns: over the reads of a case there is one at every phase (column mod 64) of the queue, and every one of them is
    tested as it enters (a 'D' step tests the entering descriptor whether or not the column before it was rare), so rare
    descriptors are met at all 64 queue positions; the FIRST column of a rare stretch, where the test's result changes
    from the step before, is asked for at 8 phases or more only."""
    from model import model
    rare, entry = set(), set()
    for k, (ref, seq, cig) in enumerate(zip(refs, seqs, cigs)):
        assert min_ref <= len(ref) and len(ref) >= 10 * 64
        s = survey(model.prep(ref, seq, cig, max_b_rows=mbr), r)
        # >= 3 chunks: a plain range in all but the tail (so also in chunks whose column origin is not 0), none in the tail
        assert s["n_chunks"] == n_full + 1 and s["n_plain_inner"] == n_full - 1 and s["n_noplain"] == 1, (k, s)
        assert s["n_big"] >= 32 and s["n_dsteps"] >= 128, (k, s)               # L >= 32 columns in the band of a plain range
        assert s["n_sentinel"] >= 1, (k, s)                                     # the band runs past the reference's end: sentinel words from the queue
        assert k % 2 or s["longest_d"] >= 65, (k, s)                           # a deletion that drains a queue and crosses a refill
        rare |= s["rare_phases"]
        entry |= s["entry_phases"]
    assert rare == set(range(64)) and len(entry) >= 8, (sorted(rare), sorted(entry))


def oracle_all(refs, seqs, cigs, tables, r, mbr):
    sub, nps = tables
    return [oracle.align(refs[k], seqs[k], cigs[k], sub, nps, r=r, max_b_rows=mbr, return_status=True) for k in range(len(refs))]


# r: waves per chunk -- 32: first + last only; 64: one middle wave; 100: four; 200: seven, on two SIMDs; 256: nine, fill_kernel<0>
@pytest.mark.parametrize("r,n_reads,t0,n_full,min_ref", [(32, 12, 2600, 2, 700), (64, 12, 2600, 2, 700), (100, 12, 2600, 2, 700),
                                                         (200, 8, 2600, 2, 700), (256, 8, 5000, 3, 2300)])
def test_every_wave_feeds_its_own_reference_words(ctx, tables, r, n_reads, t0, n_full, min_ref):
    refs, seqs, cigs, mbr = make_reads(7000 + r, n_reads, t0, n_full, r)
    check_inputs(refs, seqs, cigs, mbr, r, n_full, min_ref)
    got, st = ctx.align_batch(refs, seqs, cigs, r=r, max_b_rows=mbr, return_status=True)
    for k, (want, wst) in enumerate(oracle_all(refs, seqs, cigs, tables, r, mbr)):
        assert got[k] == want and st[k] == wst, (r, mbr, k)


def test_same_call_four_times_on_one_context(ctx, tables):
    r = 100
    refs, seqs, cigs, mbr = make_reads(7777, 64, 2600, 2, r)
    want = oracle_all(refs, seqs, cigs, tables, r, mbr)
    first = None
    for rep in range(4):
        got, st = ctx.align_batch(refs, seqs, cigs, r=r, max_b_rows=mbr, return_status=True)
        if first is None:
            first = (list(got), list(st))
        assert list(got) == first[0] and list(st) == first[1], rep
        for k, (w, wst) in enumerate(want):
            assert got[k] == w and st[k] == wst, (rep, k)
