"""The column cache of the fill step (gen_fill_asm.py: what a step derives from the column descriptor is computed in a 'D'
step and where the text is entered, and read from registers by the 'I' steps that follow) against the oracle: every string
and status, at the wave counts where the roles differ, on reads built so that a stale or clobbered cache shows
(tests/step_cache_cases.py)."""
import collections

import pytest

import oracle
from npore_amd import aln
from step_cache_cases import INS_LENGTHS, make_reads, n_waves, role_of, survey

pytestmark = pytest.mark.gpu

# r: waves per chunk -- 30: the only wave; 32: first + last; 64: one middle wave; 100: four; 256: nine, fill_kernel<0>
CASES = [(30, 12, 2600, 2, 700), (32, 12, 2600, 2, 700), (64, 12, 2600, 2, 700), (100, 12, 2600, 2, 700), (256, 8, 5000, 3, 2200)]
# the last wave of these bands holds the band's edge column alone: no band-interior column, so no candidate of any kind
EDGE_ONLY_LAST = {32, 64, 256}


@pytest.fixture(scope="module")
def ctx(tables):
    sub, nps = tables
    c = aln.Context(sub, nps, max_n=6, max_l=100, device=0)
    yield c
    c.close()


def check_inputs(refs, seqs, cigs, mbr, r, n_full, min_ref):
    """the properties the case is about, from the host twin's annotation: they cannot be absent without the test failing"""
    from model import model
    nw = n_waves(r)
    roles = {role_of(w, nw) for w in range(nw)}
    assert roles == ({0} if nw == 1 else {1, 3} if nw == 2 else {1, 2, 3})
    tot = {role: collections.Counter() for role in roles}
    longest_i, runs = 0, set()
    for k, (ref, seq, cig) in enumerate(zip(refs, seqs, cigs)):
        assert min_ref <= len(ref) <= 2600, (k, len(ref))
        s = survey(model.prep(ref, seq, cig, max_b_rows=mbr), r)
        assert s["n_chunks"] >= 3 and s["n_plain"] == n_full, (k, s)
        longest_i = max(longest_i, s["longest_i"])
        for role, d in s["roles"].items():
            tot[role].update({key: int(v) for key, v in d.items()})
        runs |= {len(x) for x in cig.replace("=", " ").replace("D", " ").split()}
        assert k % 4 or "D" * 65 + "I" in cig, k              # a deletion that drains a queue, an insertion right behind it
    assert set(INS_LENGTHS) <= runs, sorted(runs)
    assert longest_i >= 65, longest_i                         # inside a plain range: across a window, a block end and a refill
    for role, c in tot.items():
        assert c["entry_i"] >= 1 and c["window_i"] >= 1, (r, role, c)
        if role == 3 and r in EDGE_ONLY_LAST:
            assert c["interior"] == 0 and c["two_i"] == 0 and c["len_i"] == 0, (r, role, c)
        else:
            assert c["interior"] and c["two_i"] >= 1, (r, role, c)
            assert c["len_i"] >= 1, (r, role, c)              # a LEN candidate past the n-mer filter inside an insertion
        if role in (0, 1):                                    # the wave that holds band column 0 queues the read words
            assert c["refill_i"] >= 1, (r, role, c)           # a read-word refill (a block end) between two 'I' steps


def oracle_all(refs, seqs, cigs, tables, r, mbr):
    sub, nps = tables
    return [oracle.align(refs[k], seqs[k], cigs[k], sub, nps, r=r, max_b_rows=mbr, return_status=True) for k in range(len(refs))]


@pytest.mark.parametrize("r,n_reads,t0,n_full,min_ref", CASES)
def test_i_steps_read_what_the_last_d_step_derived(ctx, tables, r, n_reads, t0, n_full, min_ref):
    refs, seqs, cigs, mbr = make_reads(9000 + r, n_reads, t0, n_full, r)
    check_inputs(refs, seqs, cigs, mbr, r, n_full, min_ref)
    got, st = ctx.align_batch(refs, seqs, cigs, r=r, max_b_rows=mbr, return_status=True)
    for k, (want, wst) in enumerate(oracle_all(refs, seqs, cigs, tables, r, mbr)):
        assert got[k] == want and st[k] == wst, (r, mbr, k)


def test_same_call_four_times_on_one_context(ctx, tables):
    r = 100
    refs, seqs, cigs, mbr = make_reads(9777, 32, 2600, 2, r)
    want = oracle_all(refs, seqs, cigs, tables, r, mbr)
    for rep in range(4):
        got, st = ctx.align_batch(refs, seqs, cigs, r=r, max_b_rows=mbr, return_status=True)
        for k, (w, wst) in enumerate(want):
            assert got[k] == w and st[k] == wst, (rep, k)
