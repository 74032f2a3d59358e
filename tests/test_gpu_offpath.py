"""The out-of-line blocks of the fill step's text (npore_amd/csrc/gen_fill_asm.py: the LEN loop -- filter, evaluation from the
LDS table and from global memory, the exit of a step in which no n-mer matches -- and the two-candidate block of the SHR
pass) against the oracle: every string and status, at the bands where the wave roles differ, on short reads built so that
every path of those blocks is taken (tests/offpath_cases.py says how, and counts it from the host twin's annotation).

Which of a column's two SHR candidates wins, and whether they tie, takes the scores: a twin of the fill that notes what
the two-candidate block decided for every cell (tests/model/shr2_twin.cpp: the product's cell.hpp on the host) says it.
Every case runs under two table sets: the shipped one, and one whose entries and penalties lie on a grid of 1/4
(table_families.grid: ties everywhere), under which every role that holds two-candidate columns meets, in steps of the
text, a column whose second candidate wins AND one where it ties with the first, which must stay."""
import collections

import pytest

import oracle
from npore_amd import aln
import table_families
from offpath_cases import KEYS, make_reads, shr2_notes, shr2_outcomes, survey
from step_cache_cases import n_waves, role_of

pytestmark = pytest.mark.gpu

# r, reads, anti-diagonals per read, chunks per read.  30: the only wave; 32: two waves, the last holds the band's edge column
# alone; 64: a middle wave, the last again edge-only; 100: four waves, every role with band-interior columns
CASES = [(30, 24, 1100, 4), (32, 24, 1100, 4), (64, 24, 1150, 4), (100, 24, 1180, 3)]
EDGE_ONLY_LAST = {32, 64}


TABLE_SETS = ["shipped", "grid"]


@pytest.fixture(scope="module")
def table_sets(tables):
    """name -> (sub, np, indel_start, indel_extend), max_n = 6 and max_l = 100 in both"""
    sub, nps = tables
    return {"shipped": (sub, nps, 5.0, 1.0), "grid": table_families.grid(2, 6, 100)}


@pytest.fixture(scope="module")
def ctxs(table_sets):
    out = {name: aln.Context(t[0], t[1], max_n=6, max_l=100, device=0) for name, t in table_sets.items()}
    yield out
    for c in out.values():
        c.close()


def check_inputs(refs, seqs, cigs, mbr, r, n_chunks):
    """the paths the case is about, from the host twin's annotation: a recipe that produces none of one fails"""
    from model import model
    nw = n_waves(r)
    roles = {role_of(w, nw) for w in range(nw)}
    tot = {role: collections.Counter() for role in roles}
    units = set()
    for k, (ref, seq, cig) in enumerate(zip(refs, seqs, cigs)):
        assert len(ref) <= 600 and len(seq) <= 640, (k, len(ref), len(seq))
        s = survey(model.prep(ref, seq, cig, max_b_rows=mbr), r)
        assert s["n_chunks"] == n_chunks and s["n_plain"] == n_chunks - 1, (k, s["n_chunks"], s["n_plain"])
        for role, d in s["roles"].items():
            tot[role].update(d)
        units |= {len(x) for x in cig.replace("=", " ").split()}
    assert {1, 2, 3, 4, 6, 9} <= units, sorted(units)            # insertions of 1, 2, 3 units of 1, 2, 3 bases
    for role, c in tot.items():
        if role == 3 and r in EDGE_ONLY_LAST:
            assert not c["interior"] and not any(c[key] for key in KEYS), (r, role, c)
            continue
        assert c["interior"] and c["text"] >= 100, (r, role, c)
        for key in ("len_fail", "len_pass", "len_big", "two", "two_start", "two_cont"):
            assert c[key] >= 1, (r, role, key, c)
        if role in (1, 2):                       # lane 63 is a band-interior lane of every wave but the last
            assert c["len_lane63"] >= 1, (r, role, c)
        if role in (2, 3):                       # lane 0 of the first wave is the band's edge
            assert c["len_lane0"] >= 1, (r, role, c)
    for key in ("len_two_periods", "len_two_iter"):
        assert sum(c[key] for c in tot.values()) >= 1, (r, key)


def check_outcomes(refs, seqs, cigs, mbr, r, tset, ties_everywhere):
    """what the two-candidate block decides, from the scoring twin: per role that holds such columns, in steps of the text"""
    sub, nps, ist, iex = tset
    from model import model
    nw = n_waves(r)
    tot = {role_of(w, nw): collections.Counter() for w in range(nw)}
    for ref, seq, cig in zip(refs, seqs, cigs):
        o = shr2_outcomes(shr2_notes(ref, seq, cig, sub, nps, ist, iex, mbr, r), model.prep(ref, seq, cig, max_b_rows=mbr), r)
        for role, d in o.items():
            tot[role].update(d)
    for role, c in tot.items():
        if role == 3 and r in EDGE_ONLY_LAST:
            assert not c["two_cells"], (r, role, c)
            continue
        assert c["two_cells"] >= 100 and c["two_win"] >= 1, (r, role, c)
        if ties_everywhere:
            assert c["two_tie"] >= 1, (r, role, c)


@pytest.fixture(scope="module")
def cases(table_sets):
    """inputs and the oracle's answers under both table sets, made once"""
    out = {}
    for r, n_reads, t0, n_chunks in CASES:
        refs, seqs, cigs, mbr = make_reads(7000 + r, n_reads, t0, n_chunks)
        want = {}
        for name, (sub, nps, ist, iex) in table_sets.items():
            want[name] = [oracle.align(refs[k], seqs[k], cigs[k], sub, nps, indel_start=ist, indel_extend=iex, r=r, max_b_rows=mbr,
                                       return_status=True) for k in range(n_reads)]
        out[r] = (refs, seqs, cigs, mbr, want)
    return out


@pytest.mark.parametrize("r,n_reads,t0,n_chunks", CASES)
def test_inputs_take_every_offpath_block(cases, table_sets, r, n_reads, t0, n_chunks):
    refs, seqs, cigs, mbr, _ = cases[r]
    check_inputs(refs, seqs, cigs, mbr, r, n_chunks)
    check_outcomes(refs, seqs, cigs, mbr, r, table_sets["shipped"], False)
    check_outcomes(refs, seqs, cigs, mbr, r, table_sets["grid"], True)


@pytest.mark.parametrize("name", TABLE_SETS)
@pytest.mark.parametrize("r,n_reads,t0,n_chunks", CASES)
def test_offpath_blocks_match_the_oracle(ctxs, table_sets, cases, r, n_reads, t0, n_chunks, name):
    refs, seqs, cigs, mbr, want = cases[r]
    _, _, ist, iex = table_sets[name]
    for rep in range(2):                         # the same call twice on one context
        got, st = ctxs[name].align_batch(refs, seqs, cigs, indel_start=ist, indel_extend=iex, r=r, max_b_rows=mbr, return_status=True)
        for k, (w, wst) in enumerate(want[name]):
            assert got[k] == w and st[k] == wst, (name, r, mbr, rep, k)
