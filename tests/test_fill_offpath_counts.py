"""Static instruction counts of the OUT-OF-LINE blocks of the generated fill step (npore_amd/csrc/gen_fill_asm.py): the LEN
loop and the two-candidate block of the SHR pass, recounted on the text the way tests/test_fill_step_counts.py recounts the
common path.  These blocks run for one or two live lanes and the whole wave (and the chunk's other waves, which wait for
it) pays for every instruction of them, so their size is pinned like the common path's.  Classes: vector ALU (v_*),
scalar (s_* but s_waitcnt / s_nop, branches included), LDS (ds_*).

The paths, per wave role and step kind (the counts are the same for all eight):

  block                                                    this text        the text before it
                                                          (v,  s, LDS)         (v,  s, LDS)
  failing LEN iteration, no match yet in the step          ( 9,  4, 0)         (12,  4, 0)
      len_body ... the filter's branch, then the test of the periods left (len_topA)
  passing LEN iteration, the step's first match            (35,  7, 6)         (46,  9, 6)
      len_body ... len_top, score from the LDS table
  failing LEN iteration behind a match                     ( 9,  4, 0)         (10,  4, 0)
      len_top ... the filter's branch
  passing LEN iteration behind a match                     (36,  9, 6)         (45, 11, 6)
      len_top ... the branch back to len_top, score from the LDS table
  two-candidate block of the SHR pass                      (35,  1, 5)         (37,  1, 6)
      shr_two ... the branch to shr_done2                   2 s_nop              3 s_nop

(Before: one loop whose entry set LENV / LENRUN up whether or not a lane's n-mer matched, and whose exit was always the
LEN variant of the tail.  Now a step in which no n-mer matches leaves through len_none, the common tail.)"""
import importlib.util
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "npore_amd", "csrc")

FAIL_FIRST, PASS_FIRST, FAIL_LATER, PASS_LATER, TWO = (9, 4, 0), (35, 7, 6), (9, 4, 0), (36, 9, 6), (35, 1, 5)
TWO_NOPS = 2
CACHE = ("%[cidx]", "%[crcp]", "%[cbase]", "%[cper]", "%[csf]", "%[ctwo]", "%[cnone]")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_fill_asm", os.path.join(CSRC, "gen_fill_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


def lab(name):
    return name + "_%=:"


def walk(lines, start, stop_label=None, stop_op=None):
    """the instructions behind label `start`, labels skipped, up to label `stop_label` (exclusive) or the first
    instruction that begins with `stop_op` (inclusive)"""
    out = []
    for ln in lines[lines.index(lab(start)) + 1:]:
        if stop_label and ln == lab(stop_label):
            return out
        if ln.endswith(":"):
            continue
        out.append(ln)
        if stop_op and ln.startswith(stop_op):
            return out
    raise AssertionError((start, stop_label, stop_op))


def lds_case(path):
    """without the block that reads the score from global memory (`big`, not taken: between the branch to len_lds and
    the instruction that enables all lanes again)"""
    out, skip = [], False
    for ln in path:
        if skip:
            skip = not ln.startswith("s_mov_b64 exec, -1")
            continue
        out.append(ln)
        skip = ln.startswith("s_cbranch_vccz len_lds")
    assert not skip
    return out


def classes(path):
    ops = [ln.split()[0] for ln in path]
    vector = sum(op.startswith("v_") for op in ops)
    lds = sum(op.startswith("ds_") for op in ops)
    scalar = sum(op.startswith("s_") and op not in ("s_waitcnt", "s_nop") for op in ops)
    assert vector + lds + scalar + sum(op in ("s_waitcnt", "s_nop") for op in ops) == len(ops), path      # (no vector memory here)
    return vector, scalar, lds


def blocks(lines, kind):
    s = "_" + kind
    return {
        "fail_first": walk(lines, "len_body" + s, stop_op="s_cbranch_scc0") + walk(lines, "len_topA" + s, stop_op="s_cbranch_vccz"),
        "pass_first": lds_case(walk(lines, "len_body" + s, stop_label="len_top" + s)),
        "fail_later": walk(lines, "len_top" + s, stop_op="s_cbranch_scc0"),
        "pass_later": lds_case(walk(lines, "len_top" + s, stop_op="s_branch len_top")),
        "two": walk(lines, "shr_two" + s, stop_op="s_branch"),
    }


@pytest.mark.parametrize("role", range(4))
def test_offpath_counts(gen, role):
    lines = gen.gen_role(role)
    for kind in "ID":
        b = blocks(lines, kind)
        got = {k: classes(v) for k, v in b.items()}
        assert got == dict(fail_first=FAIL_FIRST, pass_first=PASS_FIRST, fail_later=FAIL_LATER, pass_later=PASS_LATER, two=TWO), (role, kind)
        assert sum(ln.startswith("s_nop") for ln in b["two"]) == TWO_NOPS, (role, kind)
        # the lane-table reads: two per evaluated LEN candidate, two for the second SHR candidate
        assert sum(ln.startswith("ds_bpermute_b32") for ln in b["pass_first"]) == 2
        assert sum(ln.startswith("ds_bpermute_b32") for ln in b["two"]) == 2


@pytest.mark.parametrize("role", range(4))
def test_the_paths_are_the_ones_the_text_takes(gen, role):
    """the walks above follow the text's own branches: where a failing filter goes, where a step without a match leaves,
    where the block of a step's first match falls through to"""
    lines = gen.gen_role(role)
    for kind in "ID":
        s = "_" + kind
        b = blocks(lines, kind)
        assert b["fail_first"][-1] == "s_cbranch_vccz len_none%s_%%=" % s and "s_cbranch_scc0 len_topA%s_%%=" % s in b["fail_first"]
        assert b["fail_later"][-1] == "s_cbranch_scc0 len_top%s_%%=" % s
        assert b["fail_later"][1] == "s_cbranch_vccz len_done%s_%%=" % s
        assert not [ln for ln in b["pass_first"] if ln.startswith("s_branch")]            # falls into len_top
        assert b["two"][-1] == "s_branch shr_done2%s_%%=" % s
        # len_none is the common path's own continuation: the label stands right behind the LEN entry test
        i = lines.index(lab("len_none" + s))
        assert lines[i - 1] == "s_cbranch_vccnz len_body%s_%%=" % s and lines[i - 2].startswith("v_cmp_ne_u32 vcc, 0, ")
        assert lines[i + 1] == "s_waitcnt lgkmcnt(0)"                                      # mat_part, no LEN candidate
        # a step without a match never set up, and its tail never reads, LENV / LENRUN; LENST is written by matches only
        assert not [ln for ln in b["fail_first"] if re.search(r"\b(%s|%s|%s)\b" % (gen.LENV, gen.LENRUN, gen.LENST), ln)]


@pytest.mark.parametrize("role", range(4))
def test_periods_highest_first(gen, role):
    """every iteration takes the lane's HIGHEST period left (find-first-bit from the high end, k = 31 - that, the bits
    below k stay), and a later candidate wins on strictly-less only: the first writer wins a tie"""
    lines = gen.gen_role(role)
    for kind in "ID":
        b = blocks(lines, kind)
        for name in ("pass_first", "pass_later"):
            p = b[name]
            i = next(n for n, ln in enumerate(p) if ln.startswith("v_ffbh_u32"))
            k, flags = p[i].split()[1].rstrip(","), p[i].split()[2]
            assert p[i + 1] == "v_sub_u32 %s, 31, %s" % (k, k)
            assert p[i + 2] == "v_bfe_u32 %s, %s, 0, %s" % (flags, flags, k)
            assert not [ln for ln in p if ln.startswith("v_ffbl")]
            cmps = [ln for ln in p if ln.startswith("v_cmp_lt_f32 vcc")]
            assert len(cmps) == 1 and cmps[0].endswith(", %[ev]" if name == "pass_first" else ", " + gen.LENV), cmps
            assert not [ln for ln in p if ln.startswith("v_cmp_le_f32")]


@pytest.mark.parametrize("role", range(4))
def test_offpath_blocks_do_not_write_the_column_cache(gen, role):
    lines = gen.gen_role(role)
    for kind in "ID":
        b = blocks(lines, kind)
        full = walk(lines, "len_topA_" + kind, stop_label="len_done_" + kind)              # the whole loop, `big` included
        for path in list(b.values()) + [full]:
            for ln in path:
                if " " not in ln or ln.startswith(("s_cmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop", "ds_write")):
                    continue
                dst = ln.split(None, 1)[1].split(",")[0].strip()
                assert dst not in CACHE, (role, kind, ln)
