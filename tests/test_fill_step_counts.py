"""Static instruction counts of the generated fill step (npore_amd/csrc/gen_fill_asm.py), recounted on the text the way
DESIGN.md section 4.1 states them: from the label of a step to the branch to the next step's label along the common path
(no conditional branch taken: one SHR candidate per column, no LEN candidate, the neighbour waves ready, the next step an
'I' step inside the same block).  Classes only: vector ALU (v_*), LDS (ds_*), vector memory (global_*), scalar (every
other s_* instruction, branches included); s_waitcnt and s_nop are counted apart.

What an 'I' step must NOT hold is the point of the column cache: the fields of the column descriptor rc0 are derived in
a 'D' step (and where the text is entered), an 'I' step reads them from registers and issues one lane-table read."""
import importlib.util
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "npore_amd", "csrc")

# role (0 only wave, 1 first, 2 middle, 3 last) -> kind -> (vector, scalar, LDS)
COUNTS = {
    0: {"i": (72, 11, 5), "d": (83, 15, 6)},
    1: {"i": (74, 18, 9), "d": (86, 21, 11)},
    2: {"i": (69, 13, 10), "d": (81, 17, 11)},
    3: {"i": (73, 16, 8), "d": (86, 20, 8)},
}


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_fill_asm", os.path.join(CSRC, "gen_fill_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


def common_path(lines, kind):
    """the instructions from the step's label to the branch to (or the fall-through into) the next step's label"""
    i = lines.index("mode_%s_%%=:" % kind) + 1
    out = []
    while True:
        ln = lines[i]
        i += 1
        if ln.endswith(":"):
            if ln.startswith("mode_"):
                return out
            continue
        out.append(ln)
        if ln.startswith("s_branch"):
            assert ln.split()[1].startswith("mode_"), ln      # the common path has no other unconditional branch
            return out


def classes(path):
    ops = [ln.split()[0] for ln in path]
    vector = sum(op.startswith("v_") for op in ops)
    lds = sum(op.startswith("ds_") for op in ops)
    scalar = sum(op.startswith("s_") and op not in ("s_waitcnt", "s_nop") for op in ops)
    assert vector + lds + scalar + sum(op.startswith("global_") or op in ("s_waitcnt", "s_nop") for op in ops) == len(ops)
    return vector, scalar, lds


@pytest.mark.parametrize("role", range(4))
def test_common_path_counts(gen, role):
    lines = gen.gen_role(role)
    for kind in "id":
        assert classes(common_path(lines, kind)) == COUNTS[role][kind], (role, kind)


@pytest.mark.parametrize("role", range(4))
def test_i_step_derives_nothing_from_the_descriptor(gen, role):
    path = common_path(gen.gen_role(role), "i")
    perm = [ln for ln in path if ln.startswith("ds_bpermute_b32")]
    assert len(perm) == 1 and perm[0].endswith("%[tab]"), perm           # the one table that changes every step
    # the five field extractions: summary bits, lane-table index, start flag, score-table base, period
    rc0 = re.escape("%[rc0]")
    for pat in (r"v_and_b32 \S+ (0xbc|%\[livebc\]), " + rc0, r"v_and_b32 \S+ 28, " + rc0, r"v_cmp_gt_i32 \S+ 0, " + rc0,
                r"v_bfe_u32 \S+ " + rc0 + ", 15, 16", r"v_bfe_u32 \S+ " + rc0 + ", 2, 3"):
        assert not [ln for ln in path if re.match(pat, ln)], (role, pat)
    # nor the wave-level tests of the summary bits: the decisions are scalar
    assert not [ln for ln in path if re.match(r"v_cmp_lt_u32 \S+ 28, ", ln) or re.match(r"v_cmp_ne_u32 \S+ 0, " + gen.SMR + "$", ln)], role
    # the 'D' step of the same role does hold them: that is where the cache is written
    dpath = common_path(gen.gen_role(role), "d")
    assert sum(bool(re.match(r"v_bfe_u32 \S+ " + rc0, ln)) for ln in dpath) == 2
    assert sum(ln.startswith("ds_bpermute_b32") for ln in dpath) == 2


@pytest.mark.parametrize("role", range(4))
def test_nothing_but_the_d_step_and_the_entry_writes_the_cache(gen, role):
    """the cache's registers are written in exactly two places: the head of the text and the 'D' step, both in front of
    the hand-shake poll; never by the SHR / LEN passes, the refills, the block end or the polls"""
    lines = gen.gen_role(role)
    cache = ("%[cidx]", "%[crcp]", "%[cbase]", "%[cper]", "%[csf]", "%[ctwo]", "%[cnone]")
    label = None
    writers = {}
    for ln in lines:
        if ln.endswith(":"):
            label = ln[:-4]
            continue
        # Assumes what holds for every instruction the generator emits with a cache operand: the first operand is the
        # instruction's only destination, named alone (no register range, no second destination such as a carry-out);
        # s_cmp* and ds_write* have no destination, their first operand is a source.
        dst = ln.split(None, 1)[1].split(",")[0].strip() if " " in ln else ""
        if dst in cache and not ln.startswith(("s_cmp", "ds_write")):
            writers.setdefault(dst, []).append(label)
    want = [c for c in cache if c != "%[cnone]" or role in (1, 3)]
    assert sorted(writers) == sorted(want), (role, writers)
    for dst, where in writers.items():
        assert where == [None, "mode_d"], (role, dst, where)
