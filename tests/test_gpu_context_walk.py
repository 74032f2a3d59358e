"""Every entry point after every other on ONE long-lived context (tests/context_walk_cases.py: thirteen operations, each with a
CPU reference; tests/test_context_walk_cases.py shows on the CPU what they hold and that the loop names the right pair).

The other GPU tests make a context per test or per call, whose buffers are new -- and new device memory is often zero.  Here a
context runs the operations along an Eulerian circuit of all 169 ordered pairs, so every operation meets the buffers, cursors,
work-set rotation, stream choice, device FASTA and settings that every other one (and itself) left: a buffer that has grown
and now serves a smaller call, ws.out after each of its output modes, in_seqs / in_off / out after each annotation entry,
cms_raw / cms_off between the recount and the purity counts, an error in front of a file run.  After every operation the result
is the CPU reference's -- bytes, integers and status exactly, the purity scores within the bound of tests/test_gpu_purity.py --
and what the reference does not hold (a coded file, its index) is what the operation's first occurrence gave.  A failure names
the pair and its index in the walk."""
import pytest

import context_walk_cases as cw

pytestmark = pytest.mark.gpu

WALK = [cw.NAMES[k] for k in cw.walk(len(cw.NAMES))]
QUARTERS = cw.quarters(WALK, 4)
_first = {}                  # operation -> its first result in this session: every later occurrence, in any quarter, repeats it


def _report(failures):
    return "\n".join(map(repr, failures))


@pytest.mark.parametrize("quarter", range(4))
def test_walk_quarter(quarter, tmp_path):
    """a fresh context per quarter; the quarters overlap by one operation, so no pair is lost at a cut"""
    names = QUARTERS[quarter]
    offset = sum(len(q) - 1 for q in QUARTERS[:quarter])
    assert WALK[offset:offset + len(names)] == names
    ctx = cw.shipped().context()
    try:
        failures = cw.walk_on(ctx, tmp_path, names, offset=offset, first=_first)
    finally:
        ctx.close()
    assert not failures, _report(failures)


def test_two_contexts_interleaved(tmp_path):
    """Two contexts alive together -- A with the shipped tables, B with a table family of max_n = 4, max_l = 20 -- take turns
    over all ordered pairs of four operations, each against its own references: the automatic traceback budget divides by the
    live contexts, and each context's device tables, FASTA copy and work sets are its own"""
    names = ("align30", "align100_groups", "np_info", "file_sam")
    order = [names[k] for k in cw.walk(len(names))]
    tables = {"A": cw.shipped(), "B": cw.family("random_4_20")}
    assert (tables["B"].max_n, tables["B"].max_l) == (4, 20)
    ctxs = {k: t.context() for k, t in tables.items()}
    first = {k: {} for k in tables}
    try:
        failures = []
        for k, name in enumerate(order):                         # A, B, A, B ...: each walks the circuit, the other one in between
            for which in ("A", "B"):
                found = cw.walk_on(ctxs[which], tmp_path, [name], offset=k, first=first[which], table=cw.ops(tables[which]),
                                   before=order[k - 1] if k else None)
                failures += [f"{which}: {f!r}" for f in found]
                assert not any(f.why.startswith("raised") for f in found), "\n".join(failures)      # nothing more on a context that raised
    finally:
        for c in ctxs.values():
            c.close()
    assert not failures, "\n".join(failures)


def test_settings_do_not_leak(tmp_path):
    """every npore_ctx_set key at a legal value that is not its default; each operation sets what it names and nothing else, and
    gives the reference's result: no other setting reaches a result"""
    ctx = cw.shipped().context()
    try:
        failures = []
        for name in ("align30", "purity64", "file_sam"):
            for key, (_, other) in cw.SETTINGS.items():
                ctx.set(key, other)
            failures += cw.walk_on(ctx, tmp_path, [name], first=_first)
            assert not any(f.why.startswith("raised") for f in failures), _report(failures)
        for key, (default, _) in cw.SETTINGS.items():            # ... and back at the defaults, behind the runs above
            ctx.set(key, default)
        failures += cw.walk_on(ctx, tmp_path, ["file_sam", "purity64", "align30"], offset=3, first=_first)
    finally:
        ctx.close()
    assert not failures, _report(failures)
