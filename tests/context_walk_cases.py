"""Operations for the walk over one long-lived context (tests/test_gpu_context_walk.py; tests/test_context_walk_cases.py shows on
the CPU that the inputs reach what they name and that the runner reports the right pair).

Every public entry point of a context as one OPERATION: a name, `run(ctx, tmp)` -- which first sets the context settings the
operation names, then calls ONE entry and returns a dict of plain bytes, strings, integers and arrays -- and `want`, the part
of that dict that a CPU reference gives (oracle.align / oracle.get_np_info, the Python glue of npore_amd/cig.py, bam.sam_line,
the library's host twins NativeBam.format_bam*, tests/model's pileup writers), computed once and never from a GPU run.  Keys of
a result that `want` does not hold (the bytes of a coded BAM file, its index) are compared between the occurrences of the
operation only.

An operation sets ONLY the settings it names: every result here is the same under every legal value of the others, which is
what tests/test_gpu_context_walk.py::test_settings_do_not_leak relies on.

walk(n) is an Eulerian circuit of the complete directed graph on n nodes with self-loops: n * n + 1 nodes in which every
ordered pair (a, b) -- b run directly behind a on the same context -- occurs exactly once."""
import argparse
import atexit
import functools
import os
import pathlib
import shutil
import tempfile

import numpy as np

import oracle
import bam_full_cases as fc
import scale_edge_cases as sc
import table_families
from model import cms_model, purity_model
from npore_amd import aln, bam, cfg, cig, purity, synth
from test_bam_out import Hdr, check_index, header_len, members
from test_bed import literal_np_regions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# npore_ctx_set's keys with their defaults (csrc/align_engine.hpp npore_ctx) and a legal value that is not the default
SETTINGS = {"tb_budget_mb": (0, 1), "force_chunks": (0, 1), "coresident": (1, 0), "device_glue": (1, 0), "device_pack": (1, 0),
            "device_inflate": (0, 1), "cms_batch_reads": (4000, 7), "purity_window": (1 << 22, 128), "fill_streams": (2, 1)}
PURITY_BOUND = 1e-14         # tests/test_gpu_purity.py _same: about ten roundings of values <= 1 at 2^-52 each, a factor of four over


# ---- the walk -------------------------------------------------------------------------------------------------------------
def walk(n):
    """Hierholzer on the complete directed graph with self-loops, edges of a node taken in ascending order, from node 0"""
    nxt = [0] * n                      # the next unused edge of node a is a -> nxt[a]
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if nxt[a] < n:
            stack.append(nxt[a])
            nxt[a] += 1
        else:
            out.append(stack.pop())
    return out[::-1]


def quarters(seq, k=4):
    """k contiguous pieces that overlap by one node: every neighbouring pair of `seq` lies in exactly one piece"""
    edges = len(seq) - 1
    cuts = [edges * j // k for j in range(k + 1)]
    return [seq[cuts[j]:cuts[j + 1] + 1] for j in range(k)]


def pairs(seq):
    return list(zip(seq[:-1], seq[1:]))


# ---- comparing results ----------------------------------------------------------------------------------------------------
def identical(a, b):
    """exact equality of two results, arrays by dtype, shape and value"""
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys() and all(identical(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b) and all(identical(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def exact(got, want):
    """every key of `want`, exactly; the first key that differs, or None"""
    for k in want:
        if k not in got or not identical(got[k], want[k]):
            return k
    return None


def purity_same(got, want):
    """integers exactly, the scores within PURITY_BOUND (they are float64 quotients of the integer rows)"""
    bad = exact(got, {k: v for k, v in want.items() if k != "scores"})
    if bad is None and not (got["scores"].shape == want["scores"].shape and
                            (want["scores"].size == 0 or np.abs(got["scores"] - want["scores"]).max() <= PURITY_BOUND)):
        bad = "scores"
    return bad


class Failure:
    def __init__(self, index, prev, op, why):
        self.index, self.prev, self.op, self.why = index, prev, op, why

    def __repr__(self):
        return f"walk[{self.index}]: {self.prev} -> {self.op}: {self.why}"


def run_walk(names, run, want_of, same_of=None, offset=0, first=None, steady_of=None, before=None):
    """The walk's loop: the operations `names` in order through `run(name)`; after each, the result against `want_of(name)`
    (by `same_of(name)`, default `exact`: the first key that differs, or None) and against the result of the operation's first
    occurrence (`first`: {name: result}, kept across calls; `steady_of(name)`: the part of a result that has to repeat, default
    all of it).  Returns the [Failure], each naming the pair (the operation before -> the operation; `before`: what ran in front of
    names[0]) and the index in the walk (`offset`: of names[0]).  A mismatch does not stop the walk; an exception does,
    because nothing is known of the context afterwards."""
    first = {} if first is None else first
    failures = []
    for k, name in enumerate(names):
        prev = names[k - 1] if k else before
        try:
            got = run(name)
        except Exception as e:                                   # noqa: BLE001 (reported with its pair, and the walk ends)
            failures.append(Failure(offset + k, prev, name, f"raised {type(e).__name__}: {e}"))
            break
        bad = (same_of(name) if same_of else exact)(got, want_of(name))
        got = steady_of(name)(got) if steady_of else got
        if bad is not None:
            failures.append(Failure(offset + k, prev, name, f"'{bad}' is not the reference's"))
        elif name in first and not identical(got, first[name]):
            failures.append(Failure(offset + k, prev, name, "differs from the operation's first occurrence"))
        first.setdefault(name, got)
    return failures


# ---- tables ---------------------------------------------------------------------------------------------------------------
class Tables:
    def __init__(self, sub, nps, indel_start=5.0, indel_extend=1.0, max_n=6, max_l=100):
        self.sub, self.nps, self.indel_start, self.indel_extend, self.max_n, self.max_l = sub, nps, indel_start, indel_extend, max_n, max_l

    def context(self):
        return aln.Context(self.sub, self.nps, max_n=self.max_n, max_l=self.max_l, device=0)

    def oracle_kw(self):
        return dict(indel_start=self.indel_start, indel_extend=self.indel_extend, max_n=self.max_n, max_l=self.max_l)


@functools.lru_cache(maxsize=None)
def shipped():
    z = np.load(os.path.join(GOLDEN, "tables.npz"))
    return Tables(z["sub_scores"], z["np_scores"])


@functools.lru_cache(maxsize=None)
def family(name="random_4_20"):
    return Tables(*table_families.load(name))


class _Args:
    """cfg.args as the file entries and bam.get_read_data expect them, for the time of a call"""

    def __init__(self, t, regions):
        self.ns = argparse.Namespace(max_n=t.max_n, max_l=t.max_l, regions=regions, max_reads=0)

    def __enter__(self):
        self.old, cfg.args = cfg.args, self.ns

    def __exit__(self, *exc):
        cfg.args = self.old


# ---- inputs, written once -------------------------------------------------------------------------------------------------
_DIR = None


def inputs_dir():
    global _DIR
    if _DIR is None:
        _DIR = tempfile.mkdtemp(prefix="context_walk_")
        atexit.register(shutil.rmtree, _DIR, True)
    return _DIR


@functools.lru_cache(maxsize=None)
def align_reads(which):
    """(refs, seqs, expanded CIGARs) of an align_batch operation"""
    if which == "align30":
        return synth.make_batch(301, 6, ref_len=600)
    if which == "align100_groups":
        return synth.make_batch(302, 24, ref_len=2500)
    if which == "align260":
        return synth.make_batch(303, 3, ref_len=500)
    if which == "align_final":
        refs, seqs, cigs = synth.make_batch(304, 6, ref_len=500)
        cigs = list(cigs)
        cigs[2] = bytes(cigs[2]) + b"====="                       # five bases more than the read has: refused
        return refs, seqs, cigs
    raise KeyError(which)


ALIGN_SHAPES = {"align30": dict(r=30), "align100_groups": dict(r=100, max_b_rows=333), "align260": dict(r=260), "align_final": dict(r=30)}


@functools.lru_cache(maxsize=None)
def np_info_sequence():
    """20 000 bases: two of launch_np_info's segments of 16 384 and the second one's warm-up; an array across the border"""
    return sc.segment_sequence(np.random.default_rng(305), 0, 20_000, [("hexamer", sc.NP_INFO_SEG)])


@functools.lru_cache(maxsize=None)
def region_slices():
    return sc.region_slices(171)[0]


@functools.lru_cache(maxsize=None)
def read_files(n_reads):
    """bam_full_cases.full_records as BAM + FASTA: clips, tags, mates, both strands; read 7's CIGAR disagrees with its bases"""
    references, refs, records, _ = fc.full_records(n_reads=n_reads)
    d = os.path.join(inputs_dir(), f"reads{n_reads}")
    os.makedirs(d, exist_ok=True)
    bp, fa = fc.write_inputs(pathlib.Path(d), references, refs, records)
    return bp, fa, references, refs, records


LATE_BATCH = 8               # err_contig_late: batches of 8 -- the decoy's read is the 13th, in the second batch


@functools.lru_cache(maxsize=None)
def late_files():
    """the 12 reads and, behind them in coordinate order, one on a contig the FASTA lacks"""
    bp, fa, references, refs, records = read_files(12)
    header = references + [("decoy", 400)]
    decoy = dict(name="onDecoy", flag=0, ref_id=1, pos=20, mapq=30, cigar=[(0, 100)], seq=refs["ctg"][:100], qual=bytes(range(100)))
    mp = os.path.join(inputs_dir(), "late.bam")
    bam.write_bam(mp, header, [{k: v for k, v in r.items() if not k.startswith("_")} for r in records] + [decoy])
    return mp, fa, header


CMS_SEED = 4


@functools.lru_cache(maxsize=None)
def pileup_files():
    """cms_model.make_random_bam: (BAM, FASTA, references, {contig: bases})"""
    d = inputs_dir()
    path, fa = os.path.join(d, "pile.bam"), os.path.join(d, "pile.fasta")
    references, refs = cms_model.make_random_bam(path, CMS_SEED)
    with open(fa, "w") as fh:
        for n, s in refs.items():
            fh.write(f">{n}\n")
            for k in range(0, len(s), 60):
                fh.write(s[k:k + 60] + "\n")
    return path, fa, references, refs


# ---- the references -------------------------------------------------------------------------------------------------------
def want_align(t, which):
    refs, seqs, cigs = align_reads(which)
    res, st = oracle.align_batch(refs, seqs, cigs, t.sub, t.nps, **ALIGN_SHAPES[which], **t.oracle_kw())
    return {"strings": list(res), "status": st.astype(np.int32)}


def glue(raw, ref, seq):
    """the Python statement of realign_read's glue (npore_amd/cig.py) on an op string: the collapsed final CIGAR"""
    return "".join(f"{n}{c}" for c, n in cig.standardize_runs(raw, ref, seq))


def want_align_final(t):
    refs, seqs, cigs = align_reads("align_final")
    w = want_align(t, "align_final")
    return {"strings": ["" if s & 32 else glue(raw, refs[k], seqs[k]) for k, (raw, s) in enumerate(zip(w["strings"], w["status"]))],
            "status": w["status"]}


def reference_finals(t, bp, fa, regions, r=30):
    """(get_read_data tuples, final CIGARs, status) of a BAM by the Python pipeline: get_read_data -> the oracle -> the glue"""
    with _Args(t, regions):
        rds = list(bam.get_read_data(bam.BamFile(bp), bam.read_fasta(fa)))
    pc = [cig.expand_cigar(rd[5]).replace("S", "").replace("H", "") for rd in rds]
    pr, ps = [cig.bases_to_int(rd[9]) for rd in rds], [cig.bases_to_int(rd[7]) for rd in rds]
    raws, st = oracle.align_batch(pr, ps, pc, t.sub, t.nps, r=r, **t.oracle_kw())
    finals = ["" if s & 32 else glue(raw, pr[k], ps[k]) for k, (raw, s) in enumerate(zip(raws, st))]
    return rds, finals, st.astype(np.int32)


def whole(references):
    return [(n, 0, l - 1) for n, l in references]


def want_file_sam(t):
    bp, fa, references, _, _ = read_files(12)
    rds, finals, st = reference_finals(t, bp, fa, whole(references))
    return {"status": st, "text": "".join(bam.sam_line(rd, f) for rd, f, s in zip(rds, finals, st) if not s & 32).encode()}


def _host_twin(t, n_reads, regions, fn):
    bp, fa, references, _, _ = read_files(n_reads)
    rds, finals, st = reference_finals(t, bp, fa, regions)
    nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
    try:
        idx = nb.select(regions)
        assert len(idx) == len(rds) == n_reads
        return {"status": st, "records": fn(nb, nf, idx, finals, st)}
    finally:
        nb.close(); nf.close()


def want_file_bam_tags(t):
    references = read_files(40)[2]
    return _host_twin(t, 40, whole(references), lambda nb, nf, idx, finals, st: nb.format_bam_full(nf, idx, finals, st, md=True, cs="long", de=True))


def want_onepass(t):
    references = read_files(12)[2]
    w = _host_twin(t, 12, whole(references), lambda nb, nf, idx, finals, st: nb.format_bam(idx, finals, st))
    st = w.pop("status")
    return dict(w, selected=12, bad=[(int(k), int(s)) for k, s in enumerate(st) if s])


def want_late(t):
    text = want_file_sam(t)
    lines = text["text"].splitlines(keepends=True)
    # the text of the first j whole batches in front of the decoy's (a refused read has no line)
    return {"prefixes": [b"".join(lines[:int(((text["status"][:j * LATE_BATCH] & 32) == 0).sum())]) for j in range(12 // LATE_BATCH + 1)]}


def want_np_info(t):
    return {"info": oracle.get_np_info(np_info_sequence(), max_n=t.max_n, max_l=t.max_l)}


def want_np_regions(t):
    out = []
    for seq in region_slices():
        out.append(literal_np_regions(np.asarray(oracle.get_np_info(seq, max_n=t.max_n, max_l=t.max_l)), 0, t.max_n) if len(seq) else
                   [[] for _ in range(t.max_n)])
    return {"regions": out}


def pile_ranges():
    return [(n, 0, l) for n, l in pileup_files()[2]]


@functools.lru_cache(maxsize=None)
def confusion_expected(t):
    """cms_model.expected of the pileup BAM: (matrices, the writer's tallies -- its branch counts among them)"""
    path, _, references, refs = pileup_files()
    return cms_model.expected(path, refs, pile_ranges(), t.max_n, t.max_l)


def want_confusion(t):
    mats, tallies = confusion_expected(t)
    return {"matrices": [np.asarray(m, np.int64) for m in mats], "tallies": {k: int(tallies[k]) for k in cms_model.TALLY_NAMES}}


def want_purity(t):
    rows, hb, hi, scores, tallies = purity_model.expected(pileup_files()[0], pile_ranges())
    return {"rows": rows, "base_hist": hb, "ins_hist": hi, "scores": scores, "tallies": {k: int(tallies[k]) for k in purity_model.TALLY_NAMES}}


def purity_windows(window=64):
    """the windows of `window` dense positions that the contigs of the pileup BAM hold"""
    return sum(-(-l // window) for _, l in pileup_files()[2])


# ---- the runs -------------------------------------------------------------------------------------------------------------
def _align(t, which, ctx, settings=(), final=False, min_launches=0):
    for k, v in settings:
        ctx.set(k, v)
    refs, seqs, cigs = align_reads(which)
    got, st = ctx.align_batch(refs, seqs, cigs, t.indel_start, t.indel_extend, return_status=True, final_cigars=final,
                              **dict({"max_b_rows": 20000}, **ALIGN_SHAPES[which]))
    launches = ctx.timing()["launches"]
    assert launches >= min_launches, (which, launches)
    return {"strings": list(got), "status": np.asarray(st, np.int32)}


def _run_np_info(t, ctx, tmp):
    return {"info": ctx.get_np_info(np_info_sequence())}


def _run_np_regions(t, ctx, tmp):
    got = ctx.np_regions(region_slices())
    return {"regions": [[[(int(p), int(p) + (n + 1) * int(r)) for p, r in zip(*got[n][k])] for n in range(t.max_n)]
                        for k in range(len(region_slices()))]}


def _run_confusion(t, ctx, tmp):
    path, fa, _, _ = pileup_files()
    got = bam.confusion_from_bam(ctx, path, fa, pile_ranges())
    return {"matrices": [np.asarray(m, np.int64) for m in got[:4]], "tallies": {k: int(got[4][k]) for k in cms_model.TALLY_NAMES}}


def _run_purity(t, ctx, tmp):
    ctx.set("purity_window", 64)
    ctx.set("cms_batch_reads", 3)
    hb, hi, tallies, rows, scores = purity.purity_from_bam(ctx, pileup_files()[0], pile_ranges(), per_position=True)
    assert tallies["windows"] > 1, tallies
    return {"rows": rows, "base_hist": hb, "ins_hist": hi, "scores": scores, "tallies": {k: int(tallies[k]) for k in purity_model.TALLY_NAMES}}


_serial = [0]


def _out(tmp, name):
    """a fresh output path under tmp: no run appends to another's file"""
    _serial[0] += 1
    return os.path.join(str(tmp), f"{name}_{_serial[0]}")


def _file_kw(t):
    return dict(r=30, indel_start=t.indel_start, indel_extend=t.indel_extend)


def _run_file_sam(t, ctx, tmp):
    ctx.set("device_glue", 1)
    ctx.set("device_pack", 1)
    bp, fa, references, _, _ = read_files(12)
    regions = whole(references)
    out = _out(tmp, "file") + ".sam"
    with _Args(t, regions):
        nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
        try:
            st = nb.realign_file(ctx, nf, nb.select(regions), out, batch_reads=5, **_file_kw(t))
        finally:
            nb.close(); nf.close()
    return {"status": np.asarray(st, np.int32), "text": open(out, "rb").read()}


def _read_bam(out):
    """the records that the members of a written BAM inflate to (framing, CRC-32 and ISIZE asserted), how many members hold
    them, the walk of its index; the file and the index themselves for the comparison between occurrences"""
    mem = members(out)
    data = b"".join(m[1] for m in mem)
    check_index(out, out + ".bai")
    return {"records": data[header_len(data):], "members": len(mem), "file": open(out, "rb").read(), "bai": open(out + ".bai", "rb").read()}


def _run_file_bam_tags(t, ctx, tmp):
    for k, v in (("device_glue", 1), ("device_pack", 1), ("tb_budget_mb", 2)):
        ctx.set(k, v)
    bp, fa, references, _, _ = read_files(40)
    regions = whole(references)
    out = _out(tmp, "tags") + ".bam"
    with _Args(t, regions):
        nb, nf = bam.NativeBam(bp), bam.NativeFasta(fa)
        try:
            bam.create_bam_header(out, Hdr(nb.references, nb.lengths))
            st = nb.realign_file(ctx, nf, nb.select(regions), out, batch_reads=12, out_format="bam", bai=out + ".bai", records="full",
                                 md=True, cs="long", de=True, compress="match", **_file_kw(t))
        finally:
            nb.close(); nf.close()
    got = _read_bam(out)
    assert got["members"] >= 4, got["members"]                   # the header's, more than one of records, the EOF member
    return dict(got, status=np.asarray(st, np.int32))


def _run_onepass(t, ctx, tmp):
    for k, v in (("device_glue", 1), ("device_pack", 1), ("device_inflate", 1)):
        ctx.set(k, v)
    bp, fa, references, _, _ = read_files(12)
    regions = whole(references)
    out = _out(tmp, "onepass") + ".bam"
    with _Args(t, regions):
        one, nf = bam.NativeBam(bp, one_pass=True), bam.NativeFasta(fa)
        try:
            bam.create_bam_header(out, Hdr(one.references, one.lengths))
            n, bad, _ = one.realign_sequential(ctx, nf, regions, out, batch_reads=5, out_format="bam", bai=out + ".bai", compress="huffman",
                                               **_file_kw(t))
            info = one.inflate_info()
        finally:
            one.close(); nf.close()
    assert info[7] == 1 and info[0] > 0, info                    # the blocks were inflated on the device
    return dict(_read_bam(out), selected=int(n), bad=[(int(k), int(s)) for k, s in bad])


def _run_err_r512(t, ctx, tmp):
    refs, seqs, cigs = align_reads("align30")
    try:
        ctx.align_batch(refs, seqs, cigs, t.indel_start, t.indel_extend, r=512)
    except aln.NporeError as e:
        return {"error": "NporeError", "unsupported": "r > 511" in str(e)}
    return {"error": None, "unsupported": False}


def _run_err_late(t, ctx, tmp):
    ctx.set("device_glue", 1)
    ctx.set("device_pack", 1)
    mp, fa, header = late_files()
    out = _out(tmp, "late") + ".sam"
    err = None
    with _Args(t, whole(header)):
        nb, nf = bam.NativeBam(mp), bam.NativeFasta(fa)
        try:
            idx = nb.select(whole(header))
            assert len(idx) == 13
            nb.realign_file(ctx, nf, idx, out, batch_reads=LATE_BATCH, **_file_kw(t))
        except RuntimeError as e:
            err = str(e)
        finally:
            nb.close(); nf.close()
    return {"error": err is not None and "not in the FASTA" in err, "text": open(out, "rb").read() if os.path.exists(out) else b""}


def late_same(got, want):
    """the call failed for the missing contig, and the text holds whole batches in front of the decoy's and nothing else (how
    many of them: the pipeline's overlap decides)"""
    return None if got["error"] is True and got["text"] in want["prefixes"] else "error" if got["error"] is not True else "text"


# ---- the table ------------------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, t, run, want, same=exact, steady=lambda got: got):
        self.name, self.t, self._run, self._want, self.same, self.steady = name, t, run, want, same, steady

    def run(self, ctx, tmp):
        return self._run(self.t, ctx, tmp)

    @functools.cached_property
    def want(self):
        return self._want(self.t)


NAMES = ("align30", "align100_groups", "align260", "align_final", "np_info", "np_regions", "confusion", "purity64", "file_sam",
         "file_bam_tags", "onepass_huffman", "err_r512", "err_contig_late")


@functools.lru_cache(maxsize=None)
def ops(t=None):
    """{name: Op} under the tables `t` (default: the shipped ones)"""
    t = t or shipped()
    al = lambda which, **kw: (lambda t_, ctx, tmp: _align(t_, which, ctx, **kw))
    table = [
        Op("align30", t, al("align30"), lambda t_: want_align(t_, "align30")),
        Op("align100_groups", t, al("align100_groups", settings=(("tb_budget_mb", 8),), min_launches=4), lambda t_: want_align(t_, "align100_groups")),
        Op("align260", t, al("align260"), lambda t_: want_align(t_, "align260")),
        Op("align_final", t, al("align_final", settings=(("device_glue", 1),), final=True), want_align_final),
        Op("np_info", t, _run_np_info, want_np_info),
        Op("np_regions", t, _run_np_regions, want_np_regions),
        Op("confusion", t, _run_confusion, want_confusion),
        Op("purity64", t, _run_purity, want_purity, purity_same),
        Op("file_sam", t, _run_file_sam, want_file_sam),
        Op("file_bam_tags", t, _run_file_bam_tags, want_file_bam_tags),
        Op("onepass_huffman", t, _run_onepass, want_onepass),
        Op("err_r512", t, _run_err_r512, lambda t_: {"error": "NporeError", "unsupported": True}),
        Op("err_contig_late", t, _run_err_late, want_late, late_same, lambda got: {"error": got["error"]}),
    ]
    assert tuple(o.name for o in table) == NAMES
    return {o.name: o for o in table}


def walk_on(ctx, tmp, names, offset=0, first=None, table=None, before=None):
    """run_walk of the operations `names` on one context"""
    table = table or ops()
    return run_walk(list(names), lambda name: table[name].run(ctx, tmp), lambda name: table[name].want, lambda name: table[name].same,
                    offset=offset, first=first, steady_of=lambda name: table[name].steady, before=before)
