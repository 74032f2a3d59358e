"""bam.OutputSpec, the one statement of a run's output options: its constants against include/npore_amd.h; its four words, its
refusals and NativeBam.set_output's setter calls over the whole product of the options, against the formulas and the order of checks
NativeBam.set_output had before the spec (restated here literally, numbers and all); and OutputSpec.from_args / realign.main on
argparser's own namespaces: the ERROR line of every rule, in realign's order of checks, exit status 1.  No GPU, no library call.
"""
import argparse
import dataclasses
import itertools
import os
import re

import pytest

from npore_amd import bam, cfg, realign
from conftest import REPO

NAMES = ("OUT_EOF", "OUT_PART", "OUT_DEFLATE", "OUT_MATCH", "OUT_FULL", "OUT_MD", "TAG_CS", "TAG_CS_LONG", "TAG_DE", "CIGAR_EQX", "TAG_OC")
FIELDS = ("out_format", "bai", "eof", "compress", "records", "md", "cs", "de", "pass_mask", "eqx", "oc")
DEFAULTS = dict(zip(FIELDS, ("sam", None, True, "none", "reference", False, None, False, 0, False, False)))      # set_output's, before the spec


def test_constants_are_the_headers():
    hdr = open(os.path.join(REPO, "include", "npore_amd.h")).read()
    defined = {name: int(v) for name, v in re.findall(r"^#define NPORE_(\w+) (\d+)\b", hdr, re.M)}
    for name in NAMES:
        assert getattr(bam, name) == defined[name], name
    assert bam.PART_BASE == defined["PART_BASE"] and bam.ST_PASSED == defined["ST_PASSED"]
    assert [f.name for f in dataclasses.fields(bam.OutputSpec)] == list(FIELDS)
    assert bam.OutputSpec() == bam.OutputSpec(*DEFAULTS.values())


# ---- what NativeBam.set_output did before the spec, restated ---------------------------------------------------------------------------
def old_refusal(out_format, bai, eof, compress, records, md, cs, de, pass_mask, eqx, oc):
    """the text of the ValueError, or None"""
    if pass_mask and records != "full":
        return "pass_mask needs records 'full'"
    if compress not in ("none", "huffman", "match"):
        return "compress must be 'none', 'huffman' or 'match'"
    if records not in ("reference", "full"):
        return "records must be 'reference' or 'full'"
    if records == "full" and out_format != "bam":
        return "records 'full' needs out_format 'bam'"
    if md and records != "full":
        return "md needs records 'full'"
    if cs not in (None, "short", "long"):
        return "cs must be None, 'short' or 'long'"
    if old_tags(cs, de, eqx, oc) and records != "full":
        return "cs, de, eqx and oc need records 'full'"
    if compress != "none" and out_format != "bam":
        return "compress needs out_format 'bam'"
    return None


def old_tags(cs, de, eqx, oc):
    return {None: 0, "short": 1, "long": 3}[cs] | (4 if de else 0) | (32 if eqx else 0) | (256 if oc else 0)


def old_flags(out_format, eof, compress, records, md):
    flags = 0 if out_format != "bam" else 1 if eof else 2
    flags |= {"none": 0, "huffman": 4, "match": 12}[compress]
    flags |= 16 if records == "full" else 0
    flags |= 32 if md else 0
    return flags


def old_calls(handle, out_format, bai, eof, compress, records, md, cs, de, pass_mask, eqx, oc):
    calls = [("npore_bam_set_output", (handle, {"sam": 0, "bam": 1}[out_format], os.fsencode(bai) if bai else None,
                                       old_flags(out_format, eof, compress, records, md)))]
    if old_tags(cs, de, eqx, oc):
        calls.append(("npore_bam_set_output_tags", (handle, old_tags(cs, de, eqx, oc))))
    if pass_mask:
        calls.append(("npore_bam_set_output_pass", (handle, int(pass_mask))))
    return calls


class RecordingLib:
    """stands in for the library behind a NativeBam: every call is noted and succeeds"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


def recording_handle():
    nb = bam.NativeBam.__new__(bam.NativeBam)
    nb._lib, nb.handle = RecordingLib(), 7
    return nb


def test_words_refusals_and_setter_calls_over_the_product():
    nb = recording_handle()
    product = itertools.product(("sam", "bam"), (True, False), ("none", "huffman", "match"), ("reference", "full"), (False, True),
                                (None, "short", "long"), (False, True), (False, True), (False, True), (0, bam.PASS_FLAGS))
    accepted = refused = 0
    for out_format, eof, compress, records, md, cs, de, eqx, oc, pass_mask in product:
        bai = "out.bam.bai" if md == de else None                # (the path goes through as it is; it decides nothing)
        args = (out_format, bai, eof, compress, records, md, cs, de, pass_mask, eqx, oc)
        text = old_refusal(*args)
        if text is not None:
            refused += 1
            with pytest.raises(ValueError) as e:
                bam.OutputSpec(*args)
            assert str(e.value) == text, args
            nb._lib.calls.clear()
            with pytest.raises(ValueError) as e:
                nb.set_output(**dict(zip(FIELDS, args)))
            assert str(e.value) == text and nb._lib.calls == [], args
            continue
        accepted += 1
        spec = bam.OutputSpec(*args)
        assert (spec.format_word, spec.flags, spec.tags, spec.pass_mask) == \
            ({"sam": 0, "bam": 1}[out_format], old_flags(out_format, eof, compress, records, md), old_tags(cs, de, eqx, oc), pass_mask), args
        assert bam.output_tags(cs, de, eqx, oc) == old_tags(cs, de, eqx, oc)
        for call in (lambda: nb.set_output(spec), lambda: nb.set_output(*args), lambda: nb.set_output(**dict(zip(FIELDS, args)))):
            nb._lib.calls.clear()
            call()
            assert nb._lib.calls == old_calls(7, *args), args
    assert accepted + refused == 2304 and accepted == 576 + 6 + 2      # BAM with FULL records, BAM with the reference's (eof x compress), SAM (eof)
    # a value outside a set, beside rules of the same spec that are broken too: the older check's text
    for kw, text in ((dict(compress="gzip"), "compress must be 'none', 'huffman' or 'match'"),
                     (dict(records="whole", md=True), "records must be 'reference' or 'full'"),
                     (dict(records="whole", pass_mask=4), "pass_mask needs records 'full'"),
                     (dict(out_format="bam", records="full", cs="both"), "cs must be None, 'short' or 'long'"),
                     (dict(cs="both"), "cs must be None, 'short' or 'long'"),
                     (dict(cs="both", md=True), "md needs records 'full'")):
        assert old_refusal(**{**DEFAULTS, **kw}) == text
        with pytest.raises(ValueError) as e:
            bam.OutputSpec(**kw)
        assert str(e.value) == text, kw
    with pytest.raises(ValueError) as e:
        bam.output_tags("both", False)
    assert str(e.value) == "cs must be None, 'short' or 'long'"


# ---- the command line -----------------------------------------------------------------------------------------------------------------
BASE = ["--bam", "in.bam", "--ref", "ref.fa", "--out_prefix", "out"]
FULL = ["--out_format", "bam", "--records", "full"]
TAGS_LINE = "{} needs --out_format bam --records full."
# (options, the line realign printed for them before the spec): every rule alone, then several broken at once, in realign's order
CLI_CASES = [
    (["--records", "full"], "--records full needs --out_format bam."),
    (["--records", "full", "--out_format", "sam"], "--records full needs --out_format bam."),
    (["--md"], "--md needs --records full."),
    (["--md", "--out_format", "bam"], "--md needs --records full."),
    (["--cs", "short"], TAGS_LINE.format("--cs")),
    (["--cs", "long", "--out_format", "bam", "--records", "reference"], TAGS_LINE.format("--cs")),
    (["--de"], TAGS_LINE.format("--de")),
    (["--de", "--cs", "long", "--out_format", "bam"], TAGS_LINE.format("--cs")),
    (["--eqx"], TAGS_LINE.format("--eqx")),
    (["--eqx", "--out_format", "bam"], TAGS_LINE.format("--eqx")),
    (["--oc"], TAGS_LINE.format("--oc")),
    (["--oc", "--out_format", "bam"], TAGS_LINE.format("--oc")),
    (["--pass_through"], TAGS_LINE.format("--pass_through")),
    (["--pass_through", "--out_format", "bam"], TAGS_LINE.format("--pass_through")),
    (["--bam_compress", "huffman"], "--bam_compress needs --out_format bam."),
    (["--bam_compress", "match", "--out_format", "sam"], "--bam_compress needs --out_format bam."),
    (["--records", "full", "--md", "--bam_compress", "match"], "--records full needs --out_format bam."),
    (["--pass_through", "--oc", "--eqx", "--de", "--cs", "short", "--md", "--bam_compress", "match"], "--md needs --records full."),
    (["--pass_through", "--oc", "--eqx", "--de", "--bam_compress", "match"], TAGS_LINE.format("--de")),
    (["--pass_through", "--oc", "--eqx", "--out_format", "bam"], TAGS_LINE.format("--eqx")),
    (["--pass_through", "--oc", "--bam_compress", "match"], TAGS_LINE.format("--oc")),
    (["--pass_through", "--bam_compress", "match"], TAGS_LINE.format("--pass_through")),
]


@pytest.mark.parametrize("options,line", CLI_CASES, ids=[" ".join(o) for o, _ in CLI_CASES])
def test_cli_rules(options, line, capsys, monkeypatch):
    args = realign.argparser().parse_args(BASE + options)
    with pytest.raises(bam.OutputSpecError) as e:
        bam.OutputSpec.from_args(args)
    assert e.value.cli == line and isinstance(e.value, ValueError)
    # ... and realign.main prints it, alone, and exits 1 -- with files that do not exist: nothing was opened, no GPU touched
    monkeypatch.setattr(cfg, "args", args)
    with pytest.raises(SystemExit) as stop:
        realign.main()
    assert stop.value.code == 1
    assert capsys.readouterr().out == f"\nERROR: {line}\n"
    assert not os.path.exists("out.sam") and not os.path.exists("out.bam")


def test_from_args():
    parse = lambda *more: realign.argparser().parse_args(BASE + list(more))
    assert bam.OutputSpec.from_args(parse()) == bam.OutputSpec()
    assert bam.OutputSpec.from_args(parse("--out_format", "bam"), bai="out.bam.bai", eof=False) == bam.OutputSpec("bam", "out.bam.bai", False)
    everything = parse(*FULL, "--bam_compress", "match", "--md", "--cs", "long", "--de", "--eqx", "--oc", "--pass_through")
    assert bam.OutputSpec.from_args(everything, bai="x.bai") == \
        bam.OutputSpec("bam", "x.bai", True, "match", "full", True, "long", True, bam.PASS_FLAGS, True, True)
    assert bam.OutputSpec.from_args(parse(*FULL, "--cs", "short", "--bam_compress", "huffman"), eof=False) == \
        bam.OutputSpec("bam", eof=False, compress="huffman", records="full", cs="short")
    # a namespace that lacks an option has it off (callers that build their own, as the tests do)
    assert bam.OutputSpec.from_args(argparse.Namespace()) == bam.OutputSpec()
    assert bam.OutputSpec.from_args(argparse.Namespace(out_format="bam", md=1, records="full")) == bam.OutputSpec("bam", records="full", md=True)
    with pytest.raises(ValueError):                              # an override is held to the rules like any field
        bam.OutputSpec.from_args(parse(), records="full")
