"""The one way the tests reach the FULL-record entries: the host ladder npore_bam_format_bam_full{,_md,_tags,_pass} (host_full)
and its device twins npore_debug_format_bam_full{,_md,_tags,_pass}_device (device_full).  `entry` names the rung, the widest by
default; a rung gets exactly the arguments it has, and an option it cannot say is an error here, not a silent zero.
"""
import ctypes as C

import numpy as np

from npore_amd import bam

ENTRIES = ("", "_md", "_tags", "_pass")


def rung_words(entry, flags, tags, mask):
    """(flags, tags, mask) cut to what the rung `entry` takes"""
    words = (flags, tags, mask)[:ENTRIES.index(entry)]
    if any((flags, tags, mask)[len(words):]):
        raise ValueError(f"npore_bam_format_bam_full{entry} cannot say flags {flags}, tags {tags}, mask {mask}")
    return words


def host_full(nb, nf, idx, finals, status, *, entry="_pass", flags=0, tags=0, mask=0):
    """(return code, record bytes) of npore_bam_format_bam_full<entry> with the raw words flags / tags / mask"""
    _keep, reads = bam.marshal_finals(idx, finals, status)
    fmap = nb.fasta_map(nf)
    recs, n = C.c_void_p(), C.c_int64()
    rc = getattr(nb._lib, "npore_bam_format_bam_full" + entry)(nb.handle, nf.handle, fmap.ctypes.data, *reads, 0, C.byref(recs), C.byref(n),
                                                               *rung_words(entry, flags, tags, mask))
    return rc, C.string_at(recs.value, n.value) if rc == 0 and n.value else b""


def device_full(ctx, nb, nf, idx, finals, status, *, cap=None, entry="_pass", mask=0, **options):
    """(record bytes, nm[n], md_len[n]) of npore_debug_format_bam_full<entry>_device; options: md, cs, de, eqx, oc as
    NativeBam.format_bam_full takes them.  nm and md_len start at -1 (md_len stays there where the rung or the options have no MD).
    cap: the room for the records, by default the host twin's length for the same options plus 4096."""
    if cap is None:
        cap = len(nb.format_bam_full(nf, idx, finals, status, pass_mask=mask, **options)) + 4096
    flags = bam.OUT_MD if options.get("md") else 0
    tags = bam.output_tags(*(options.get(k) for k in ("cs", "de", "eqx", "oc")))
    _keep, reads = bam.marshal_finals(idx, finals, status)
    n = reads[1]
    fmap = nb.fasta_map(nf)
    recs, nm, md_len, got = np.zeros(cap, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32), C.c_int64()
    words = list(rung_words(entry, flags, tags, mask))
    words[1:1] = [md_len.ctypes.data] if words else []            # (md_len stands behind the flags)
    nb._check(getattr(nb._lib, f"npore_debug_format_bam_full{entry}_device")(ctx.handle, nb.handle, nf.handle, fmap.ctypes.data, *reads, recs.ctypes.data,
                                                                              cap, C.byref(got), nm.ctypes.data, *words))
    return recs[:got.value].tobytes(), nm, md_len
