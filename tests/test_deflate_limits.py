"""The DEFLATE coder of --bam_compress match at its limits, the host side: the payloads of deflate_limit_cases.py -- tokens
of up to 48 bits, emitting rounds of more than 2 048 bits, token histograms whose optimal code is deeper than 15 bits --
reach what they are built for (asserted from the Python statement alone), and on each of them the host twin
(npore_debug_deflate_member_mode) writes the Python statement's member, which zlib, this tree's decoder and the
device-inflate host twin take back.  No GPU.

What the payloads must reach are conditions on the kernel's code paths (csrc/bam_deflate_kernels.hpp emit_match_kernel), not
measurements:
  * a token of nb bits that starts at bit sh of a 32-bit word reaches a third word iff sh + nb > 64, so nb >= 34; the words
    are the memory's, so sh follows from the token's place in the block AND the address of the block's first byte modulo 4,
    and the kernel's third atomicOr runs only if one of the bits behind bit 64 is set (the top extra bits of the distance):
    props()["third_word_set"] counts such tokens for each of the four addresses;
  * a round of 64 tokens stores nw = (carry bits + its bits) >> 5 words, a word per lane per pass: more than 2 080 bits are
    more than 64 words whatever the carry (at most 31 bits), and the store loop needs its second pass;
  * the Kraft repair acts iff the unlimited optimal code is deeper than 15.
emit_model() restates the kernel's staging of a round in Python: as the kernel has it, it gives the block's bytes; with
the third word dropped, the staging buffer cut to the words of 2 048 bits, or the store loop's second pass left out, it
does not -- on `wide`, and on none of the contents the suite had before (test_old_contents_do_not_reach_the_limits).
"""
import struct
import zlib

import pytest

from npore_amd import bam
import deflate_limit_cases as dlc
import inflate_device_cases as idc
from test_bam_deflate import host_member, inflate
from test_bam_match import ALL, any_content, host_member_mode, replay

P = dlc.P


def emit_model(data, align=2, third_word=True, stage=100, passes=2):
    """The block as emit_match_kernel stages it, its first byte at an address = align modulo 4 (a member at a multiple of 4:
    2): the header's bytes in front of the last word boundary, then rounds of 64 tokens OR-ed into `stage` 32-bit words (a
    token into up to three of them), nw whole words stored per round in `passes` passes of 64 lanes, the carry word handed on."""
    acc, header_bits, fields, *_ = dlc.token_fields(data)
    hb = header_bits >> 3
    lead = hb - (align + hb) % 4
    out = bytearray(acc.to_bytes((header_bits + 7) // 8, "little")[:lead])
    carry, cbits = acc >> (8 * lead), header_bits - 8 * lead
    for t0 in range(0, len(fields), 64):
        s = [0] * stage
        s[0] = carry
        pos = cbits
        for v, nb in fields[t0:t0 + 64]:
            if nb:
                w, sh = pos >> 5, pos & 31
                rest = v >> (32 - sh)
                parts = [(w, (v << sh) & 0xFFFFFFFF), (w + 1, rest & 0xFFFFFFFF)] + ([(w + 2, rest >> 32)] if third_word else [])
                for j, x in parts:
                    if x and j < stage:                             # (the model drops what the kernel would write out of bounds)
                        s[j] |= x
            pos += nb
        nw = pos >> 5
        words = [s[j] if j < min(stage, 64 * passes) else 0 for j in range(nw)]
        out += struct.pack("<%dI" % nw, *words)
        carry, cbits = s[nw] if nw < stage else 0, pos & 31
    out += carry.to_bytes(4, "little")[:(cbits + 7) >> 3]
    return bytes(out)


# ---- 1. what each payload is built for: conditions, from the Python statement alone ------------------------------------------
@pytest.mark.parametrize("name", dlc.NAMES)
def test_payload_is_a_member_and_written(name):
    data, pr = dlc.case(name)
    print(name, pr)
    assert len(data) == P
    assert pr["written"] and bam.deflate_member(data, matches=True) != bam.deflate_member(data)
    assert pr["match_member"] < pr["huffman_member"] <= P + 31
    assert pr["widest_token"] <= 48 and pr["heaviest_round"] <= 64 * 48


def test_wide_conditions():
    data, pr = dlc.case("wide")
    print(pr)
    assert pr["longest_wide_run"] >= 128                               # 131 .. 257 bytes from 16 385 .. 32 768 back, one after the other
    assert pr["tokens_34_or_wider"] >= 64                               # (b)
    assert pr["third_word_tokens"] >= 1                                 # (c)
    assert min(pr["third_word_set"]) >= 1                               # ... with bits set there, wherever the member begins
    assert pr["heaviest_round"] > 2080                                  # (d): nw > 64 whatever the carry
    # (c) and (d) once more, from the fields themselves
    _, header_bits, fields, *_ = dlc.token_fields(data)
    at, third = header_bits, 0
    for _, nb in fields:
        third += nb >= 34 and at % 32 + nb > 64
        at += nb
    assert third == pr["third_word_tokens"]
    assert max(sum(nb for _, nb in fields[k:k + 64]) for k in range(0, len(fields), 64)) == pr["heaviest_round"]


def test_widest_conditions():
    pr, wide = dlc.case("widest")[1], dlc.case("wide")[1]
    print(pr)
    assert pr["widest_token"] > wide["widest_token"] and pr["widest_token"] >= 40


@pytest.mark.parametrize("name,key,longest", [("deep_ll", "ll_depth", "ll_longest_code"), ("deep_dist", "dist_depth", "dist_longest_code"),
                                              ("widest", "ll_depth", "ll_longest_code"), ("widest", "dist_depth", "dist_longest_code")])
def test_deep_conditions(name, key, longest):
    """The unlimited optimal code of the token histogram is deeper than 15, so the limited one reaches 15: the repair acts."""
    pr = dlc.case(name)[1]
    print(name, pr)
    assert pr[key] > 15 and pr[longest] == 15


@pytest.mark.parametrize("name", dlc.NAMES)
def test_codes_are_complete_and_limited(name):
    data = dlc.payload(name)
    _, header_bits, _, ll_lens, d_lens, (ll_freq, d_freq) = dlc.token_fields(data)
    for lens, freq in ((ll_lens, ll_freq), (d_lens, d_freq)):
        assert all((l > 0) == (f > 0) for l, f in zip(lens, freq)) and max(lens) <= 15
        assert sum(1 for l in lens if l) >= 2
        assert sum(1 << (15 - l) for l in lens if l) == 1 << 15       # the Kraft sum is exactly 1
        unlimited = bam.huffman_lengths(freq, 300)
        cost, best = sum(f * l for f, l in zip(freq, lens)), sum(f * l for f, l in zip(freq, unlimited))
        assert cost >= best and (cost == best) == (max(unlimited) <= 15)
    assert header_bits <= 17 + 19 * 3 + 316 * 7


# ---- 2. the statements agree, the members decode ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dlc.NAMES)
def test_member(name):
    data, pr = dlc.case(name)
    m = host_member_mode(data, 2)
    assert m == bam.deflate_member(data, matches=True)
    h = host_member(data)
    assert h == host_member_mode(data, 1) == bam.deflate_member(data)
    assert (len(m), len(h)) == (pr["match_member"], pr["huffman_member"])
    assert m[:4] == b"\x1f\x8b\x08\x04" and m[10:16] == b"\x06\x00BC\x02\x00"
    assert struct.unpack_from("<H", m, 16)[0] + 1 == len(m)
    assert struct.unpack("<II", m[-8:]) == (zlib.crc32(data), P)
    block = m[18:-8]
    assert zlib.decompress(block, -15) == data
    assert inflate(block, P, 1) == (1, data)                            # this tree's decoder, without a fallback to zlib
    assert len(m) <= len(h) <= P + 31
    tokens = bam.match_tokens(data)
    assert replay(tokens) == data
    py_block, header_bits, data_bits = bam.deflate_match_block(data, tokens)
    assert block == py_block and len(block) == (header_bits + data_bits + 7) // 8
    assert block[0] & 7 == 0b101 and len(block) < P + 5
    assert header_bits == pr["header_bits"] <= 17 + 19 * 3 + 316 * 7


@pytest.mark.parametrize("guard", (0, idc.GUARD))
def test_device_inflate_twin_takes_the_members(guard):
    """The decoder of csrc/inflate_wave.hpp (its host twin) takes every limit member's block, the match block and the Huffman
    block: codes of 15 bits in both alphabets, 18 extra bits a token."""
    launch = dlc.inflate_launch(guard)
    status, out = idc.twin(launch)
    assert launch.guards_intact(out)
    for k, (name, raw, n, want) in enumerate(launch.cases):
        assert idc.zlib_inflate(raw, n) == want, name
        assert status[k] == 1 and launch.piece(out, k) == want, name


# ---- 3. the tests can fail: the kernel's staging restated, and three ways to get it wrong -----------------------------------------
@pytest.mark.parametrize("name", dlc.NAMES)
def test_emit_model_is_the_block(name):
    data = dlc.payload(name)
    want = bam.deflate_match_block(data)[0]
    for align in range(4):
        assert emit_model(data, align) == want, align


def test_wide_tells_a_wrong_staging():
    """Without the third word, with a staging buffer of the 65 words that 2 048 + 31 bits need, or with one pass of the store
    loop, the model writes other bytes for `wide`, wherever the member begins; a buffer of the heaviest round's whole words +
    the carry is enough."""
    data, pr = dlc.case("wide")
    want = bam.deflate_match_block(data)[0]
    for align in range(4):
        assert emit_model(data, align, third_word=False) != want, align
        assert emit_model(data, align, stage=65) != want, align
        assert emit_model(data, align, passes=1) != want, align
    assert emit_model(data, stage=(31 + pr["heaviest_round"]) // 32 + 1) == want


def test_old_contents_do_not_reach_the_limits():
    """Why the payloads are needed: on the twelve contents the suite had, the model with all three faults writes the same
    bytes wherever a match block is written."""
    n_written = 0
    for kind, new in ALL:
        data = any_content(kind, new, P)
        if bam.deflate_member(data, matches=True) == bam.deflate_member(data):
            continue
        n_written += 1
        want = bam.deflate_match_block(data)[0]
        for align in range(4):
            assert emit_model(data, align, third_word=False, stage=65, passes=1) == want, (kind, align)
    assert n_written >= 5
