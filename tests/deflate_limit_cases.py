"""Payloads at the limits of the device DEFLATE coder (csrc/bam_deflate_kernels.hpp plan_match_kernel / emit_match_kernel):
tokens wider than a word, emitting rounds of more than 64 words, token histograms whose optimal code is deeper than 15.
test_deflate_limits.py runs them through the Python statement and the host twin, test_gpu_deflate_limits.py through the
kernels.  No tests here.  Only numpy and the Python statement of npore_amd/bam.py: what a payload must reach is asserted
in test_deflate_limits.py from bam.match_tokens / bam.huffman_lengths / bam.deflate_member alone.

How a payload is made (Builder): the token list is written first and the bytes follow from it, so that the greedy parse
of the rule gives back exactly that list (payload() asserts it).
  * region(n): random bytes, each rejected while its new 4-gram falls into an occupied hash bucket: n literals, and n
    places a later copy can take as its source without a nearer 4-gram of equal hash in the way;
  * copy(length, lo, hi): the next `length` bytes copy those `d` back, lo <= d <= hi, from a source whose first 4-gram is the
    most recent one of its bucket (the three 4-grams that straddle the chunk's start included) and whose first byte differs
    from the byte behind the previous chunk's source: the previous match ends at the chunk's end, this one starts at once;
  * literals(n): random bytes, each rejected while the 4-gram it completes equals the one at its bucket's candidate.

The payloads, P = 65 280 bytes each (what they reach: props(); these are the figures of the seeds in use):

  name       widest token  heaviest round  ll depth  dist depth  match member  Huffman member  tokens  matches
  wide            35 bits       2192 bits        11           6         34628   65311 stored   30246     3555
  widest          48 bits        994 bits        18          16         48432           60790   44057     4180
  deep_ll         24 bits        829 bits        19           4         34126           36531   53181     2582
  deep_dist       32 bits        852 bits        10          16         55917           63513   52740     4180
  (depth: that of the unlimited optimal code of the token histogram, max(bam.huffman_lengths(freq, 300)); a round: 64 tokens)

  wide       26 624 distinct-hash bytes over 256 values (a multiple of 64: the run begins with an emitting round), then 128
             copies of 131 .. 257 bytes (length symbols 281 .. 284, 32 each) from the upper half of the distance symbols 28 and
             29 (so that the last of the 13 extra bits is set), then 3 427 length-4 copies over the distance symbols 10 .. 27,
             then literals.  All 128 are 34 or 35 bits wide; 5 of them have bits in a third word wherever the member begins.
             It stops at 35: 32 of 30 246 tokens are a code of 10 or 11 bits, 64 of 3 555 distances one of 6, and a run of
             128 such copies with its sources takes 50 000 of the 65 280 bytes.
  widest     both Fibonacci ladders in one block: length symbols 284, 283, 282, 281, 269 .. 258 with 1, 2, 3, 5, 8 .. 1 598
             copies, distance symbols 29 .. 13 with 1, 1, 2, 3 .. 1 597; the long copies take the far distances, the rarest
             of each meet in one token: 15 + 5 + 15 + 13 = 48 bits, the most the format allows.
  deep_ll    8 000 distinct-hash bytes over 24 letters, then 2 582 copies whose length symbols 272 .. 258 carry 1, 2, 3, 5 ..
             987 (end-of-block is the other 1; the rarest symbol the longest length) at short distances, then literals.
  deep_dist  25 024 distinct-hash bytes over 256 values, then 4 180 length-4 copies whose distance symbols 29 .. 13 carry
             1, 1, 2, 3 .. 1 597, then literals.
  A chain needs the counts 1, 1, 2, 3, 5 ..: with a third count of 1 (1, 1, 1, 2, 3 ..) two chains grow side by side and the
  depth is half.  In the literal / length alphabet end-of-block is one of the two.
"""
import functools

import numpy as np

from npore_amd import bam

P = bam.BGZF_STORED_PAYLOAD
NAMES = ("wide", "widest", "deep_ll", "deep_dist")
FIB = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987)       # a code of these counts is a chain: 16 leaves, depth 15
FIB17 = FIB + (1597,)                                                        # ... and depth 16; a third count of 1 would halve it


def _bucket(a, b, c, d):
    return (((a | b << 8 | c << 16 | d << 24) * 2654435761) & 0xFFFFFFFF) >> (32 - bam.MATCH_HASH_BITS)


class Builder:
    """Bytes that the greedy parse of bam.match_tokens cuts into the tokens asked for."""

    def __init__(self, seed, values):
        self.rng = np.random.default_rng(seed)
        self.values = [int(v) for v in values]
        self.out = bytearray()
        self.last = [-1] * (1 << bam.MATCH_HASH_BITS)          # bucket -> most recent position, for the positions < entered
        self.entered = 0
        self.tokens = []
        self.avoid = -1                                        # the byte that would lengthen the previous match
        self.lit_from = 0                                      # the literals behind the last copy begin here

    def _enter(self):
        o = self.out
        while self.entered + 4 <= len(o):
            i = self.entered
            self.last[_bucket(o[i], o[i + 1], o[i + 2], o[i + 3])] = i
            self.entered += 1

    def _byte_ok(self, b, distinct):
        """may b be the next byte: the 4-gram it completes (at q) leaves position q a literal"""
        o = self.out
        if len(o) == self.lit_from and b == self.avoid:
            return False
        q = len(o) - 3
        if q < 0:
            return True
        c = self.last[_bucket(o[q], o[q + 1], o[q + 2], b)]
        if distinct:
            return c < 0
        return q < self.lit_from or c < 0 or bytes(o[c:c + 4]) != bytes(o[q:q + 3]) + bytes([b])

    def _literals(self, n, distinct):
        for _ in range(n):
            for b in self.rng.permutation(self.values).tolist():
                if self._byte_ok(b, distinct):
                    break
            else:
                raise AssertionError("no byte value is left at %d" % len(self.out))
            self.out.append(b)
            self.tokens.append(b)
            self._enter()

    def region(self, n):
        self._literals(n, True)

    def literals(self, n):
        self._literals(n, False)

    def copy(self, length, lo, hi, tries=4000):
        o, p = self.out, len(self.out)
        lo, hi = max(lo, length), min(hi, p)
        assert bam.MATCH_MIN <= length <= bam.MATCH_MAX and lo <= hi, (length, lo, hi, p)
        for _ in range(tries):
            d = int(self.rng.integers(lo, hi + 1))
            s = p - d
            if o[s] == self.avoid:
                continue
            hs = _bucket(o[s], o[s + 1], o[s + 2], o[s + 3])
            if self.last[hs] != s:
                continue
            new = bytes(o[max(0, p - 3):p]) + bytes(o[s:s + 3])
            ok = True
            for j in range(len(new) - 6, len(new) - 3):            # the 4-grams at p - 3, p - 2, p - 1
                if j < 0:
                    continue
                q = p - (len(new) - 3) + j
                h = _bucket(new[j], new[j + 1], new[j + 2], new[j + 3])
                c = self.last[h]
                if h == hs or (q >= self.lit_from and c >= 0 and bytes(o[c:c + 4]) == new[j:j + 4]):
                    ok = False
            if not ok:
                continue
            o += o[s:s + length]
            self.avoid = o[s + length] if length < bam.MATCH_MAX else -1
            self.tokens.append((length, d))
            self.lit_from = len(o)
            self._enter()
            return
        raise AssertionError("no source for a copy of %d bytes %d .. %d back at %d" % (length, lo, hi, p))

    def payload(self):
        data = bytes(self.out)
        assert len(data) == P and bam.match_tokens(data) == self.tokens
        return data


def _dist_range(sym):
    lo = bam._DIST_BASE[sym]
    return lo, lo + (1 << bam._DIST_EXTRA[sym]) - 1


def _len_range(sym):
    lo = bam._LEN_BASE[sym - 257]
    return lo, 258 if sym == 285 else min(257, lo + (1 << bam._LEN_EXTRA[sym - 257]) - 1)


def _copy_of(b, len_sym, dist_sym):
    lo, hi = _len_range(len_sym)
    b.copy(int(b.rng.integers(lo, hi + 1)), *_dist_range(dist_sym))


def _ladder(symbols, counts, rng):
    """the symbols, each as often as its count, shuffled"""
    return rng.permutation(np.repeat(np.asarray(symbols), counts)).tolist()


def _build_wide():
    b = Builder(101, range(256))
    b.region(26624)                                                # a multiple of 64: the run begins with an emitting round
    for k in range(128):                                           # two emitting rounds of nothing else
        lo, hi = _len_range(281 + k % 4)
        dlo, dhi = _dist_range(28 + (k // 4) % 2 if k >= 16 else 28)       # (the upper half of 29 lies 28 673 back and more)
        b.copy(int(b.rng.integers(lo, hi + 1)), (dlo + dhi + 1) // 2, dhi)     # the upper half: the token's last bit is set
    k = 0
    while len(b.out) + 4 <= P - 64:
        _copy_of(b, 258, 10 + k % 18)
        k += 1
    b.literals(P - len(b.out))
    return b.payload()


def _build_deep_ll():
    b = Builder(102, b"ACGTNacgtn0123456789=*!#")
    b.region(8000)
    for sym in _ladder(range(258, 273), FIB[:0:-1], b.rng):        # end-of-block once, 272 once, 271 twice ... 258: 987 times
        lo, hi = _len_range(sym)
        length = int(b.rng.integers(lo, hi + 1))
        for reach in (64, 256, 1024, 8192):                        # near where there is a source: few extra bits of the distance
            try:
                b.copy(length, 5, max(reach, 2 * length), tries=200)
                break
            except AssertionError:
                if reach == 8192:
                    raise
    b.literals(P - len(b.out))
    return b.payload()


def _build_deep_dist():
    b = Builder(103, range(256))
    b.region(25024)
    for sym in _ladder(range(13, 30), FIB17[::-1], b.rng):         # 13: 1 597 times ... 27: twice, 28 and 29 once
        _copy_of(b, 258, sym)
    b.literals(P - len(b.out))
    return b.payload()


def _build_widest():
    b = Builder(104, range(256))
    b.region(25024)
    # lengths: end-of-block once, 284 once, 283 twice, 282: 3, 281: 5, 269: 8 ... 259: 987, 258: 1 597 + 1
    # distances: 29 and 28 once, 27 twice, 26: 3 ... 13: 1 597
    lens = _ladder(list(range(258, 270)) + [281, 282, 283, 284], (FIB17[-1] + 1,) + FIB17[-2:4:-1] + (5, 3, 2, 1), b.rng)
    dists = _ladder(range(13, 30), FIB17[::-1], b.rng)
    assert len(lens) == len(dists)
    # a long copy takes a far source, in the region (a near one would hide every source behind it); the rarest of each meet
    long_lens = sorted(s for s in lens if s > 280)
    far = sorted(dists)[-len(long_lens):]
    lens = [s for s in lens if s <= 280]
    for s in far:
        dists.remove(s)
    for ls, ds in list(zip(lens, dists)) + list(zip(long_lens, far)):
        _copy_of(b, ls, ds)
    b.literals(P - len(b.out))
    return b.payload()


_BUILD = {"wide": _build_wide, "widest": _build_widest, "deep_ll": _build_deep_ll, "deep_dist": _build_deep_dist}


@functools.lru_cache(8)
def token_fields(data):
    """(header bits as an integer, how many, [(value, bits)] per token with end-of-block last, code lengths of both alphabets)
    of the payload's match block, from the Python statement"""
    tokens = bam.match_tokens(data)
    ll_freq, d_freq = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            ll_freq[bam._len_symbol(t[0])[0]] += 1
            d_freq[bam._dist_symbol(t[1])[0]] += 1
        else:
            ll_freq[t] += 1
    ll_freq[256] = 1
    ll_lens, d_lens = bam.huffman_lengths(ll_freq, 15), bam.huffman_lengths(d_freq, 15)
    ll_codes, d_codes = bam.canonical_codes(ll_lens), bam.canonical_codes(d_lens)
    hlit = max([257] + [s + 1 for s in range(286) if ll_freq[s]])
    hdist = max([1] + [s + 1 for s in range(30) if d_freq[s]])
    acc, header_bits = bam._code_length_header(ll_lens[:hlit], d_lens[:hdist])
    fields = []
    for t in tokens + [256]:
        if isinstance(t, tuple):
            ls, le, lv = bam._len_symbol(t[0])
            ds, de, dv = bam._dist_symbol(t[1])
            v, nb = 0, 0
            for val, w in ((ll_codes[ls][1], ll_codes[ls][0]), (lv, le), (d_codes[ds][1], d_codes[ds][0]), (dv, de)):
                v |= val << nb
                nb += w
            fields.append((v, nb))
        else:
            fields.append((ll_codes[t][1], ll_codes[t][0]))
    return acc, header_bits, fields, ll_lens, d_lens, (ll_freq, d_freq)


def props(data):
    """What the Python statement makes of the payload: token widths, round bits, depths, sizes."""
    tokens = bam.match_tokens(data)
    _, header_bits, fields, ll_lens, d_lens, (ll_freq, d_freq) = token_fields(data)
    assert (header_bits, sum(nb for _, nb in fields)) == bam.deflate_match_block(data, tokens)[1:]
    nb = np.asarray([w for _, w in fields])                        # (end-of-block is token n_tokens of the emitting rounds)
    at = header_bits + np.concatenate([[0], np.cumsum(nb)[:-1]])
    # the third word's bits, were the block's first byte at an address = a modulo 4: the kernel's words are the memory's
    third_set = [sum(1 for (v, w), p in zip(fields, at.tolist()) if w >= 34 and v >> (64 - (8 * a + p) % 32)) for a in range(4)]
    run = best = 0
    for t in tokens:
        run = run + 1 if isinstance(t, tuple) and 131 <= t[0] <= 257 and 16385 <= t[1] <= 32768 else 0
        best = max(best, run)
    match_member, huffman_member = bam.deflate_member(data, matches=True), bam.deflate_member(data)
    return {
        "tokens": len(tokens), "matches": int(sum(d_freq)),
        "widest_token": int(nb.max()), "tokens_34_or_wider": int((nb >= 34).sum()),
        "third_word_tokens": int(((nb >= 34) & (at % 32 + nb > 64)).sum()), "third_word_set": third_set,
        "longest_wide_run": best, "heaviest_round": max(int(nb[k:k + 64].sum()) for k in range(0, len(nb), 64)),
        "ll_depth": max(bam.huffman_lengths(ll_freq, 300)), "dist_depth": max(bam.huffman_lengths(d_freq, 300)),
        "ll_longest_code": max(ll_lens), "dist_longest_code": max(d_lens),
        "ll_symbols": sum(1 for f in ll_freq if f), "dist_symbols": sum(1 for f in d_freq if f),
        "header_bits": header_bits, "written": match_member != huffman_member,
        "match_member": len(match_member), "huffman_member": len(huffman_member),
    }


@functools.lru_cache(None)
def case(name):
    """(payload, what it reaches): built once per process"""
    data = _BUILD[name]()
    return data, props(data)


def payload(name):
    return case(name)[0]


@functools.lru_cache(None)
def inflate_launch(guard):
    """The payloads' match blocks and Huffman blocks (the Python statement's) as one launch of inflate_device_cases, for the
    decoders: streams that inflate to 65 280 bytes, within the 65 536 a member may hold."""
    import inflate_device_cases as idc
    cases = []
    for name in NAMES:
        data = payload(name)
        assert len(data) <= idc.IW_MAX_OUT
        for what, member in (("match", bam.deflate_member(data, matches=True)), ("huffman", bam.deflate_member(data))):
            cases.append(("%s, %s block" % (name, what), member[18:-8], len(data), data))
    return idc.Launch("limit members " + ("guard" if guard else "tight"), cases, guard)


if __name__ == "__main__":
    for name in NAMES:
        print(name, case(name)[1])
