"""The layout of the fill kernel's two LDS score tables (layout.hpp NP_CT / SUBT_ENTRIES): free of bank conflicts by the
bank model of the hardware, and -- on the GPU -- the oracle's strings on reads that go through both tables on every step.

Bank model (gfx950 LDS, ds_read_b32): 32 banks, bank = (byte address / 4) % 32; the 64 lanes of a wave are served as two
halves of 32; a half costs as many cycles as its fullest bank has DISTINCT addresses (lanes on one address share one
access), at least one.  A wave read of no conflicts is therefore 2.0 cycles.  The lanes of a wave are consecutive band
columns of one anti-diagonal, that is consecutive reference positions: a half is 32 consecutive `refw` entries.
"""
import os
import re

import numpy as np
import pytest

import oracle
import table_families as tf
from model import model
from npore_amd import aln, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "npore_amd", "csrc")


def _half_cycles(addr):
    """LDS cycles of one 32-lane half reading the byte addresses `addr`."""
    words = np.unique(np.asarray(addr, np.int64) >> 2)
    return int(np.bincount(words % 32, minlength=32).max())


def _wave_read_cycles(addr):
    """Mean LDS cycles per wave read over the 32-column halves of a chunk's columns (every 8th alignment of the half
    against the columns: where the band lies over the reference moves with the anti-diagonal)."""
    per_half = [_half_cycles(addr[k:k + 32]) for off in range(0, 32, 8) for k in range(off, len(addr) - 31, 32)]
    return 2.0 * float(np.mean(per_half)), len(per_half)


def test_first_candidate_score_read_is_nearly_conflict_free():
    """The score read of a column's first SHR candidate, no copy deleted yet (q = 0, nearly every step): the byte address
    is bits 15-30 of refw.z as the prep twin packs it (make_shr_desc), 0 for a column without a candidate.  Mean cycles
    per wave read <= 2.5 on seeded synthetic 10 kb reads (2.0 is the floor).  Figures: 2.25 with rows of 34 words; with
    rows of 33 words -- the layout before -- every descriptor lies on bank 0 and the same model gives 6.99, which is
    recomputed here from the descriptors' (period, L) so that the model is seen to tell the two apart."""
    new, old = [], []
    for k in range(6):
        ref, seq, cig = synth.make_pair(2, k, 10_000)
        p = model.prep(ref, seq, cig)
        z = p["refw"][:, 2].astype(np.int64)
        addr = (z >> 15) & 0xFFFF
        n, L = (z >> 2) & 7, (z >> 8) & 0x7F
        assert (n > 0).mean() > 0.05                         # the reads do have candidates
        in_table = (n > 0) & (L < 32) & (L > 0)
        # what the address means (layout.hpp): entry "call length L - 1" of row min(L, max_l - 1) = L of period n
        rows34 = ((n - 1) * 32 + L) * 34 + 32 - L
        assert np.array_equal(addr[in_table], 4 * rows34[in_table])
        assert int(addr.max()) + 4 * 31 < 6 * 32 * 34 * 4 and int(addr.max()) < 1 << 16
        new.append(_wave_read_cycles(addr))
        old.append(_wave_read_cycles(np.where(in_table, 4 * (((n - 1) * 32 + L) * 33 + 32 - L), 0)))
    mean = lambda xs: sum(c * w for c, w in xs) / sum(w for _, w in xs)
    print(f"first-candidate score read, LDS cycles per wave read: rows of 34 words {mean(new):.2f}, of 33 words {mean(old):.2f}")
    assert mean(new) <= 2.5
    assert mean(old) > 5.0


def _sub_index_ops():
    """(shift, mask, base) of the substitution-table read as the step assembly does it (gen_fill_asm.sub_read)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_fill_asm", os.path.join(CSRC, "gen_fill_asm.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    t = G.Text()
    G.sub_read(t)
    text = "\n".join(t.lines)
    shift = int(re.search(r"v_alignbit_b32 \S+ \S+ \S+ (\d+)", text).group(1))
    mask = int(re.search(r"v_and_b32 \S+ (0x[0-9a-f]+),", text).group(1), 16)
    base = int(re.search(r"ds_read_b32 \S+ \S+ offset:(\d+)", text).group(1))
    return shift, mask, base


def test_substitution_table_pairs_on_distinct_banks():
    """The 16 (ref, seq) pairs of the base codes 1 ... 4 read 16 different banks, whatever the other bits of the two
    words are: a wave's substitution read has no bank conflict.  The index is evaluated as the assembly computes it
    (v_alignbit_b32 of {refw.x, seqw}, then the mask), and the compiled step's (kernels.hpp DevEnv::sub) is the same."""
    shift, mask, base = _sub_index_ops()
    src = open(os.path.join(CSRC, "kernels.hpp")).read()
    m = re.search(r"alignbit\(refx, seqw, (\d+)\) & (0x[0-9A-Fa-f]+)u", src)
    assert (int(m.group(1)), int(m.group(2), 16)) == (shift, mask)
    assert base == 6 * 32 * 34 * 4 and base % 128 == 0
    rng = np.random.default_rng(11)
    banks = {}
    for rb in range(1, 5):
        for sb in range(1, 5):
            seen = set()
            for _ in range(64):           # own bases fixed, every other bit random
                seqw = (int(rng.integers(0, 1 << 29)) | sb << 29)
                refx = (int(rng.integers(0, 1 << 29)) << 3 | rb)
                off = (((refx << 32) | seqw) >> shift) & 0xFFFFFFFF & mask
                assert off == 4 * (rb << 3 | sb)                      # entry ref << 3 | seq of a [8][8] table
                seen.add(((base + off) >> 2) % 32)
            assert len(seen) == 1
            banks[(rb, sb)] = seen.pop()
    assert len(set(banks.values())) == 16, banks


# ---------------------------------------------------------------------------------------------------------------------

def _repeat_read(rng, k, n_blocks=10):
    """Flanks and the repeat blocks of table_families.BLOCKS, each with a copy-number change between read and reference
    in the middle of the block (both signs: LEN and SHR moves), and a substitution now and then."""
    ref, seq, cig = [], [], []
    order = [int(b) for b in rng.integers(0, len(tf.BLOCKS), n_blocks)]
    for i, b in enumerate(order):
        unit = tf.BLOCKS[b]
        flank = [int(x) for x in rng.integers(1, 5, int(rng.integers(5, 30)))]
        ref += flank; seq += flank; cig += ["="] * len(flank)
        if i % 3 == 0:                                   # a mismatch in front of the block
            ref.append(1 + (flank[0] % 4)); seq.append(1 + ((flank[0] + 1) % 4)); cig.append("X")
        d = int(rng.integers(1, 9))
        cut = int(rng.integers(len(unit) // 4, 3 * len(unit) // 4))
        if (k + i) % 2:                                  # copies missing in the read
            ref += unit; seq += unit[:cut] + unit[cut + d:]
            cig += ["="] * cut + ["D"] * d + ["="] * (len(unit) - cut - d)
        else:                                            # copies added in the read
            ref += unit[:cut] + unit[cut + d:]; seq += unit
            cig += ["="] * cut + ["I"] * d + ["="] * (len(unit) - cut - d)
    return np.array(ref, np.uint8), np.array(seq, np.uint8), "".join(cig)


@pytest.mark.gpu
@pytest.mark.parametrize("mbr", [64, 700])
def test_repeat_rich_reads_vs_oracle(mbr):
    """Repeat-rich reads -- every column with SHR candidates, LEN candidates on most rows -- at bands of two to seven
    waves per chunk, short and long chunks: every string and status equal to the live oracle's.  The test sees the LEN
    pass of the step assembly: a library built from the generator's --nolen text fails the case max_b_rows = 700 at its
    first read and band (checked once by hand).  Chunks of 64 anti-diagonals never leave the band's border region, so
    that case runs the compiled steps only -- and the tables through DevEnv::sub / np_small / np_full."""
    sub, nps, _, _ = aln.load_default_tables()
    rng = np.random.default_rng(77)
    reads = [_repeat_read(rng, k) for k in range(12)]
    refs, seqs, cigs = [x[0] for x in reads], [x[1] for x in reads], [x[2] for x in reads]
    c = aln.Context(sub, nps, device=0)
    try:
        moves = set()
        for r in (64, 95, 100, 127, 200):
            got, st = c.align_batch(refs, seqs, cigs, r=r, max_b_rows=mbr, return_status=True)
            for k in range(len(refs)):
                want, wst = oracle.align(refs[k], seqs[k], cigs[k], sub, nps, r=r, max_b_rows=mbr, return_status=True)
                assert got[k] == want and st[k] == wst, (r, mbr, k)
                moves |= set(want)
        assert {"I", "D", "=", "X"} <= moves, moves
    finally:
        c.close()
