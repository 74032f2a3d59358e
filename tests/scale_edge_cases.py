"""Inputs of tests/test_gpu_scale_edges.py and tests/test_scale_edge_cases.py: the smallest inputs that reach the paths of the
purity, region and plane kernels which only run above a size threshold.  Every threshold stands next to the constant of
the kernel source it comes from.

  1. purity_kernels.hpp: the offsets of a window's insertion buckets are prefix sums over the window's positions, by blocks
     of PUR_SCAN_PER_BLOCK positions; purity_scan_top_kernel scans the blocks' sums PUR_TOP_ROUND at a time behind a carry.
     A window of more than 256 x 1024 = 262 144 positions is the first that uses the carry.  big_purity_case(): one contig
     of 518 blocks (three rounds, the last block partial) with insertions on both sides of every border.
  2. prep_kernels.hpp region_scan_kernel: REGION_SCAN_THREADS threads share the max_n x n_slices counts, `per` =
     ceil(max_n n_slices / 1024) consecutive counts each.  region_slices(): 170, 171 and 1 100 slices, so that at max_n = 6
     per is 1, 2 and 7 and the tail threads are empty.
  3. npore_api.cpp launch_np_info: a slice is cut into segments of NP_INFO_SEG positions, one wave each, warmed up on the
     np_info_warm() positions in front of its segment.  segment_sequence(): arrays of every period, a homopolymer longer
     than the warm-up, an N stretch and an array that starts exactly on a border; border_case(): a contig of two and a half
     segments with reads that carry copy-number INDELs at the polymer starts next to the borders.
"""
import numpy as np

# ---- 1. purity_kernels.hpp ---------------------------------------------------------------------------------------------
PUR_SCAN_PER_BLOCK = 1024                    # purity_kernels.hpp PUR_SCAN_PER_BLOCK: 256 threads, four positions each
PUR_TOP_ROUND = 256                          # purity_scan_top_kernel: blocks scanned per round (its workgroup's threads)
PUR_CARRY_FROM = PUR_SCAN_PER_BLOCK * PUR_TOP_ROUND      # 262 144: the first window position behind the carry
PURITY_WINDOW_DEFAULT = 1 << 22              # align_engine.hpp purity_window: 4 096 blocks, 16 rounds

BIG_NAME, BIG_LEN = "big", 530_000           # 518 blocks: rounds of 256, 256 and 6, the last block of 592 positions
ANCHORS = (5, 1023, 1024, 262_143, 262_144, 262_145, 263_167, 263_168, 524_287, 524_288, 524_988, 529_960)
ANCHOR_BLOCKS = (0, 0, 1, 255, 256, 256, 256, 257, 511, 512, 512, 517)
INSERTS = ("A", "AC", "A", "ACGTTGCAACGTTGCAT", "A")     # t = 5, sum v^2 = 3^2 + 1 + 1; the 17-mer takes the hashed key path
GAP_CUT = 2000                               # big_ranges()[1] leaves [1000, 3000) out: dense index = position - 2000 behind it


def _random_bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def big_purity_case(seed=21):
    """-> references, records.  Five reads per anchor a: a first M that ends ON a, the I of INSERTS, a closing M of 9 ... 13."""
    rng = np.random.default_rng(seed)
    ctg = _random_bases(rng, BIG_LEN)
    records = []
    for a in ANCHORS:
        for k, ins in enumerate(INSERTS):
            m0, m1 = min(a + 1, 14 + 3 * k), 9 + k
            pos = a + 1 - m0
            seq = ctg[pos:a + 1] + ins + ctg[a + 1:a + 1 + m1]
            records.append({"name": f"a{a}_{k}", "flag": 16 if k == 1 else 0, "ref_id": 0, "pos": pos, "cigar": [(0, m0), (1, len(ins)), (0, m1)],
                            "seq": seq, "qual": bytes([30] * len(seq))})
    records.sort(key=lambda r: r["pos"])
    return [(BIG_NAME, BIG_LEN)], records


def big_ranges():
    """the whole contig; the contig without [1000, 3000): dense index != contig position across the block-256 border"""
    return [[(BIG_NAME, 0, BIG_LEN)], [(BIG_NAME, 0, 1000), (BIG_NAME, 1000 + GAP_CUT, BIG_LEN)]]


# ---- 2. prep_kernels.hpp region_scan_kernel ----------------------------------------------------------------------------
REGION_SCAN_THREADS = 1024                   # region_scan_kernel's one workgroup (block_scan_1024)
STRIDE_LENGTHS = (0, 1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)      # around a wave, region_emit's 256, region_count's 1024
REGION_SLICE_COUNTS = (170, 171, 1100)       # x max_n = 6: 1 020, 1 026 and 6 600 counts
REGION_CONTEXTS = [(170, 6, 100), (171, 6, 100), (1100, 6, 100), (1100, 4, 20), (1100, 1, 5)]


def scan_per(n_slices, max_n):
    """`per` of region_scan_kernel: the counts one thread sums"""
    return (max_n * n_slices + REGION_SCAN_THREADS - 1) // REGION_SCAN_THREADS


def region_slices(n_slices, seed=0):
    """-> (slices, kinds).  kinds[j]: 'empty' (length 0, in runs of ten), 'plain' (random bases: few or no starts) or 'rich'
    (synth.make_ref at p_np = 0.2, what tests/test_bed.py tricky_sequences draws).  Runs of ten empty slices and three plain
    ones behind each: at the front, at multiples of 7, 2 and 5 slices (thread borders of per = 7, 2 and 5 in the first period's
    counts; the other periods' counts are shifted by n_slices mod per) a third and two thirds in, and in front of the LAST
    slice, which is a rich one of 257 bases.  Lengths of the rich slices: STRIDE_LENGTHS in turn for every third slice, the
    smaller of two draws <= 600 for the others.  An empty slice has length 0 whatever its turn, and a plain one at least 40
    bases (a turn of 0, 1 or 3 becomes 40 there; every stride length still falls on rich slices, which the CPU test asserts)."""
    from npore_amd import synth
    rng = np.random.default_rng(1000 * n_slices + seed)
    kinds = ["rich"] * n_slices
    for s in (0, 70 * (n_slices // 210), 70 * (n_slices // 105), n_slices - 14):
        for j in range(s, s + 10):
            kinds[j] = "empty"
        for j in range(s + 10, s + 13):
            kinds[j] = "plain"
    slices = []
    for j, kind in enumerate(kinds):
        n = STRIDE_LENGTHS[(j // 3) % len(STRIDE_LENGTHS)] if j % 3 == 0 else int(min(rng.integers(0, 601, 2)))
        if j == n_slices - 1:
            n = 257
        if kind == "empty":
            s = np.zeros(0, np.uint8)
        elif kind == "plain":
            s = rng.integers(1, 5, max(n, 40)).astype(np.uint8)
        else:
            s = synth.make_ref(rng, max(n, 8), 0.2)[0][:n]
        slices.append(np.ascontiguousarray(s, np.uint8))
    return slices, kinds


# ---- 3. npore_api.cpp launch_np_info -----------------------------------------------------------------------------------
NP_INFO_SEG = 16384                          # launch_np_info: q.seg, the positions one wave writes
SEGMENT_CONTEXTS = [(6, 100), (6, 127), (4, 20), (3, 5)]
HEXAMER = (1, 2, 3, 4, 1, 3)                 # no shorter period


def np_info_warm(max_n, max_l):
    """launch_np_info: q.warm, the positions a wave annotates in front of its segment (2 176 at max_n = 6, max_l = 100)"""
    return (sum((max_l + 2) * k for k in range(1, max_n + 1)) + 63) & ~63


def segment_sequence(rng, kind, n=70_000, plant=()):
    """A sequence far longer than one segment.  kind 0: arrays of every period back to back; kind 1: two letters (periodic
    everywhere).  Arrays of 1 000 positions are planted across every segment border, at every phase, then four N stretches.
    plant (after every draw, so that it changes none): ("homopolymer", b): 3 000 equal bases, longer than the warm-up, from
    b - 2 500 on; ("n_stretch", b): 100 N from b - 40 on; ("hexamer", b): 30 copies of HEXAMER whose start is exactly b;
    ("short_array", b): 14 copies of a dinucleotide from b - 20 on.  (An array of more than max_l copies says nothing about
    the warm-up: every position that has more than max_l copies ahead is a start whatever came before.  The short array
    does: position b is no start, and a wave that began at b would make it one.)"""
    if kind == 0:
        parts = []
        while sum(map(len, parts)) < n:
            per = int(rng.integers(1, 7))
            parts.append(np.tile(rng.integers(1, 5, per).astype(np.uint8), int(rng.integers(3, 400))))
            parts.append(rng.integers(1, 5, int(rng.integers(0, 6))).astype(np.uint8))
        s = np.concatenate(parts)[:n]
    else:
        s = rng.integers(1, 3, n).astype(np.uint8)
    for b in (16384, 32768, 49152):              # arrays planted across every segment boundary, at every phase
        if b >= n + 900:
            continue
        per = int(rng.integers(1, 7))
        a = b - int(rng.integers(1, 900))
        if a + per > n:
            continue
        m = min(1000, n - a)
        s[a:a + m] = np.tile(s[a:a + per], 1000 // per + 1)[:m]
    for _ in range(4):
        a = int(rng.integers(0, n - 50))
        s[a:a + int(rng.integers(1, 40))] = 0
    for what, b in plant:
        if what == "homopolymer":
            s[b - 2500:b + 500] = 3
        elif what == "n_stretch":
            s[b - 40:b + 60] = 0
        elif what == "hexamer":
            s[b - 1] = 2                         # != HEXAMER[5]: the array cannot start earlier
            s[b:b + 180] = np.tile(np.array(HEXAMER, np.uint8), 30)
            s[b + 180] = 2                       # ... and ends here
        elif what == "short_array":
            s[b - 21] = s[b + 8] = 4                 # 14 copies of (1, 2), four of them behind b: below every max_l, so the
            s[b - 20:b + 8] = np.tile(np.array([1, 2], np.uint8), 14)      # values at b hang on the start 20 positions before
        else:
            raise ValueError(what)
    return s


def border_slices(seed=31):
    """One np_regions call: slices of NP_INFO_SEG - 1, NP_INFO_SEG, NP_INFO_SEG + 1, 40 000 and 70 000 positions between three
    short ones, so that no long slice starts at an offset that is a multiple of anything."""
    rng = np.random.default_rng(seed)
    short = lambda n: np.concatenate([np.tile(rng.integers(1, 5, int(rng.integers(1, 7))).astype(np.uint8), int(rng.integers(3, 30)))
                                      for _ in range(40)])[:n]
    B = NP_INFO_SEG
    return [short(701), segment_sequence(rng, 0, B - 1), segment_sequence(rng, 0, 70_000, [("homopolymer", B), ("n_stretch", 2 * B), ("hexamer", 3 * B), ("short_array", 4 * B)]),
            short(63), segment_sequence(rng, 1, B), segment_sequence(rng, 0, 40_000, [("hexamer", B), ("n_stretch", 2 * B)]),
            segment_sequence(rng, 0, B + 1), short(1300)]


BORDER_NAME, BORDER_LEN = "seg", 40_000      # both borders, 16 384 and 32 768, inside
BORDERS = (NP_INFO_SEG, 2 * NP_INFO_SEG)


def polymer_starts(info):
    """{position: [periods that start an n-polymer there]} of a get_np_info() result"""
    st = (info[:, 0] != 0) & (info[:, 1] == 0)
    return {int(p): [int(m) + 1 for m in np.nonzero(st[p])[0]] for p in np.nonzero(st.any(axis=1))[0]}


class _Read:
    """a read under construction on the contig ctg: CIGAR operations, their bases, the reference position r behind them"""

    def __init__(self, ctg, pos):
        self.ctg, self.pos, self.r, self.cigar, self.seq = ctg, pos, pos, [], []

    def match(self, rng, m):
        """m positions as M, = or X, three in a hundred of them redrawn"""
        chunk = list(self.ctg[self.r:self.r + m])
        for i in range(m):
            if rng.random() < .03:
                chunk[i] = "ACGT"[int(rng.integers(0, 4))]
        self.cigar.append((int(rng.choice([0, 0, 7, 8])), m))
        self.seq.append("".join(chunk))
        self.r += m

    def insert(self, bases):
        self.cigar.append((1, len(bases)))
        self.seq.append(bases)

    def delete(self, d):
        self.cigar.append((2, d))
        self.r += d

    def record(self, rng, name):
        if self.cigar[-1][0] in (1, 2):              # close with a match so that the record ends on the contig
            self.cigar.append((0, 3))
            self.seq.append(self.ctg[self.r:self.r + 3])
            self.r += 3
        seq = "".join(self.seq)
        u = rng.random()
        strand = 16 if rng.random() < .5 else 0
        excluded = 0x400 if u < .05 else 0x800 if u < .1 else 0
        qual = bytes(int(x) for x in rng.choice([7, 12, 13, 20, 30, 40], size=len(seq), p=[.03, .03, .04, .2, .4, .3]))
        return {"name": name, "flag": strand | excluded, "ref_id": 0, "pos": self.pos, "cigar": self.cigar, "seq": seq, "qual": qual}


def _forced_starts(starts):
    """the polymer starts nearest to each border: the first at or behind it, the last in front of it"""
    where = np.array(sorted(starts))
    forced = set()
    for b in BORDERS:
        forced.add(int(where[where >= b][0]))
        forced.add(int(where[(where < b) & (where > b - 140)][-1]))
    return forced


def _placement(rng, k):
    """(pos, span) of read k: the even reads start within 150 bases of a border, the odd ones anywhere"""
    if k % 2:
        span = int(rng.integers(40, 300))
        return int(rng.integers(0, BORDER_LEN - span - 40)), span
    b = BORDERS[(k // 2) % 2]
    pos, span = b + int(rng.integers(-150, 151)), int(rng.integers(200, 400))
    if k % 8 == 0:
        pos = b - 150 + k // 8                       # ... some of them certainly in front of both forced starts
    return pos, span


def _match_length(rng, r, end, starts, forced):
    """up to the next forced start if one lies within 60 bases (inside an array of more than max_l copies every position is
    a start: the nearest start would never be the forced one), else, six times in ten, up to the next start, else 3 ... 24"""
    ahead = [p for p in range(r + 1, min(end, r + 60)) if p in starts]
    must = [p for p in ahead if p in forced]
    if must:
        return must[0] - r
    if ahead and rng.random() < .6:
        return ahead[0] - r
    return int(min(end - r, rng.integers(3, 25)))


def _indel(rng, read, starts, forced):
    """behind a match: at a forced start always, at another start every other time, one or two copies of a unit that starts
    there gained or lost; elsewhere, three times in ten, a short INDEL of other bases"""
    r = read.r
    if r in starts and (r in forced or rng.random() < .5):
        n = int(rng.choice(starts[r]))
        copies = int(rng.integers(1, 3))
        if rng.random() < .5:
            read.insert(read.ctg[r:r + n] * copies)
        else:
            read.delete(n * copies)
    elif rng.random() < .3:
        if rng.random() < .5:
            read.insert("".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 5)))))
        else:
            read.delete(int(rng.integers(1, 6)))


def border_case(seed=41, n_reads=80):
    """-> references, refs, records, forced.  A contig of BORDER_LEN bases from segment_sequence (a hexamer array starts at
    16 384, a short dinucleotide array crosses 32 768) and n_reads reads placed like cms_model.make_random_bam's: the even
    ones start within 150 bases of a border and carry a copy-number INDEL at the polymer starts nearest to it on either side (`forced`), and at half of the other starts
    they cross; the odd ones lie anywhere.  Both strands, qualities on both sides of 13, a few excluded reads."""
    import oracle
    rng = np.random.default_rng(seed)
    codes = segment_sequence(rng, 0, BORDER_LEN, [("hexamer", NP_INFO_SEG), ("short_array", 2 * NP_INFO_SEG)])
    ctg = np.frombuffer(b"NACGT", np.uint8)[codes].tobytes().decode()
    starts = polymer_starts(np.asarray(oracle.get_np_info(codes, max_n=6, max_l=100)))
    forced = _forced_starts(starts)
    records = []
    for k in range(n_reads):
        pos, span = _placement(rng, k)
        read, end = _Read(ctg, pos), pos + span
        while read.r < end:
            read.match(rng, _match_length(rng, read.r, end, starts, forced))
            if read.r >= end:
                break
            _indel(rng, read, starts, forced)
        records.append(read.record(rng, f"b{k}"))
    records.sort(key=lambda r: r["pos"])
    return [(BORDER_NAME, BORDER_LEN)], {BORDER_NAME: ctg}, records, sorted(forced)


def border_range_sets(references):
    """the whole contig as one range; chunks of 20 000 (a range across each border) and of NP_INFO_SEG (ranges that end on them)"""
    from model import cms_model
    return [[(BORDER_NAME, 0, BORDER_LEN)], cms_model.whole_contig_ranges(references, 20000), cms_model.whole_contig_ranges(references, NP_INFO_SEG)]
