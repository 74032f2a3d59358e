"""Score tables other than the shipped ones, and the input set that is aligned under them (tests/test_gpu_tables.py,
tests/test_oracle_golden.py, tests/test_model_vs_oracle.py, tests/golden/make_golden_tables.py).

A family is a function (seed, max_n=6, max_l=100) -> (sub f32[5,5], np f32[max_n, max_l+1, max_l+1], indel_start,
indel_extend).  The families draw from NumPy's random streams, so the tests never call them: they load the tables that
make_golden_tables.py stored in tests/golden/tables_variety.npz (G8) through `load()`.  The input set is different:
input_set() draws its reads from NumPy's Generator (and npore_amd.synth) at test time, and G8 keeps only its seed and the
reference's per-read digests -- a change of NumPy's streams would make the G8 checks fail loudly, as it would G5's.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def random(seed, max_n=6, max_l=100, np_step=None):
    """Every entry drawn on its own with a full mantissa: an asymmetric sub with a non-zero diagonal and non-zero N row
    and column, np entries in [-1, 25], penalties that are not exact in binary.  np_step: np entries on that grid
    instead (a large table that has to stay small in G8)."""
    rng = np.random.default_rng(seed)
    sub = rng.uniform(0.5, 12.0, (5, 5))
    sub[np.diag_indices(5)] = rng.uniform(0.01, 2.0, 5)
    nps = rng.uniform(-1.0, 25.0, (max_n, max_l + 1, max_l + 1))
    if np_step:
        nps = np.round(nps / np_step) * np_step
    return sub.astype(F32), nps.astype(F32), 4.3, 0.7


def grid(seed, max_n=6, max_l=100):
    """Multiples of 1/4, some negative, penalties on the same grid: ties everywhere."""
    rng = np.random.default_rng(seed)
    sub = rng.integers(-2, 24, (5, 5)) / 4.0
    nps = rng.integers(-4, 40, (max_n, max_l + 1, max_l + 1)) / 4.0
    return sub.astype(F32), nps.astype(F32), 1.5, 0.25


def equal(seed, max_n=6, max_l=100):
    """Every entry 1: every candidate of a cell ties with its neighbours."""
    return np.ones((5, 5), F32), np.ones((max_n, max_l + 1, max_l + 1), F32), 1.0, 0.0


def cms_counts(max_n=6, max_l=100):
    """The count matrices of tests/golden/cms.json summed over its cases (subs [5,5], nps [max_n, max_l+1, max_l+1],
    inss / dels [max_l+1], int64): what `realign --recalc_cms` over a small region writes to --stats_dir."""
    with open(os.path.join(GOLDEN, "cms.json")) as fh:
        g = json.load(fh)
    assert (g["max_n"], g["max_l"]) == (max_n, max_l)
    subs = np.zeros((5, 5), np.int64)
    nps = np.zeros((max_n, max_l + 1, max_l + 1), np.int64)
    inss = np.zeros(max_l + 1, np.int64)
    dels = np.zeros(max_l + 1, np.int64)
    for c in g["cases"]:
        subs += np.array(c["subs"], np.int64)
        inss += np.array(c["inss"], np.int64)
        dels += np.array(c["dels"], np.int64)
        for a, b, d, v in c["nps_nonzero"]:
            nps[a, b, d] += v
    return subs, nps, inss, dels


def recalc(seed, max_n=6, max_l=100, calc_score_matrices=None):
    """calc_score_matrices of the sparse cms.json counts: mostly the eps constant plus fix_matrix_properties' ramps.
    `calc_score_matrices` defaults to the product's (npore_amd.aln, under cfg.args' max_n / max_l)."""
    if calc_score_matrices is None:
        from npore_amd import aln
        calc_score_matrices = aln.calc_score_matrices
    sub, nps, _, _ = calc_score_matrices(*cms_counts(max_n, max_l))
    return np.asarray(sub, F32), np.asarray(nps, F32), 5.0, 1.0


def ulp(seed, max_n=6, max_l=100, base=None):
    """G1 (tests/golden/tables.npz unless `base` is given) with entries moved by 1...3 ulp either way, signed zeros,
    a few f32 denormals in sub and np, and a few +inf np entries: catches reassociation, flush-to-zero and a wrong
    operand order in a candidate's add."""
    rng = np.random.default_rng(seed)
    if base is None:
        z = np.load(os.path.join(GOLDEN, "tables.npz"))
        base = z["sub_scores"], z["np_scores"]
    sub = np.array(base[0], F32)
    nps = np.array(base[1][:max_n, :max_l + 1, :max_l + 1], F32)
    for t in (sub, nps):
        flat = t.reshape(-1)
        pick = rng.random(flat.size) < 0.5
        steps = rng.integers(1, 4, flat.size) * rng.choice([-1, 1], flat.size)
        moved = flat.copy()
        for _ in range(3):                      # nextafter one ulp at a time, up to |steps| times
            go = pick & (np.abs(steps) > 0)
            moved[go] = np.nextafter(moved[go], np.where(steps[go] > 0, F32(np.inf), F32(-np.inf)))
            steps = steps - np.sign(steps)
        flat[:] = moved
    sub[0, 0] = F32(-0.0); sub[2, 2] = F32(-0.0); sub[0, 3] = F32(-0.0)
    den = np.array([1e-45, 3e-39, -2e-40, 1.1e-38], F32)          # denormals of f32 (and the smallest normal's neighbour)
    assert (np.abs(den) < np.finfo(F32).tiny).all() and (den != 0).all()
    sub[1, 1], sub[3, 3], sub[4, 0] = den[0], den[1], den[2]
    zeros = np.argwhere(nps == 0)
    for k, i in enumerate(rng.choice(len(zeros), min(len(zeros), 40), replace=False)):
        nps[tuple(zeros[i])] = F32(-0.0) if k % 2 else den[k % 4]
    for i in range(max_n):                       # single-step calls: L -> L +- 1 of short polymers
        for L in range(3, min(max_l, 12)):
            nps[i, L, L + (1 if (i + L) % 2 else -1)] = den[(i + L) % 4]
    for i, L, c in ((0, 7, 2), (1, 3, 9), (2, 5, 1), (0, 20, 30)):
        if i < max_n and max(L, c) <= max_l:
            nps[i, L, c] = F32(np.inf)
    return sub, nps, 5.0, 1.0


def inf_boundary(seed, max_n=6, max_l=100):
    """Entries in [60, 200], indel_start 120, indel_extend 60: the single-move penalties reach the reference's
    INF = 100 (src/aln.pyx:426-428), its band edges and start values take part in the minima, and its traceback
    stops on run < 1 (status bit 4) and returns truncated strings."""
    rng = np.random.default_rng(seed)
    sub = rng.uniform(60.0, 200.0, (5, 5))
    nps = rng.uniform(60.0, 200.0, (max_n, max_l + 1, max_l + 1))
    return sub.astype(F32), nps.astype(F32), 120.0, 60.0


# name -> (family function, seed, max_n, max_l, keyword arguments) of every table set kept in G8
TABLE_SETS = {
    "random": (random, 1, 6, 40, {}),
    "grid": (grid, 2, 6, 40, {}),
    "equal": (equal, 0, 6, 100, {}),
    "recalc": (recalc, 0, 6, 100, {}),
    "ulp": (ulp, 5, 6, 100, {}),
    "inf_boundary": (inf_boundary, 6, 6, 40, {}),
    "random_6_100": (random, 7, 6, 100, {}),
    "random_6_127": (random, 8, 6, 127, {"np_step": 1 / 4}),
    "random_4_20": (random, 9, 4, 20, {}),
    "random_6_5": (random, 10, 6, 5, {}),
    "random_3_31": (random, 11, 3, 31, {}),
}
FAMILIES = {"random": random, "grid": grid, "equal": equal, "recalc": recalc, "ulp": ulp, "inf_boundary": inf_boundary}


# ---------------------------------------------------------------------------------------------------------------------
# the input set

A, C, G, T = 1, 2, 3, 4
BLOCKS = [[A] * 150, [A, C] * 70, [A, C, G] * 45, [A] * 40 + [C] * 33, [A, A, C, A, A, C] * 30,
          [G, T, G, T, G, T, G, T, A] * 12, [T] * 101, [C, A, G, T] * 36, [A] * 12 + [A, C] * 9 + [A, C, G] * 7,
          [G] * 34 + [G, C] * 17, [C] * 45]


def _polymer_read(rng, k, blocks):
    """Flanks and repeat blocks with copy-number changes between read and reference: polymers of >= 32 copies and
    longer than max_l, columns where several periods meet (more than two SHR candidates)."""
    ref, seq, cig = [], [], []
    for b in rng.permutation(len(blocks))[:4]:
        unit = blocks[b]
        flank = [int(x) for x in rng.integers(1, 5, int(rng.integers(5, 25)))]
        if k % 3 == 0:
            flank[int(rng.integers(0, len(flank)))] = 0          # an N in both strands
        ref += flank; seq += flank; cig += ["="] * len(flank)
        drop = int(rng.integers(1, 9)) * (1 if (k + b) % 2 else -1)
        ref += unit
        if drop >= 0:
            seq += unit[:len(unit) - drop]; cig += ["="] * (len(unit) - drop) + ["D"] * drop
        else:
            seq += unit + unit[:(-drop)]; cig += ["="] * len(unit) + ["I"] * (-drop)
    return np.array(ref, np.uint8), np.array(seq, np.uint8), "".join(cig)


def _clamp_read(rng, max_l, unit_len):
    """A polymer of max_l - 1 + d copies in the reference and max_l - 1 + e in the read (d, e in -1 ... 2): a LEN
    candidate of the reference row max_l - 1 or max_l, which np_score clamps to row max_l - 1."""
    unit = [int(x) for x in rng.integers(1, 5, unit_len)]
    if unit_len == 2 and unit[0] == unit[1]:
        unit[1] = unit[0] % 4 + 1
    cr = max(2, max_l - 1 + int(rng.integers(-1, 3)))
    cs = max(1, cr + int(rng.choice([-2, -1, 1, 2])))
    f1 = [int(x) for x in rng.integers(1, 5, int(rng.integers(4, 12)))]
    f2 = [int(x) for x in rng.integers(1, 5, int(rng.integers(4, 12)))]
    ref = f1 + unit * cr + f2
    seq = f1 + unit * cs + f2
    m = min(cr, cs) * unit_len
    body = "=" * m + ("D" * ((cr - cs) * unit_len) if cr > cs else "I" * ((cs - cr) * unit_len))
    return np.array(ref, np.uint8), np.array(seq, np.uint8), "=" * len(f1) + body + "=" * len(f2)


def input_set(max_l, seed=0):
    """The reads aligned under every table set: list of (ref uint8[], seq uint8[], expanded cigar str, kind)."""
    from npore_amd import synth
    rng = np.random.default_rng(4000 + seed)
    out = []
    for k in range(14):                                   # fuzz reads, N in both strands
        ref, seq, cig = synth.make_pair(4100 + seed, k, int(rng.integers(1, 650)), float(rng.choice([0.0, 0.05, 0.15, 0.4])),
                                        float(rng.choice([0.0, 0.3, 0.9])))
        ref, seq = ref.copy(), seq.copy()
        if len(ref) > 3:
            ref[rng.integers(0, len(ref), size=3)] = 0
        if len(seq) > 3:
            seq[rng.integers(0, len(seq), size=3)] = 0
        out.append((ref, seq, cig.decode(), "fuzz"))
    for k in range(8):
        out.append(_polymer_read(rng, k, BLOCKS) + ("polymer",))
    for k in range(6):
        out.append(_clamp_read(rng, max_l, (1, 1, 2, 3, 1, 2)[k]) + ("clamp",))
    for k in range(3):                                    # input path far from the best one
        ref, seq, _ = synth.make_pair(4200 + seed, k, int(rng.integers(200, 500)), 0.15, 0.5)
        m = min(len(ref), len(seq)) - 30
        out.append((ref, seq, "I" * (len(seq) - m) + "D" * (len(ref) - m) + "=" * m, "far"))
    ref, seq, _ = out[14][:3]                             # ... and through polymers
    m = min(len(ref), len(seq)) - 20
    out.append((ref, seq, "D" * (len(ref) - m) + "I" * (len(seq) - m) + "=" * m, "far"))
    b = lambda s: np.array(["NACGT".index(ch) for ch in s], np.uint8)
    for ref, seq, cig in (("", "", ""), ("A", "A", "="), ("N", "N", "="), ("A", "G", "X"), ("N", "C", "X"),
                          ("A", "", "D"), ("", "T", "I"), ("C", "CC", "=I"), ("GG", "G", "=D")):
        out.append((b(ref), b(seq), cig, "tiny"))
    return out


def load(name):
    """(sub, np, indel_start, indel_extend, max_n, max_l) of a table set as G8 holds it."""
    z = _g8()
    return (z[f"{name}/sub"], z[f"{name}/np"], float(z[f"{name}/indel"][0]), float(z[f"{name}/indel"][1]),
            int(z[f"{name}/shape"][0]), int(z[f"{name}/shape"][1]))


_G8 = None


def _g8():
    global _G8
    if _G8 is None:
        _G8 = dict(np.load(os.path.join(GOLDEN, "tables_variety.npz")))
    return _G8


def g8():
    return _g8()


def g8_check(name, got, r, mbr):
    """got[k]: the string of read k of input_set under table set `name` at (r, max_b_rows), a configuration of G8; every
    read the reference was run on must give the reference's string (length + sha256[:16]).  Returns how many were."""
    import hashlib
    z = _g8()
    ln, dg = z[f"{name}/r{r}_m{mbr}/len"], z[f"{name}/r{r}_m{mbr}/dig"]
    n = 0
    for k, (l, d) in enumerate(zip(ln.tolist(), dg.tolist())):
        if l >= 0:
            assert len(got[k]) == l and int(hashlib.sha256(got[k].encode()).hexdigest()[:16], 16) == d, (name, r, mbr, k)
            n += 1
    return n
