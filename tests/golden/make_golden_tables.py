#!/usr/bin/env python3
"""G8 tables_variety.npz: the reference's own align() under score tables other than the shipped ones.

Runs ONLY in the build container (needs /root/reference + Cython + gcc); see make_golden.py.  The reference is compiled
in a throw-away directory outside the repo; only the outputs below are written.

    python tests/golden/make_golden_tables.py     # rewrites tests/golden/tables_variety.npz

For every table set of tests/table_families.py (TABLE_SETS) the file holds
    {name}/sub, {name}/np, {name}/indel (start, extend), {name}/shape (max_n, max_l), {name}/seed
and for every configuration (r, max_b_rows) of G8_CONFIGS, per read of table_families.input_set(max_l, INPUT_SEED),
    {name}/r{r}_m{mbr}/len   int32  length of the reference's string (-1: the reference was not asked: an empty strand)
    {name}/r{r}_m{mbr}/dig   uint64 first 16 hex digits of its sha256
plus input/seed, input/configs and the reference's calc_score_matrices of the cms.json counts (recalc/sub, recalc/np
are those; recalc/ins, recalc/del the other two outputs).
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, build_reference, import_reference  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import table_families as tf  # noqa: E402

INPUT_SEED = 0
G8_CONFIGS = ((1, 20000), (5, 7), (30, 20000), (30, 333), (100, 333), (230, 7), (300, 150))


def digest(s):
    return int(hashlib.sha256(s.encode()).hexdigest()[:16], 16)


def main():
    out = {"input/seed": np.array([INPUT_SEED], np.int64), "input/configs": np.array(G8_CONFIGS, np.int32)}
    with tempfile.TemporaryDirectory(prefix="npore_ref_") as wd:
        rcfg, raln, _ = import_reference(build_reference(wd))
        g1 = np.load(os.path.join(HERE, "tables.npz"))
        for name, (fam, seed, max_n, max_l, kw) in tf.TABLE_SETS.items():
            rcfg.args.max_n, rcfg.args.max_l = max_n, max_l
            if fam is tf.recalc:
                rsub, rnp, rins, rdel = raln.calc_score_matrices(*tf.cms_counts(max_n, max_l))
                out["recalc/ins"], out["recalc/del"] = np.asarray(rins, np.float32), np.asarray(rdel, np.float32)
                sub, nps, ist, iex = tf.recalc(seed, max_n, max_l, calc_score_matrices=lambda *a: (rsub, rnp, rins, rdel))
            elif fam is tf.ulp:
                sub, nps, ist, iex = tf.ulp(seed, max_n, max_l, base=(g1["sub_scores"], g1["np_scores"]))
            else:
                sub, nps, ist, iex = fam(seed, max_n, max_l, **kw)
            assert sub.dtype == nps.dtype == np.float32 and nps.shape == (max_n, max_l + 1, max_l + 1)
            out[f"{name}/sub"], out[f"{name}/np"] = sub, nps
            out[f"{name}/indel"] = np.array([ist, iex], np.float64)
            out[f"{name}/shape"] = np.array([max_n, max_l], np.int32)
            out[f"{name}/seed"] = np.array([seed], np.int64)
            reads = tf.input_set(max_l, INPUT_SEED)
            for r, mbr in G8_CONFIGS:
                ln = np.full(len(reads), -1, np.int32)
                dg = np.zeros(len(reads), np.uint64)
                for k, (ref, seq, cig, _) in enumerate(reads):
                    if len(ref) == 0 or len(seq) == 0:
                        continue
                    s = raln.align(ref, seq, cig, sub, nps, indel_start=ist, indel_extend=iex, max_b_rows=mbr, r=r)
                    ln[k], dg[k] = len(s), digest(s)
                out[f"{name}/r{r}_m{mbr}/len"], out[f"{name}/r{r}_m{mbr}/dig"] = ln, dg
            print(name, (max_n, max_l), "reads", len(reads), flush=True)
    np.savez_compressed(os.path.join(HERE, "tables_variety.npz"), **out)
    print("G8:", os.path.getsize(os.path.join(HERE, "tables_variety.npz")), "bytes")


if __name__ == "__main__":
    main()
