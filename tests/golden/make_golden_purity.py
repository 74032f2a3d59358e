#!/usr/bin/env python3
"""Golden vectors for the Gini purity of pileup columns, from the reference's own `compute_purity` (src/purity.py:11-84).

Runs ONLY in the build container (needs /root/reference); see make_golden.py.

    python tests/golden/make_golden_purity.py        # rewrites tests/golden/purity.json

The reference reads its columns from `samtools mpileup ... | cut -f5`, upper-cased (src/purity.py:182-184); samtools is
absent here, so the INPUT columns of the fixture are hand-written ones that hit `^` + mapping quality, `$`, `*`, +k / -k
with multi-digit k, lower case and the same insertion twice, plus the columns of the golden reads (data/reads.bam) from the
pileup writer of tests/model/purity_model.py.  `pysam` and `matplotlib`, which the module imports and compute_purity does
not use, are stubbed the way make_golden_cms.py stubs `Bio`.  Every column is handed over the way the reference's main()
does it: upper-cased bytes."""
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, REF  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HAND = [
    "A", "AAAA", "ACGT", "AACC*", "****", "*", "a", "acgtACGT", "A$", "^]A", "^!a^~C$",
    "A+1C", "A+1CA+1C", "A+1CA+1G", "A+2ACA+2ACA+2AG", "a+2aca+2AC", "A+12ACGTACGTACGTA", "A+12ACGTACGTACGTA+12ACGTACGTACGTA+12ACGTACGTACGG",
    "A-1N", "A-1NA-1N", "A-12NNNNNNNNNNNNC", "a-3nnnC-2NN", "A-1NC+1T", "A+1T*", "*+1A", "*-1N",
    "^]A+3ACGT$", "^]A+3ACG^]A+3ACGT", "AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAC",
    "A+100" + "ACGT" * 25 + "A+100" + "ACGT" * 25 + "C", "ACGT*ACGT*ACGT*", "AAC", "AAAC", "AAAAC", "AAAAAAAC", "A+1CA", "A+1CAA", "A+1CAAA",
    "A+1CA+1CA", "A+1CA+2CCA", "A+1CA+1cA", "GGGGGGGGGT+1A", "T$T$T$", "^FT^FT", "C-10NNNNNNNNNNC-10NNNNNNNNNN", "g+15acgtacgtacgtacgG+15ACGTACGTACGTACG",
    "AC+2GTG*T-1N", "***A", "AAAAAAAAAA*", "CCCCC+3AAAC+3AAAC+3AAT", "", "^]", "$",
]


def main():
    for name in ("pysam", "matplotlib", "matplotlib.pyplot"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    spec = importlib.util.spec_from_file_location("ref_purity", os.path.join(REF, "src", "purity.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    from model import purity_model as pm
    from npore_amd import bam
    f = bam.BamFile(os.path.join(HERE, "data", "reads.bam"))
    ranges = [(n, 0, l) for n, l in zip(f.references, f.lengths)]
    written, _ = pm.write_columns(f.records, f.references, f.lengths, ranges, min_bq=0)
    rich = [c for c in written if c and (len(set(c.upper()) & set("ACGT*")) > 1 or "+" in c)]
    plain = [c for c in written if c and c not in rich]
    columns = HAND + rich[:120] + plain[:200 - len(HAND) - min(120, len(rich))]
    out = []
    for col in columns:
        res = ref.compute_purity(col.upper().encode())
        out.append({"column": col, "scores": None if res is None else [float(res[0]), float(res[1])]})
    with open(os.path.join(HERE, "purity.json"), "w") as fh:
        json.dump({"source": "src/purity.py compute_purity on the upper-cased column", "columns": out}, fh, indent=0)
    print(len(out), "columns,", sum(1 for o in out if o["scores"] is None), "without coverage")


if __name__ == "__main__":
    main()
