#!/usr/bin/env python3
"""Records what the REAL reference objects (oracle/_ref/libbsmapref.so, built from the reference's sources by `make -C oracle ref`)
compute for every case of tests/test_oracle_vs_reference.py, into oracle_vs_reference.json.gz: per case a digest of its inputs,
digests of the packed genome and seed index, and digests of the record of every read (tests/test_oracle_vs_reference.py: read_record,
pair_record, rrbs_record, sam_fields; summarize_records).  Only data is stored; no reference source text.

Run where the reference is present:   python tests/golden/make_golden_vs_reference.py
"""
import base64
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_oracle_vs_reference as T  # noqa: E402
from oracle import ref_ffi as R  # noqa: E402


def record_case(kind, case, genome):
    kw, fa, reads = T.case_inputs(kind, case, genome)
    ref = R.Reference(fa, **kw)
    nclass = kw["v"] + 1
    recs, mapped = [], []
    for i, r in enumerate(reads):
        if kind == "pe":
            st, _, _ = ref.pe(i, r["name"] + "/1", r["seq1"], r["qual1"], r["name"] + "/2", r["seq2"], r["qual2"])
            recs.append(T.pair_record(st, ref.pe_hits, ref.pe_pairs, nclass))
        elif kind == "rrbs":
            st, _ = ref.se(i, r["name"], r["seq"], r["qual"])
            recs.append(T.rrbs_record(st, ref.se_hits, nclass))
        else:
            st, line = ref.se(i, r["name"], r["seq"], r["qual"])
            sam = T.sam_fields(line) if kw.get("out_sam") and not st.filtered else None
            mapped.append(sam is not None)
            recs.append([T.read_record(st, ref.se_hits, nclass), sam])
    total, short = T.summarize_records([T.record_digest(x) for x in recs])
    out = {"kw": kw, "inputs": T.input_digest(kind, fa, reads), "index": T.index_digests(kind, kw, ref), "n_reads": len(reads),
           "records": total, "read_digest16": short}
    if kind == "se":
        out["sam_mapped"] = base64.b64encode(np.packbits(np.array(mapped, bool)).tobytes()).decode()
    return out


def main():
    if not R.available():
        assert R.build(), "needs the reference's sources (oracle/Makefile: REF)"
    cases = T.all_cases()
    out = {"cases": {}}
    with tempfile.TemporaryDirectory() as d:
        genome = T.make_genomes(d)
        for n, (name, (kind, case)) in enumerate(cases.items()):
            out["cases"][name] = T._json(record_case(kind, case, genome))
            print("%d/%d %s" % (n + 1, len(cases), name), flush=True)
    with open(os.path.join(HERE, "oracle_vs_reference.json.gz"), "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
            f.write(json.dumps(out, separators=(",", ":")).encode())


if __name__ == "__main__":
    main()
