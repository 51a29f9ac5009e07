#!/usr/bin/env python3
"""Records what the REAL reference objects (oracle/_ref/libbsmapref.so, built from the reference's sources by `make -C oracle ref`)
compute for every case of tests/test_oracle_boundaries.py, into boundaries_vs_reference.json.gz: per case a digest of its inputs, digests
of the packed genome and seed index, digests of the record of every read (tests/test_oracle_vs_reference.py: read_record, pair_record,
rrbs_record, sam_fields; summarize_records), the mapped bits, and per read class how many reads the reference found at their origin.
Only digests, labels and counts are stored; no reference source text.

What the script enforces from the reference's own answers:
  * every case is recorded twice, each time in a process of its own, and the two results must be identical — the reference reads undefined
    memory at exactly these places (the margins of the packed array; CCGG_seglen one past the site vector), and an input whose
    record differs between two runs has no recordable answer and is removed from the generator, not tolerated.  None of the recorded inputs
    differed.  Left out of the generator beforehand, for the reason DESIGN.md 4 gives: RRBS reads that lie inside their chromosome but end
    behind the last site's fragment end (bsx_testdata.boundary_rrbs_reads skips them) — for them the reference's CCGG_seglen takes the
    element past its site vector as the fragment end;
  * the floors of tests/test_oracle_boundaries.py: check_floors — at least 8 reads of every class found at their origin, at least 8 of every
    class beyond a limit (overhang, v + 1 mismatches, f + 1 N letters, inserts below -m or above -x, fragments outside [-m, -x]) not found.

Run where the reference is present:   python tests/golden/make_golden_boundaries.py
"""
import base64
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_oracle_boundaries as TB  # noqa: E402
import test_oracle_vs_reference as T  # noqa: E402
from oracle import ref_ffi as R  # noqa: E402


def record_case(kind, case, d):
    kw, g, fa, reads = TB.case_inputs(kind, case, d)
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
            sam = T.sam_fields(line) if not st.filtered else None
            mapped.append(sam is not None)
            recs.append([T.read_record(st, ref.se_hits, nclass), sam])
    recs = T._json(recs)
    total, short = T.summarize_records([T.record_digest(x) for x in recs])
    out = {"kw": kw, "inputs": T.input_digest(kind, fa, reads), "index": T.index_digests(kind, kw, ref), "n_reads": len(reads),
           "records": total, "read_digest16": short, "classes": TB.class_counts(kind, reads, recs)}
    if kind == "se":
        out["sam_mapped"] = base64.b64encode(np.packbits(np.array(mapped, bool)).tobytes()).decode()
    return T._json(out)


def main():
    if not R.available():
        assert R.build(), "needs the reference's sources (oracle/Makefile: REF)"
    cases = TB.all_cases()
    if len(sys.argv) > 3 and sys.argv[1] == "--case":   # one case in this process: its record as JSON into the named file
        kind, case = cases[sys.argv[2]]
        with tempfile.TemporaryDirectory() as d:
            rec = record_case(kind, case, d)
        with open(sys.argv[3], "w") as f:
            json.dump(rec, f, sort_keys=True)
        return
    out = {"cases": {}}
    for n, (name, (kind, case)) in enumerate(cases.items()):
        runs = []
        for _ in range(2):
            with tempfile.TemporaryDirectory() as d:
                subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, os.path.join(d, "rec.json")], check=True, stdout=subprocess.DEVNULL)
                runs.append(open(os.path.join(d, "rec.json")).read())
        if runs[0] != runs[1]:
            a, b = json.loads(runs[0]), json.loads(runs[1])
            da, db = base64.b64decode(a["read_digest16"]), base64.b64decode(b["read_digest16"])
            bad = [i for i in range(a["n_reads"]) if da[2 * i:2 * i + 2] != db[2 * i:2 * i + 2]]
            raise SystemExit("%s: the reference gave two answers in two runs; reads %s; differing keys %s" % (name, bad[:20], [k for k in a if a[k] != b[k]]))
        rec = json.loads(runs[0])
        TB.check_floors(kind, rec["classes"])
        out["cases"][name] = rec
        print("%d/%d %s %s" % (n + 1, len(cases), name, rec["classes"]), flush=True)
    with open(os.path.join(HERE, "boundaries_vs_reference.json.gz"), "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
            f.write(json.dumps(out, separators=(",", ":"), sort_keys=True).encode())


if __name__ == "__main__":
    main()
