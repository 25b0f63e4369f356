#!/usr/bin/env python3
"""Generates tests/golden/msw_cases.npz: what the REFERENCE's own compiled ksw_align2 (oracle/ref_harness.c: ref_align2, called as mem_matesw
calls it) returns for every job of tests/msw_cases.py, in table order.

  out    int32 [n_jobs, 7] = score, te, qe, score2, te2, tb, qb
  digest the table's digest (msw_cases.digest()): the test refuses a table that was edited without running this again

The jobs of the byte-overflow family whose first pass ends at 255 are recorded from that first pass alone (the call without KSW_XSTART): the
reference's second pass then runs over an empty query and reads in front of its arrays.  Its result, {255, te, -1, -1, -1, -1, -1}, is what
ksw_align2 returns for them as well.  No other job is treated this way, and no other job scores 255.

Runs only where the reference's sources are present (oracle/Makefile: ref).  Nothing here is produced by this project's kernels or host code."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import msw_cases  # noqa: E402
import oracle_py  # noqa: E402


def main():
    oracle_py.build(ref=True)
    ref = oracle_py.Ref()
    rows = []
    for name, c in msw_cases.all_cases().items():
        r = msw_cases.reference_rows(ref, c)
        assert (r[c.overflow, 0] == 255).all() and (r[~c.overflow, 0] != 255).all(), name
        rows.append(r)
    out = np.concatenate(rows)
    np.savez_compressed(os.path.join(HERE, "msw_cases.npz"), out=out, digest=np.array(msw_cases.digest()))
    print(f"{len(rows)} cases, {len(out)} jobs, {int((out[:, 0] == 255).sum())} overflows")


if __name__ == "__main__":
    main()
