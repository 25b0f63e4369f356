#!/usr/bin/env python3
"""Generates tests/golden/cigar_cases.npz: what the REFERENCE's own compiled mem_reg2aln (oracle/ref_tail_harness.cpp: ref_tail_reg2aln) returns for every
job of tests/cigar_cases.py that bwa_gen_cigar2 accepts, in table order.

  aln     int64 [n_jobs, 4] = pos, is_rev, n_cigar, NM
  cigar   uint32: the operations of all jobs (len << 4 | op, clips included), cg_off [n_jobs + 1] where a job's begin
  md      uint8: the MD strings of all jobs, md_off [n_jobs + 1]
  digest  the table's digest (cigar_cases.digest()): the test refuses a table that was edited without running this again

mem_reg2aln does not return the global score; that word is pinned through the oracle (tests/test_cigar_cases.py).  The regions the reference rejects
(empty, inverted, bridging the strands) have no row here: it has no CIGAR for them.

Runs only where the reference's sources are present (oracle/Makefile: ref).  Nothing here is produced by this project's kernels, host code or oracle."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cigar_cases  # noqa: E402
import oracle_py  # noqa: E402


def main():
    oracle_py.build(ref=True)
    ref = oracle_py.RefTail()
    jobs = cigar_cases.fixture_jobs()
    rows = [cigar_cases.reference_row(ref, j) for j in jobs]
    np.savez_compressed(os.path.join(HERE, "cigar_cases.npz"), digest=np.array(cigar_cases.digest()), **cigar_cases.pack_rows(rows))
    print(f"{len(cigar_cases.batches())} batches, {len(rows)} jobs, {sum(len(r['cigar']) for r in rows)} operations, {sum(len(r['MD']) for r in rows)} MD characters")


if __name__ == "__main__":
    main()
