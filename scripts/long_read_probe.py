"""Cell rate of the long-query extension kernel (bmh_extend_batch_long) on flanks of 1 000 / 2 500 / 8 000 query bases, and of
extend_wide_kernel<12> on 705..768-column flanks in the same process, bit-exact against the oracle first.

    python3 scripts/long_read_probe.py [reps]

Cells are the oracle's count (the cells ksw_extend2 computes inside the trimmed [beg,end) of every row); time is the device time of
the whole bmh_extend_batch[_long] call (prefilter, job sort and class kernels: bmh_extend_last_ms), best of `reps`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bwa-mem_gpu_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def flanks(rng, n, qlo, qhi, sub=0.02, indel=0.002):
    """query = the start of the target with substitutions and short indels; target = query span + 100 (a seed's flank window)"""
    qs, ts = [], []
    for _ in range(n):
        ql = int(rng.integers(qlo, qhi + 1))
        t = rng.integers(0, 4, size=ql + 200).astype(np.uint8)
        src = np.arange(ql)
        cut = np.flatnonzero(rng.random(ql) < indel)
        for c in cut:
            src[c:] += int(rng.integers(-3, 4))
        src = np.clip(src, 0, len(t) - 1)
        q = t[src].copy()
        m = rng.random(ql) < sub
        q[m] = (q[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
        qs.append(q); ts.append(t[:ql + 100])
    qlen = np.array([len(x) for x in qs], np.uint32); tlen = np.array([len(x) for x in ts], np.uint32)
    qoff = np.concatenate([[0], np.cumsum(qlen)[:-1]]).astype(np.uint32)
    toff = np.concatenate([[0], np.cumsum(tlen)[:-1]]).astype(np.uint32)
    h0 = rng.integers(20, 60, size=n).astype(np.uint32)
    return np.concatenate(qs), qoff, qlen, np.concatenate(ts), toff, tlen, h0


def main():
    import torch
    import bwamem_hip as B
    import oracle_py
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = B.load_library()
    orc = oracle_py.Oracle()
    rng = np.random.default_rng(5)
    cases = [("wide<12> 705..768", 8192, 705, 768, False), ("long 1000", 4096, 990, 1010, True),
             ("long 2500", 1024, 2490, 2510, True), ("long 8000", 256, 7990, 8010, True), ("long 12000", 64, 11990, 12010, True)]
    print(f"{'case':22s} {'jobs':>6s} {'Gcells':>8s} {'ms':>8s} {'Gcells/s':>9s}")
    for name, n, lo, hi, lng in cases:
        jobs = flanks(rng, n, lo, hi)
        want3, want6, cells = orc.extend_batch(*jobs, n_threads=16, want_raw=True)
        d = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x)).cuda() for x in jobs]
        out = torch.zeros(n, 3, dtype=torch.int32, device="cuda"); raw = torch.zeros(n, 6, dtype=torch.int32, device="cuda")
        B.extend_batch(*d, out, raw_t=raw, long_queries=lng)
        torch.cuda.synchronize()
        assert L.bmh_extend_last_unsupported() == 0
        assert np.array_equal(out.cpu().numpy(), want3) and np.array_equal(raw.cpu().numpy(), want6), name
        best = 1e30
        for _ in range(reps):
            B.extend_batch(*d, out, long_queries=lng)      # the production form: three results, no raw tuple
            torch.cuda.synchronize()
            best = min(best, L.bmh_extend_last_ms())
        print(f"{name:22s} {n:6d} {cells / 1e9:8.3f} {best:8.2f} {cells / best / 1e6:9.2f}")
    # what the long entry costs a batch without a long query: the five long classes are launched and find their lists empty
    import common
    jobs = common.make_ext_jobs_fast(200_000, rng, maxq=281)
    d = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x)).cuda() for x in jobs]
    out = torch.zeros(len(jobs[2]), 3, dtype=torch.int32, device="cuda")
    for lng in (False, True, False, True):
        t = []
        for _ in range(reps):
            B.extend_batch(*d, out, long_queries=lng)
            torch.cuda.synchronize()
            t.append(L.bmh_extend_last_ms())
        print(f"200 000 jobs of <= 281 bases, long_queries={lng!s:5s}: best {min(t):.3f} ms, median {sorted(t)[len(t) // 2]:.3f} ms")


if __name__ == "__main__":
    main()
