#!/usr/bin/env python
"""What `python -m bwamem_hip.bam --markdup --collate` costs (BDP_TPL_FILE): --pairs synthetic FR pairs (two 100-base records each, distinct names,
drawn from --positions positions of one contig so that many are duplicates) as a name-grouped BAM and as the coordinate-sorted BAM of the same records, through
bam_post_file on the device: records per second of --markdup on the name-grouped file with the option off and on, and of --markdup --collate on the sorted file
with the library's own split into batches, grouping and merge (BMH_ALIGNER_TRACE).  Medians of --runs runs after a warm-up, with their spreads.  With
--parent-json FILE ... (this script's outputs under BMH_LIB=<the parent commit's library> with --parent, same visit, one taken before and one after) the option-off
row is compared with each of the parent's.
Writes profiles/bam_post_collate.json (or --out).

    python scripts/bam_post_collate_rate.py [--pairs 1000000] [--runs 3] [--parent] [--parent-json FILE ...] [--out FILE]
"""
import argparse
import io
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bwa-mem_gpu_amd"))
import numpy as np


def records(n_pairs: int, positions: int, seed: int = 1):
    """(the records of n_pairs FR pairs as one uint8 matrix, one row per record in name-grouped order, their sort keys)"""
    rng = np.random.default_rng(seed)
    L, name_w = 100, 10
    size = 36 + name_w + 1 + 4 + L // 2 + L
    R = np.zeros((2 * n_pairs, size), np.uint8)
    pos1 = (1000 + 150 * rng.integers(0, positions, n_pairs)).astype(np.int32)
    pos = np.stack([pos1, pos1 + 250], 1).reshape(-1)
    flag = np.tile(np.array([0x1 | 0x40 | 0x20, 0x1 | 0x80 | 0x10], np.uint16), n_pairs)

    def put(col, v, dt):
        R[:, col:col + np.dtype(dt).itemsize] = np.ascontiguousarray(v.astype(dt)).view(np.uint8).reshape(len(v), -1)
    put(0, np.full(2 * n_pairs, size - 4), "<u4"); put(4, np.zeros(2 * n_pairs), "<i4"); put(8, pos, "<i4")
    R[:, 12] = name_w + 1; R[:, 13] = 60
    put(14, 4681 + (pos >> 14), "<u2"); put(16, np.ones(2 * n_pairs), "<u2"); put(18, flag, "<u2"); put(20, np.full(2 * n_pairs, L), "<u4")
    put(24, np.zeros(2 * n_pairs), "<i4"); put(28, np.stack([pos1 + 250, pos1], 1).reshape(-1), "<i4")
    names = np.frombuffer("".join(np.char.zfill((np.arange(2 * n_pairs) // 2).astype(str), name_w - 1).tolist()).encode(), np.uint8).reshape(2 * n_pairs, name_w - 1)
    R[:, 36] = ord("p"); R[:, 37:36 + name_w] = names
    put(36 + name_w + 1, np.full(2 * n_pairs, L << 4), "<u4")
    q0 = 36 + name_w + 1 + 4 + L // 2
    R[:, q0 - L // 2:q0] = rng.integers(0, 256, (2 * n_pairs, L // 2), dtype=np.uint8) & 0x77 | 0x11
    R[:, q0:] = rng.integers(10, 41, (2 * n_pairs, 1), dtype=np.uint8)
    key = (pos.astype(np.int64) + 1) << 1 | (flag >> 4 & 1)
    return R, key


def write_bam(path, stream: bytes):
    from bwamem_hip.lib import bam_header, bgzf_compress, bgzf_eof
    with open(path, "wb") as f:
        f.write(bgzf_compress(bam_header("@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:c\tLN:400000000\n", [("c", 400_000_000)]), 1, host=True))
        step = 16 << 20
        for a in range(0, len(stream), step):
            f.write(bgzf_compress(stream[a:a + step], 1, host=False))
        f.write(bgzf_eof())


class Counter(io.RawIOBase):
    mode = "wb"

    def __init__(self):
        self.n = 0

    def write(self, b):
        self.n += len(b)
        return len(b)


def timed(path, runs, n_rec, **kw):
    from bwamem_hip.bam import bam_post_file
    secs, splits, counts = [], [], None
    for it in range(runs + 1):
        err = tempfile.TemporaryFile()
        saved = os.dup(2)
        sys.stderr.flush(); os.dup2(err.fileno(), 2)
        try:
            t0 = time.perf_counter()
            r = bam_post_file(path, Counter(), markdup=True, **kw)
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2); os.close(saved)
        err.seek(0)
        m = re.search(rb"sorted in ([0-9.]+) ms, templates by name over the file in ([0-9.]+) ms, merged in ([0-9.]+) ms", err.read())
        if it:
            secs.append(dt)
            if m:
                splits.append([float(x) for x in m.groups()])
        counts = r["markdup"]
    med = sorted(secs)[len(secs) // 2]
    row = {"unit": "Mrecords/s", "median": round(n_rec / med / 1e6, 3), "runs": [round(n_rec / s / 1e6, 3) for s in secs], "spread_pct": round(100 * (max(secs) - min(secs)) / med, 1),
           "seconds": [round(s, 3) for s in secs], "duplicate_pairs": counts["duplicate_pairs"], "pairs_examined": counts["pairs_examined"]}
    if splits:
        row["split_ms"] = {k: {"median": sorted(s[i] for s in splits)[len(splits) // 2], "runs": [s[i] for s in splits]} for i, k in enumerate(("batches", "grouping", "merge"))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--positions", type=int, default=400_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent", action="store_true", help="the library is the parent commit's (BMH_LIB): only the option-off row is run")
    ap.add_argument("--parent-json", nargs="*", default=[], help="the parent's outputs of the same visit, taken before and after this run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import bwamem_hip as B
    torch.cuda.set_device(0)
    B.load_library()
    os.environ["BMH_ALIGNER_TRACE"] = "1"
    R, key = records(a.pairs, a.positions)
    n_rec = len(R)
    tmp = tempfile.mkdtemp(prefix="bmh_post_collate_")
    grouped, srt = os.path.join(tmp, "grouped.bam"), os.path.join(tmp, "sorted.bam")
    write_bam(grouped, R.tobytes())
    result = {"pairs": a.pairs, "records": n_rec, "record_bytes": int(R.shape[1]), "positions": a.positions, "runs": a.runs, "library": os.environ.get("BMH_LIB", "this commit's"), "rows": {}}
    result["rows"]["name_grouped_markdup"] = timed(grouped, a.runs, n_rec)
    if not a.parent:
        write_bam(srt, R[np.argsort(key, kind="stable")].tobytes())
        result["rows"]["name_grouped_markdup_collate"] = timed(grouped, a.runs, n_rec, collate=True)
        result["rows"]["coordinate_sorted_markdup_collate"] = timed(srt, a.runs, n_rec, collate=True)
        off, on = result["rows"]["name_grouped_markdup"], result["rows"]["name_grouped_markdup_collate"]
        assert on["duplicate_pairs"] == off["duplicate_pairs"] == result["rows"]["coordinate_sorted_markdup_collate"]["duplicate_pairs"]
        result["option_cost_pct"] = round(100 * (off["median"] / on["median"] - 1), 1)
        os.remove(srt)
    result["parent_rows"], result["option_off_vs_parent"] = [], []
    for pj in a.parent_json:
        with open(pj) as f:
            parent = json.load(f)
        pr, tr = parent["rows"]["name_grouped_markdup"], result["rows"]["name_grouped_markdup"]
        diff = 100 * abs(tr["median"] - pr["median"]) / pr["median"]
        result["parent_rows"].append(pr)
        result["option_off_vs_parent"].append({"difference_pct": round(diff, 1), "larger_spread_pct": max(tr["spread_pct"], pr["spread_pct"]), "within_spread": diff <= max(tr["spread_pct"], pr["spread_pct"])})
    result["not_measured"] = "real files (names of 30 to 40 bytes, tags), spilled runs, SAM text, files beyond one batch of 256 MiB per 1.3 M records, the host form"
    os.remove(grouped); os.rmdir(tmp)
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_post_collate.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
