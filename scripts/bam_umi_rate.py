#!/usr/bin/env python
"""What barcode-aware duplicate keys cost in the decision: bam_sorted_file(markdup=True) on one synthetic record stream of a million templates --
500 000 FR pairs on 125 000 keys and 500 000 fragments on 250 000 ends, every first record with one of four RX:Z barcodes -- without and with barcode_tag="RX".
The decision's milliseconds are the library's own (the BMH_ALIGNER_TRACE line of the merge: a host clock around bdp_decide_device, which ends in a stream
synchronise), read from the standard error of one child process per leg; the legs alternate, each runs --warmup calls and then --runs timed ones.

    python scripts/bam_umi_rate.py [--runs 7] [--warmup 2] [--rounds 2] [--templates 1000000] [--parent DIR] [--edits N] [--out FILE]

--parent DIR: the bwa-mem_gpu_amd directory of another build of the library (the parent commit's, built beside this one): its leg without the option runs in
turn with this build's two legs.  Writes profiles/bam_markdup_umi.json (or --out).
--edits N: what grouping the barcodes within N mismatches costs instead -- the legs are barcode_tag="RX" alone (on --parent's build too) and with barcode_edits=N;
two of the stream's four barcodes are one mismatch apart.  Writes profiles/bam_markdup_umi_edits.json (or --out)."""
import argparse
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def stream(n_tpl: int):
    """the records, built as one numpy array per kind (no Python loop over records)"""
    import numpy as np
    rec = np.dtype([("block_size", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_ops", "<u2"), ("flag", "<u2"), ("l_seq", "<u4"),
                    ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "u1", 9), ("cigar", "<u4"), ("seq", "u1", 10), ("qual", "u1", 20), ("tag", "u1", 12)])
    assert rec.itemsize == 91
    rng = np.random.default_rng(1)
    n_pair = n_tpl // 2
    n_frag = n_tpl - n_pair
    umis = np.frombuffer(b"ACGTACGTACGTACGATTGACAGGACGTTTTT", np.uint8).reshape(4, 8)

    def make(tpl, pos, flag):
        r = np.zeros(len(tpl), rec)
        r["block_size"] = rec.itemsize - 4; r["ref"] = 0; r["pos"] = pos; r["l_name"] = 9; r["mapq"] = 30; r["n_ops"] = 1; r["flag"] = flag; r["l_seq"] = 20
        r["next_ref"] = -1; r["next_pos"] = -1; r["cigar"] = 20 << 4; r["seq"] = 0x12; r["qual"] = 30
        beg, end = pos.astype(np.int64), pos.astype(np.int64) + 19
        b = np.zeros(len(tpl), np.int64)
        for sh, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
            b = np.where(beg >> sh == end >> sh, base + (beg >> sh), b)
        r["bin"] = b
        for k in range(8):
            r["name"][:, k] = 48 + (tpl // 10 ** (7 - k)) % 10
        r["tag"][:, 0:3] = np.frombuffer(b"RXZ", np.uint8)
        r["tag"][:, 3:11] = umis[(tpl * 2654435761 >> 7) % 4]
        return r
    t = np.arange(n_pair, dtype=np.int64)
    p = 100 + 1000 * rng.integers(0, max(1, n_pair // 4), n_pair)
    pairs = np.empty(2 * n_pair, rec)
    pairs[0::2] = make(t, p, 0x61)
    pairs[1::2] = make(t, p + 200, 0x91)
    f = np.arange(n_pair, n_pair + n_frag, dtype=np.int64)
    frags = make(f, 100 + 1000 * rng.integers(0, max(1, n_frag // 2), n_frag), 0)
    return pairs.tobytes() + frags.tobytes(), int(max(p.max(), frags["pos"].max())) + 1000


def child(a):
    sys.path.insert(0, a.package)
    from bwamem_hip.lib import bam_sorted_file
    s, length = stream(a.templates)
    kw = dict(barcode_tag="RX") if a.leg == "tag" else dict(barcode_tag="RX", barcode_edits=a.edits) if a.leg == "edits" else {}
    for k in range(a.warmup + a.runs):
        sys.stderr.write("[run] %s\n" % ("warm-up" if k < a.warmup else "timed")); sys.stderr.flush()
        _bam, _bai, counts = bam_sorted_file("@HD\tVN:1.6\tSO:coordinate\n", [("c1", length)], s, 1, 0, markdup=True, **kw)
    print(json.dumps(counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--templates", type=int, default=1_000_000)
    ap.add_argument("--parent", default="")
    ap.add_argument("--edits", type=int, default=-1)
    ap.add_argument("--out", default="")
    ap.add_argument("--leg", default="")
    ap.add_argument("--package", default=os.path.join(HERE, "..", "bwa-mem_gpu_amd"))
    a = ap.parse_args()
    if a.leg:
        return child(a)
    a.out = a.out or os.path.join(HERE, "..", "profiles", "bam_markdup_umi_edits.json" if a.edits >= 0 else "bam_markdup_umi.json")
    legs = ([("parent, option off", a.parent, "off")] if a.parent else []) + [("this commit, option off", a.package, "off"), ("this commit, barcode_tag", a.package, "tag")]
    if a.edits >= 0:
        legs = ([("parent, barcode_tag", a.parent, "tag")] if a.parent else []) + [("this commit, barcode_tag", a.package, "tag"), ("this commit, barcode_edits=%d" % a.edits, a.package, "edits")]
    res = {name: {"decision_ms": [], "counts": None} for name, _p, _l in legs}
    for _round in range(a.rounds):
        for name, package, leg in legs:                               # (one process at a time holds the device)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--package", package, "--runs", str(a.runs), "--warmup", str(a.warmup), "--templates", str(a.templates), "--edits", str(a.edits)],
                               env=dict(os.environ, BMH_ALIGNER_TRACE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr.decode(errors="replace")[-2000:])
                return 1
            timed, ms = False, []
            for line in r.stderr.decode(errors="replace").split("\n"):
                if line.startswith("[run]"):
                    timed = line.endswith("timed")
                m = re.search(r"decided in ([0-9.]+) ms", line)
                if m and timed:
                    ms.append(float(m.group(1)))
            assert len(ms) == a.runs, (name, len(ms))
            res[name]["decision_ms"].append(ms)
            res[name]["counts"] = json.loads(r.stdout.decode().strip().split("\n")[-1])
    for name, v in res.items():
        flat = sorted(x for ms in v["decision_ms"] for x in ms)
        v["median_ms"] = flat[len(flat) // 2]
        v["spread_pct"] = round(100 * (flat[-1] - flat[0]) / v["median_ms"], 1)
        v["process_medians_ms"] = [sorted(ms)[len(ms) // 2] for ms in v["decision_ms"]]
        print(name, v["median_ms"], "ms, spread", v["spread_pct"], "%, per process", v["process_medians_ms"], v["counts"])
    with open(a.out, "w") as f:
        json.dump(dict({"templates": a.templates, "runs": a.runs, "warmup": a.warmup, "rounds": a.rounds}, **({"edits": a.edits} if a.edits >= 0 else {}), legs=res), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
