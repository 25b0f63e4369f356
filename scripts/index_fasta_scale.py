#!/usr/bin/env python3
"""Times `bwa index` on the device (bwamem_hip.index_fasta) on an hg38-like FASTA: synth.make_genome_device's genome in
24 contigs with 'N' in its holes, 60-column lines; once plain and, with --gz, once gzip-compressed (level 1).  Each run uses
--verify; the stats (read / H2D / pack / build / write seconds) and the peak HBM in use (device-wide, polled every 50 ms)
go to --out as JSON.   Usage: scripts/index_fasta_scale.py [--mbp 3100] [--gz] [--out FILE] [--dir DIR]"""
import argparse
import gzip
import json
import os
import shutil
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem_gpu_amd"))


def write_fasta(path, n_bases):
    import torch
    from bwamem_hip import synth
    g, meta = synth.make_genome_device(n_bases, "cuda:0", seed=1, return_meta=True)
    asc = synth.codes_to_ascii(g.cpu().numpy()).copy()
    del g
    torch.cuda.empty_cache()
    for a, b in meta["holes"]:
        asc[a:b] = ord("N")
    with open(path, "wb") as f:
        off = 0
        for name, ln in meta["contigs"]:
            f.write(b">" + name.encode() + b" hg38-like\n")
            s = asc[off:off + ln]
            w = 60
            body = s[: (ln // w) * w].reshape(-1, w)
            f.write(np.concatenate([body, np.full((body.shape[0], 1), 10, np.uint8)], axis=1).tobytes())
            if ln % w:
                f.write(s[(ln // w) * w:].tobytes() + b"\n")
            off += ln
    return int(sum(b - a for a, b in meta["holes"]))


def timed_index(fa, prefix):
    import torch
    import bwamem_hip as B
    free0, total = torch.cuda.mem_get_info()
    peak = [0]
    stop = threading.Event()

    def poll():
        while not stop.is_set():
            peak[0] = max(peak[0], total - torch.cuda.mem_get_info()[0])
            time.sleep(0.05)
    th = threading.Thread(target=poll, daemon=True)
    th.start()
    t0 = time.time()
    st = B.index_fasta(fa, prefix, sa_intv=16, verify=True)
    st["wall_seconds"] = time.time() - t0
    stop.set()
    th.join()
    st["peak_hbm_gb"] = round(peak[0] / 1e9, 2)
    st["hbm_in_use_before_gb"] = round((total - free0) / 1e9, 2)
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=3100)
    ap.add_argument("--gz", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default=None, help="scratch directory for the FASTA and the index [a temporary one]")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="ixscale")
    res = {"mbp": a.mbp}
    try:
        fa = os.path.join(d, "hg.fa")
        t0 = time.time()
        res["n_bases_in_holes"] = write_fasta(fa, int(a.mbp * 1e6))
        res["fasta_bytes"] = os.path.getsize(fa)
        res["make_fasta_seconds"] = round(time.time() - t0, 1)
        res["plain"] = timed_index(fa, os.path.join(d, "ix"))
        if a.gz:
            with open(fa, "rb") as fi, gzip.open(fa + ".gz", "wb", compresslevel=1) as fo:
                shutil.copyfileobj(fi, fo, 64 << 20)
            res["gz_bytes"] = os.path.getsize(fa + ".gz")
            res["gz"] = timed_index(fa + ".gz", os.path.join(d, "ixgz"))
            res["gz_files_equal_plain"] = all(open(os.path.join(d, "ix") + e, "rb").read() == open(os.path.join(d, "ixgz") + e, "rb").read()
                                              for e in (".bwt", ".sa", ".pac", ".ann", ".amb"))
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
