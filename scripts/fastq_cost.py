"""What FASTQ costs in reads -> SAM text: the native pipeline (bmh_aligner_run / bmh_aligner_run_file) on the bench's hg38-scale synthetic
genome and index (seed 42, bench.py's generator and builder), the bench's reads -> SAM row shape (four batches of a million 150 bp reads,
two distinct batches taken twice; two lanes single-end, four lanes and eight batches paired; letters in registered host memory), for
  * the reads without qualities (QUAL '*': the bench's row),
  * the same reads with qualities (QUAL written by the SAM kernels; the qualities registered too, as the letters),
  * the same reads from files in the page cache: FASTA (bmh_aligner_run_fasta) and FASTQ (bmh_aligner_run_file).
Every configuration runs once to warm the lanes, then --runs times; the JSON line lists every run, the median and the spread.

    python scripts/fastq_cost.py [--genome-mbp 3100] [--runs 3] [--paired] [--out profiles/fastq_cost.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem_gpu_amd"))
import numpy as np
import torch

import bwamem_hip as B
from bwamem_hip import fmindex as F
from bwamem_hip.aligner import ReadSet
from bwamem_hip.lib import ChainOpt, ExtParams, NativeAligner, PeOpt, PostOpt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=3100)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="se,pe")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = B.load_library()
    n_genome = int(a.genome_mbp * 1e6)
    t0 = time.time()
    g_t, meta = B.synth.make_genome_device(n_genome, dev, seed=42, return_meta=True)
    pac_t = F.pack_pac_device(g_t)
    del g_t
    torch.cuda.empty_cache()
    d = F.build_fmd_index_device(pac_t, n_genome, sa_intv=1, verify=False)
    dindex = B.Index.from_device(d.primary, d.L2.astype(np.uint64), d.seq_len, d.bwt_t, d.sa_intv, d.sa_t, d.bits_t, pac_t=pac_t, l_pac=n_genome)
    g = F.unpack_pac_device(pac_t, n_genome).cpu().numpy()
    pac_h = pac_t.cpu().numpy()
    contigs, holes = meta["contigs"], meta["holes"]
    t_setup = time.time() - t0
    nth = int(L.bmh_effective_cpus())
    co = ChainOpt(); L.bmh_chain_opt_default(C.byref(co))
    po = PostOpt(); L.bmh_post_opt_default(C.byref(po))
    pe_o = PeOpt(); L.bmh_pe_opt_default(C.byref(pe_o))
    params = ExtParams.default()
    L.bmh_host_pin.argtypes = [C.c_void_p, C.c_size_t]; L.bmh_host_unpin.argtypes = [C.c_void_p]
    rl = 150
    result = {"genome_mbp": a.genome_mbp, "setup_s": round(t_setup, 1), "runs": a.runs, "rows": {}}
    for mode in a.modes.split(","):
        paired = mode == "pe"
        n = a.reads
        if paired:
            r1 = B.synth.make_pairs(g, n // 2, rl, seed=7, holes=holes)[0]; r2 = B.synth.make_pairs(g, n // 2, rl, seed=1007, holes=holes)[0]
        else:
            r1 = B.synth.make_reads(g, n, rl, seed=7, holes=holes)[0]; r2 = B.synth.make_reads(g, n, rl, seed=1007, holes=holes)[0]
        flat4 = np.concatenate([r1.reshape(-1), r2.reshape(-1), r1.reshape(-1), r2.reshape(-1)])
        n4 = 4 * n
        asc = B.synth.codes_to_ascii(flat4)
        qual = np.random.default_rng(3).integers(33, 75, size=asc.size).astype(np.uint8)
        w = len(str(n4))
        names = np.char.add("r", np.char.zfill((np.arange(n4) // (2 if paired else 1)).astype(str), w))
        blob = np.frombuffer(("\0".join(names.tolist()) + "\0").encode(), dtype=np.uint8)
        noff = np.arange(n4, dtype=np.uint64) * np.uint64(w + 2)
        offs = np.arange(n4, dtype=np.uint64) * np.uint64(rl); lens = np.full(n4, rl, np.uint32)
        rs_plain = ReadSet(asc, offs, lens, blob, noff, codes=flat4)
        rs_qual = ReadSet(asc, offs, lens, blob, noff, codes=flat4, qual=qual)
        lanes = 4 if paired else 2
        nb4 = 8 if paired else 4
        cuts4 = [((n4 * k // nb4) & ~1) for k in range(nb4)] + [n4]
        nat = NativeAligner(dindex, pac_h, n_genome, contigs, None, co, params, po, pe_o)
        pinned = L.bmh_host_pin(asc.ctypes.data, asc.nbytes) == 0 and L.bmh_host_pin(qual.ctypes.data, qual.nbytes) == 0
        # the two files: the same reads, names and (FASTQ) qualities
        tmp = tempfile.gettempdir()
        fa, fq = os.path.join(tmp, "bmh_cost_%d.fa" % os.getpid()), os.path.join(tmp, "bmh_cost_%d.fq" % os.getpid())
        nm = np.frombuffer("".join(names.tolist()).encode(), np.uint8).reshape(n4, w + 1)
        recs = np.empty((n4, w + 3 + rl + 1), np.uint8)
        recs[:, 0] = ord(">"); recs[:, 1:w + 2] = nm; recs[:, w + 2] = 10; recs[:, w + 3:w + 3 + rl] = asc.reshape(n4, rl); recs[:, -1] = 10
        recs.tofile(fa)
        recs = np.empty((n4, w + 3 + rl + 3 + rl + 1), np.uint8)
        recs[:, 0] = ord("@"); recs[:, 1:w + 2] = nm; recs[:, w + 2] = 10; recs[:, w + 3:w + 3 + rl] = asc.reshape(n4, rl)
        recs[:, w + 3 + rl] = 10; recs[:, w + 4 + rl] = ord("+"); recs[:, w + 5 + rl] = 10; recs[:, w + 6 + rl:w + 6 + 2 * rl] = qual.reshape(n4, rl); recs[:, -1] = 10
        recs.tofile(fq); del recs
        bytes_out = [0]

        def sink(mv):
            bytes_out[0] += len(mv)
        configs = {
            "reads_to_sam_no_qual": lambda: nat.run(rs_plain, cuts4, paired, sink, n_lanes=lanes, n_threads=nth),
            "reads_to_sam_qual": lambda: nat.run(rs_qual, cuts4, paired, sink, n_lanes=lanes, n_threads=nth),
            "fasta_file_to_sam": lambda: nat.run_fasta(fa, paired, sink, batch_reads=(n4 // nb4) & ~1, n_lanes=lanes, n_threads=nth),
            "fastq_file_to_sam": lambda: nat.run_file(fq, paired, sink, batch_reads=(n4 // nb4) & ~1, n_lanes=lanes, n_threads=nth),
        }
        rows = {}
        for key, fn in configs.items():
            secs, st = [], None
            for it in range(a.runs + 1):
                bytes_out[0] = 0
                t0 = time.perf_counter()
                st = fn()
                dt = time.perf_counter() - t0
                if it:
                    secs.append(dt)
            med = sorted(secs)[len(secs) // 2]
            rows[key] = {"Mreads_per_s": round(n4 / med / 1e6, 2), "runs_Mreads_per_s": [round(n4 / s / 1e6, 2) for s in secs],
                         "spread_pct": round(100 * (max(secs) - min(secs)) / med, 1), "sam_bytes": int(bytes_out[0]),
                         "h2d_bytes": int(st.h2d_bytes), "d2h_bytes": int(st.d2h_bytes),
                         "h2d_copy_s": round(st.h2d_copy_seconds, 4), "d2h_copy_s": round(st.d2h_copy_seconds, 4)}
            print(mode, key, json.dumps(rows[key]), flush=True)
        os.remove(fa); os.remove(fq)
        if pinned:
            L.bmh_host_unpin(asc.ctypes.data); L.bmh_host_unpin(qual.ctypes.data)
        nat.free()
        result["rows"][mode] = dict(rows, reads=n4, lanes=lanes, batches=nb4, registered_host_memory=bool(pinned))
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
