"""What re-seeding (gase_aln -g: BWA-MEM's second and third seeding rounds) costs on the hg38-scale workload of bench.py.

    python3 scripts/reseed_perf.py [--genome-mbp 3100] [--reads 1000000] [--out bench_out/reseed_perf.json]

The synthetic hg38-scale genome of bench.py (synth.make_genome_device, seed 42) and its FMD index (built on the device, sa_intv 1),
1 M 150 bp reads drawn from it (1 % substitutions), then:
  * bmh_seed_batch against bmh_seed_batch_reseed: ms per batch (median of 5 after a warm-up), seed groups per read of each round
    (round 2 alone: max_mem_intv = 0), and the fraction of reads whose seeds change;
  * reads -> SAM through the native pipeline (bmh_aligner_run, two lanes, four batches of the reads), without and with -g: Mreads/s
    (median of 3 after a warm-up) and the fraction of records whose MAPQ changes.
One JSON line on stdout.  Each run of it is one GPU step: the caller puts it under a time limit of its own."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem_gpu_amd"))

import bwamem_hip as B  # noqa: E402
from bwamem_hip import fmindex as F  # noqa: E402
from bwamem_hip.lib import ReseedOpt, seeds_to_host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=3100.0)
    ap.add_argument("--reads", type=int, default=1_000_000)
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
    d = F.build_fmd_index_device(pac_t, n_genome, sa_intv=1)
    dindex = B.Index.from_device(d.primary, d.L2.astype(np.uint64), d.seq_len, d.bwt_t, d.sa_intv, d.sa_t, d.bits_t, pac_t=pac_t, l_pac=n_genome)
    t_index = time.time() - t0
    # reads: uniform positions, either strand, 1 % substitutions (N-runs of the genome included, as they fall)
    rng = np.random.default_rng(7)
    n, rl = a.reads, 150
    pos = torch.from_numpy(rng.integers(0, n_genome - rl, size=n)).to(dev)
    g_codes = F.unpack_pac_device(pac_t, n_genome)
    reads = g_codes[pos[:, None] + torch.arange(rl, device=dev)[None, :]].cpu().numpy().astype(np.uint8)
    del g_codes
    torch.cuda.empty_cache()
    rev = rng.random(n) < 0.5
    rc = reads[rev][:, ::-1]
    reads[rev] = np.where(rc < 4, 3 - rc, 4)
    m = rng.random(reads.shape) < 0.01
    reads[m] = np.where(reads[m] < 4, (reads[m] + rng.integers(1, 4, size=int(m.sum()))) & 3, reads[m])
    flat = np.ascontiguousarray(reads.reshape(-1))
    asc = B.synth.codes_to_ascii(flat)
    r_t = torch.from_numpy(asc).to(dev)
    o_t = (torch.arange(n, dtype=torch.int32, device=dev) * rl)
    l_t = torch.full((n,), rl, dtype=torch.int32, device=dev)
    ws = B.SeedWorkspace(n, n * rl)

    def seed(opt):
        ms, s = [], None
        for it in range(6):
            torch.cuda.synchronize(); t = time.perf_counter()
            s = ws.seed_batch(dindex, r_t, o_t, l_t, 19, reseed=opt)
            torch.cuda.synchronize()
            if it:
                ms.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ms)), s
    ms_off, s_off = seed(None)
    h_off = seeds_to_host(s_off, n); g_off = int(s_off.n_smems)
    ms_r2, s_r2 = seed(ReseedOpt.default(enable=1, max_mem_intv=0))
    g_r2 = int(s_r2.n_smems)
    ms_on, s_on = seed(ReseedOpt.default(enable=1))
    h_on = seeds_to_host(s_on, n); g_on = int(s_on.n_smems)
    changed = int(np.count_nonzero(h_off["n_ref_pos"] != h_on["n_ref_pos"]))
    ws.free()

    # reads -> SAM, native pipeline, without and with -g
    from bwamem_hip.aligner import ReadSet
    from bwamem_hip.lib import ChainOpt, NativeAligner, PeOpt, PostOpt
    co = ChainOpt(); L.bmh_chain_opt_default(C.byref(co))
    po = PostOpt(); L.bmh_post_opt_default(C.byref(po))
    pe = PeOpt(); L.bmh_pe_opt_default(C.byref(pe))
    params = B.ExtParams.default()
    pac_h = np.ascontiguousarray(np.concatenate([pac_t.cpu().numpy(), np.zeros(2, np.uint8)]))
    contigs = [tuple(c) for c in meta["contigs"]]
    w = len(str(n))
    names = np.char.add("r", np.char.zfill(np.arange(n).astype(str), w))
    blob = np.frombuffer(("\0".join(names.tolist()) + "\0").encode(), dtype=np.uint8)
    rs = ReadSet(asc, np.arange(n, dtype=np.uint64) * np.uint64(rl), np.full(n, rl, np.uint32), blob, np.arange(n, dtype=np.uint64) * np.uint64(w + 2), codes=flat)
    cuts = [n * k // 4 for k in range(4)] + [n]
    nat = NativeAligner(dindex, pac_h, n_genome, contigs, None, co, params, po, pe)
    res = {}
    for tag, opt in (("off", None), ("g", ReseedOpt.default(enable=1))):
        nat.set_reseed(opt)
        secs, text = [], []
        for it in range(4):
            parts = []
            st = nat.run(rs, cuts, False, (lambda mv: parts.append(bytes(mv))) if it == 0 else (lambda mv: None), n_lanes=2, n_threads=0)
            if it == 0:
                text = b"".join(parts)
            else:
                secs.append(st.seconds)
        res[tag] = (n / float(np.median(secs)) / 1e6, text)
    mq = {}
    for tag in res:
        mq[tag] = [int(l.split(b"\t")[4]) for l in res[tag][1].split(b"\n") if l and not (int(l.split(b"\t")[1]) & 0x900)]
    mq_changed = sum(1 for x, y in zip(mq["off"], mq["g"]) if x != y)
    nat.free()
    row = {"genome_mbp": a.genome_mbp, "reads": n, "read_len": rl, "index_s": round(t_index, 1),
           "seed_ms_off": round(ms_off, 2), "seed_ms_reseed": round(ms_on, 2), "seed_ms_reseed_round2_only": round(ms_r2, 2),
           "groups_per_read_round1": round(g_off / n, 3), "groups_per_read_added_round2": round((g_r2 - g_off) / n, 3),
           "groups_per_read_added_round3": round((g_on - g_r2) / n, 3), "reads_with_changed_seeds": round(changed / n, 4),
           "sam_mreads_s_off": round(res["off"][0], 3), "sam_mreads_s_g": round(res["g"][0], 3), "records_with_changed_mapq": round(mq_changed / max(len(mq["off"]), 1), 4)}
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
