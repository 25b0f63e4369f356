#!/usr/bin/env python
"""What BAM output costs: reads -> SAM text (the yardstick: the path before BAM output existed), reads -> BAM at level 0 and level 1, the two kernels alone,
bytes out per read, and the level-1 size against zlib level 1 on the same 0xff00-byte pieces -- on the bench's index and read set, in one process, medians of
--runs runs with their spreads.  Writes profiles/bam_output.json (or --out).

    python scripts/bam_output_rate.py [--runs 3] [--reads 1000000] [--genome-mbp 3100] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bwa-mem_gpu_amd"))
import numpy as np
import torch

import bwamem_hip as B
from bwamem_hip import fmindex as F
from bwamem_hip.lib import BamOut, ChainOpt, ExtParams, NativeAligner, PeOpt, PostOpt, _contig_table


def stats(secs, unit_count, scale):
    med = sorted(secs)[len(secs) // 2]
    return {"median": round(unit_count / med / scale, 3), "runs": [round(unit_count / s / scale, 3) for s in secs], "spread_pct": round(100 * (max(secs) - min(secs)) / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=3100)
    ap.add_argument("--reads", type=int, default=1_000_000, help="reads per distinct batch; a run takes four times as many")
    ap.add_argument("--runs", type=int, default=3)
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
    nth = int(L.bmh_effective_cpus())
    co = ChainOpt(); L.bmh_chain_opt_default(C.byref(co))
    po = PostOpt(); L.bmh_post_opt_default(C.byref(po))
    pe_o = PeOpt(); L.bmh_pe_opt_default(C.byref(pe_o))
    rl, n = 150, a.reads
    r1 = B.synth.make_reads(g, n, rl, seed=7, holes=holes)[0]; r2 = B.synth.make_reads(g, n, rl, seed=1007, holes=holes)[0]
    asc = B.synth.codes_to_ascii(np.concatenate([r1.reshape(-1), r2.reshape(-1), r1.reshape(-1), r2.reshape(-1)]))
    n4 = 4 * n
    w = len(str(n4))
    names = np.frombuffer("".join(np.char.add(">r", np.char.zfill(np.arange(n4).astype(str), w)).tolist()).encode(), np.uint8).reshape(n4, w + 2)
    recs = np.empty((n4, w + 3 + rl + 1), np.uint8)
    recs[:, :w + 2] = names; recs[:, w + 2] = 10; recs[:, w + 3:w + 3 + rl] = asc.reshape(n4, rl); recs[:, -1] = 10
    tmp = tempfile.mkdtemp(prefix="bmh_bam_output_")
    path = os.path.join(tmp, "se.fa")
    recs.tofile(path)
    del recs
    nat = NativeAligner(dindex, pac_h, n_genome, contigs, None, co, ExtParams.default(), po, pe_o)
    result = {"genome_mbp": a.genome_mbp, "reads_per_run": n4, "setup_s": round(time.time() - t0, 1), "runs": a.runs, "host_threads": nth, "rows": {}}
    keep = []

    def run(fmt, level, keep_text=False):
        nat.set_output(fmt, level)
        nbytes = [0]

        def sink(mv):
            nbytes[0] += len(mv)
            if keep_text and len(keep) < 1:
                keep.append(bytes(mv))
        secs = []
        for it in range(a.runs + 1):
            nbytes[0] = 0
            t1 = time.perf_counter()
            nat.run_file(path, False, sink, batch_reads=n4 // 4, n_lanes=2, n_threads=nth)
            if it:
                secs.append(time.perf_counter() - t1)
        row = stats(secs, n4, 1e6)
        row["unit"] = "Mreads/s"; row["bytes_out_per_read"] = round(nbytes[0] / n4, 1)
        return row
    result["rows"]["reads_to_sam_text"] = run("sam", 1, keep_text=True)
    result["rows"]["reads_to_bam_level0"] = run("bam", 0)
    result["rows"]["reads_to_bam_level1"] = run("bam", 1)
    nat.set_output("sam", 1)
    # ---- the two kernels alone, on the first batch's text
    text = keep[0]
    blob, off = _contig_table(contigs)
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
    d_blob, d_off = torch.from_numpy(blob).to(dev), torch.from_numpy(off.view(np.int32).copy()).to(dev)
    L.bmh_bam_ws_create.restype = C.c_void_p
    L.bmh_bam_ws_free.argtypes = [C.c_void_p]
    L.bmh_sam_to_bam_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BamOut)]
    L.bmh_bgzf_deflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    ws = L.bmh_bam_ws_create()
    o = BamOut()
    secs = []
    for it in range(a.runs + 1):
        torch.cuda.synchronize(); t1 = time.perf_counter()
        assert L.bmh_sam_to_bam_device(ws, d_text.data_ptr(), len(text), len(contigs), d_blob.data_ptr(), d_off.data_ptr(), None, C.byref(o)) == 0
        torch.cuda.synchronize()
        if it:
            secs.append(time.perf_counter() - t1)
    assert o.n_refused == 0
    row = stats(secs, len(text), 1e9); row["unit"] = "GB/s of SAM text (the entry point: kernels, scans and its two waits)"; row["text_bytes"] = len(text); row["bam_bytes"] = int(o.bam_bytes)
    result["rows"]["sam_to_bam_device"] = row
    bam = torch.empty(int(o.bam_bytes), dtype=torch.uint8, device=dev)
    from bwamem_hip.lib import _memcpy_d2d
    _memcpy_d2d(bam.data_ptr(), o.d_bam, int(o.bam_bytes))
    for level in (0, 1):
        out, nb = C.c_void_p(), C.c_uint64()
        secs = []
        for it in range(a.runs + 1):
            torch.cuda.synchronize(); t1 = time.perf_counter()
            assert L.bmh_bgzf_deflate_device(ws, bam.data_ptr(), int(o.bam_bytes), level, None, C.byref(out), C.byref(nb)) == 0
            torch.cuda.synchronize()
            if it:
                secs.append(time.perf_counter() - t1)
        row = stats(secs, int(o.bam_bytes), 1e9); row["unit"] = "GB/s of BAM bytes (the entry point)"; row["members_bytes"] = int(nb.value)
        result["rows"][f"bgzf_deflate_device_level{level}"] = row
    # ---- level-1 size against zlib level 1 on the same pieces (the first 64 MiB)
    bam_h = bam[:64 << 20].cpu().numpy().tobytes()
    from bwamem_hip.lib import bgzf_compress
    ours = len(bgzf_compress(bam_h, 1))
    zl = 0
    for p in range(0, len(bam_h), 0xff00):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        zl += len(c.compress(bam_h[p:p + 0xff00]) + c.flush()) + 26
    result["rows"]["level1_size_vs_zlib1"] = {"input_bytes": len(bam_h), "ours_bytes": ours, "zlib1_bytes": zl, "ratio": round(ours / zl, 3)}
    L.bmh_bam_ws_free(ws)
    os.remove(path); os.rmdir(tmp)
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_output.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
