"""What the read-input path costs in file -> SAM text: FASTQ files of 150 bp reads on the bench's hg38-scale synthetic genome and index
(scripts/fastq_cost.py's setup), single-end and paired, through
  * bmh_aligner_run_file on the plain interleaved file (the yardstick: the path that exists without csrc/reads_parse.hip) -- in this tree
    and, with --parent DIR, in a built tree of the parent commit (a child process with that tree's package and library, the same files),
  * bmh_aligner_run_files on the same plain file, on two plain files (paired), on BGZF and on single-member gzip,
  * bmh_aligner_run_files on the same reads as unaligned BAM (align_files_bam; --configs align_files_bgzf,align_files_bam gives the two rows to compare),
  * that BAM rewritten with four read groups -- @RG lines in its header, RG:Z on every record, the groups changing read by read (pairs: template by template) --
    once plain (align_files_bam_rg_plain: the tags are ignored, the code path of a run without the option) and once keeping its read groups
    (align_files_bam_keep_rg: bmh_aligner_set_keep_rg); --configs align_files_bam_rg_plain,align_files_bam_keep_rg --out FILE --out-key keep_rg adds the two rows
    to FILE under that key and leaves the rest of it as it is.
Every configuration runs once to warm the lanes, then --runs times; each row lists every run, the median, the spread, the host CPU
seconds of the process per million reads, and how many windows the device parser cut and how many the host walker took.

--parser-only times nothing else than the parser: it loads a FASTQ file of --reads reads through bmh_reads_load_files (64 MiB windows), for a
kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python scripts/reads_input_rate.py --parser-only).

--inflate-only times nothing else than the device inflate (csrc/inflate_kernels.hip): the BGZF members of a FASTQ text of --reads reads go up once, then the
kernel alone runs on the first 1024, 4096, 16384 ... and on all of them, several launches each (rocprofv3 --kernel-trace --stats -- python
scripts/reads_input_rate.py --inflate-only); beside it zlib on the same members on the host's threads, the yardstick, and the library's own host decoder.

--collate (paired mode) adds two rows: the aligner's own coordinate-sorted BAM of the run's pairs realigned with mates collated by name
(align_files_bam_sorted_collate: bmh_aligner_set_collate) beside the name-grouped BAM of the same pairs in the order the collation gives them
(align_files_bam_grouped: the code path of a run without the option); --modes pe --reads 500000 --collate --configs align_files_bam_grouped,align_files_bam_sorted_collate
is one million pairs.
--bam-only times nothing else than the BAM input path: the host's chain walk over the records alone, then loads of the BAM file for a kernel trace.

    python scripts/reads_input_rate.py [--genome-mbp 3100] [--reads 1000000] [--runs 3] [--modes se,pe] [--parent DIR] [--out profiles/reads_input.json]
"""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.environ.get("BMH_RATE_TREE") or ROOT, "bwa-mem_gpu_amd"))      # (--parent's child: the parent tree's package and library)
import numpy as np
import torch

import bwamem_hip as B
from bwamem_hip import fmindex as F
from bwamem_hip.lib import ChainOpt, ExtParams, NativeAligner, PeOpt, PostOpt


def _deflate_raw(data: bytes, level: int = 1) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def write_gzip(path: str, data: bytes) -> None:
    with open(path, "wb") as f:
        f.write(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + _deflate_raw(data) + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF))


def write_bgzf(path: str, data: bytes, block: int = 65280) -> None:
    with open(path, "wb") as f:
        for i in list(range(0, len(data), block)) + [None]:
            d = b"" if i is None else data[i:i + block]
            z = _deflate_raw(d)
            f.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(z) + 25) + z + struct.pack("<II", zlib.crc32(d) & 0xFFFFFFFF, len(d)))


def fastq_records(names: np.ndarray, w: int, asc: np.ndarray, qual: np.ndarray, rl: int) -> np.ndarray:
    n = asc.size // rl
    nm = np.frombuffer("".join(names.tolist()).encode(), np.uint8).reshape(n, w + 1)
    recs = np.empty((n, w + 3 + rl + 3 + rl + 1), np.uint8)
    recs[:, 0] = ord("@"); recs[:, 1:w + 2] = nm; recs[:, w + 2] = 10; recs[:, w + 3:w + 3 + rl] = asc.reshape(n, rl)
    recs[:, w + 3 + rl] = 10; recs[:, w + 4 + rl] = ord("+"); recs[:, w + 5 + rl] = 10; recs[:, w + 6 + rl:w + 6 + 2 * rl] = qual.reshape(n, rl); recs[:, -1] = 10
    return recs


NT16 = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    NT16[_c] = _i


def bam_records(names: np.ndarray, w: int, asc: np.ndarray, qual: np.ndarray, rl: int, paired: bool, n_groups: int = 0) -> np.ndarray:
    """the same reads as unaligned BAM records (one row each): flag 4, or 0x4D / 0x8D in turn for pairs; no CIGAR; no tags, or with n_groups (up to 10) the tag
    RG:Z:g<k>, k changing template by template"""
    n = asc.size // rl
    nm = np.frombuffer("".join(names.tolist()).encode(), np.uint8).reshape(n, w + 1)
    l_name, half = w + 2, (rl + 1) // 2
    bs = 32 + l_name + half + rl + (6 if n_groups else 0)
    rec = np.zeros((n, 4 + bs), np.uint8)
    if n_groups:
        rec[:, -6:-2] = np.frombuffer(b"RGZg", np.uint8)
        rec[:, -2] = ord("0") + (np.arange(n) // (2 if paired else 1)) % n_groups
    rec[:, 0:4] = np.frombuffer(struct.pack("<I", bs), np.uint8)
    rec[:, 4:12] = 0xff                                                          # refID, pos: -1
    rec[:, 12] = l_name
    rec[:, 14:16] = np.frombuffer(struct.pack("<H", 4680), np.uint8)
    rec[:, 18] = 4
    if paired:
        rec[0::2, 18] = 0x4D; rec[1::2, 18] = 0x8D
    rec[:, 20:24] = np.frombuffer(struct.pack("<I", rl), np.uint8)
    rec[:, 24:32] = 0xff                                                         # next_refID, next_pos: -1
    rec[:, 36:36 + w + 1] = nm
    nib = np.zeros((n, 2 * half), np.uint8); nib[:, :rl] = NT16[asc.reshape(n, rl)]
    s0 = 36 + l_name
    rec[:, s0:s0 + half] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    rec[:, s0 + half:s0 + half + rl] = qual.reshape(n, rl) - 33
    return rec


BAM_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
BAM_HEADER = b"BAM\1" + struct.pack("<I", len(BAM_TEXT)) + BAM_TEXT + struct.pack("<I", 0)      # no reference sequences: the reads are unaligned
BAM_RG_TEXT = BAM_TEXT + b"".join(b"@RG\tID:g%d\tLB:lib%d\tSM:s\n" % (k, k // 2) for k in range(4))      # four groups in two libraries
BAM_RG_HEADER = b"BAM\1" + struct.pack("<I", len(BAM_RG_TEXT)) + BAM_RG_TEXT + struct.pack("<I", 0)


def bgzf_members(blob: bytes):
    """the inflated text of every member of a BGZF stream whose members carry the BC field alone (what write_bgzf and the library write)"""
    p = 0
    while p < len(blob):
        size = struct.unpack_from("<H", blob, p + 16)[0] + 1
        yield zlib.decompress(blob[p + 18:p + size - 8], -15)
        p += size


def grouped_records(records: bytes) -> bytes:
    """--collate's definition over BAM records: the kept records of the pairs in the order in which their later record comes, the 0x40 record first"""
    open_, out, p = {}, [], 0
    while p < len(records):
        n = 4 + struct.unpack_from("<I", records, p)[0]
        flag = struct.unpack_from("<H", records, p + 18)[0]
        if not flag & 0x900:
            nm = records[p + 36:p + 36 + records[p + 12]]
            q = open_.pop(nm, None)
            if q is None:
                open_[nm] = (p, n)
            else:
                a, b = records[q[0]:q[0] + q[1]], records[p:p + n]
                out += [a, b] if flag & 0x80 else [b, a]
        p += n
    assert not open_, "the sorted BAM holds records without partner"
    return b"".join(out)


def measure(fn, runs: int, n4: int) -> dict:
    """fn once to warm, then `runs` times: median rate, every run, spread, host CPU seconds (user + system of the process) per million reads"""
    secs, cpus = [], []
    for it in range(runs + 1):
        c0 = os.times(); t1 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t1; c1 = os.times()
        if it:
            secs.append(dt); cpus.append((c1.user - c0.user) + (c1.system - c0.system))
    med = sorted(secs)[len(secs) // 2]
    return {"Mreads_per_s": round(n4 / med / 1e6, 2), "runs_Mreads_per_s": [round(n4 / s / 1e6, 2) for s in secs],
            "spread_pct": round(100 * (max(secs) - min(secs)) / med, 1), "host_cpu_s_per_Mreads": round(sorted(cpus)[len(cpus) // 2] / (n4 / 1e6), 3)}


def parser_only(a):
    from bwamem_hip.aligner import read_reads_files
    from bwamem_hip.lib import reads_last_counts
    B.load_library()
    n, rl = a.reads, 150
    rng = np.random.default_rng(1)
    asc = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * rl)]
    qual = rng.integers(33, 75, size=n * rl).astype(np.uint8)
    w = len(str(n))
    names = np.char.add("r", np.char.zfill(np.arange(n).astype(str), w))
    path = os.path.join(tempfile.gettempdir(), "bmh_parser_only_%d.fq" % os.getpid())
    fastq_records(names, w, asc, qual, rl).tofile(path)
    for it in range(3):
        t0 = time.perf_counter()
        rs = read_reads_files(path, comments=True)
        dt = time.perf_counter() - t0
        print(json.dumps({"reads": len(rs), "text_bytes": os.path.getsize(path), "load_s": round(dt, 3), "counts": reads_last_counts()}), flush=True)
    os.remove(path)


def bam_only(a):
    """nothing but the BAM input path: the host's chain walk over the records of --reads reads in memory, timed alone, then the file loaded through
    bmh_reads_load_files (64 MiB windows), for a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python scripts/reads_input_rate.py --bam-only)"""
    from bwamem_hip.aligner import read_reads_files
    from bwamem_hip.lib import reads_last_counts
    L = B.load_library()
    n, rl = a.reads, 150
    rng = np.random.default_rng(1)
    asc = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * rl)]
    qual = rng.integers(33, 75, size=n * rl).astype(np.uint8)
    w = len(str(n))
    names = np.char.add("r", np.char.zfill(np.arange(n).astype(str), w))
    records = bam_records(names, w, asc, qual, rl, False).tobytes()
    L.bmh_bam_chain_count.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    nr, end = C.c_uint64(), C.c_uint64()
    ms = []
    for it in range(4):
        t0 = time.perf_counter()
        assert L.bmh_bam_chain_count(records, len(records), C.byref(nr), C.byref(end)) == 0
        ms.append((time.perf_counter() - t0) * 1e3)
    assert nr.value == n and end.value == len(records)
    print(json.dumps({"chain_walk_ms": [round(x, 3) for x in ms], "records": n, "ms_per_Mrecords": round(sorted(ms[1:])[1] / (n / 1e6), 3)}), flush=True)
    path = os.path.join(tempfile.gettempdir(), "bmh_bam_only_%d.bam" % os.getpid())
    write_bgzf(path, BAM_HEADER + records)
    for it in range(3):
        t0 = time.perf_counter()
        rs = read_reads_files(path, comments=True)
        dt = time.perf_counter() - t0
        print(json.dumps({"reads": len(rs), "record_bytes": len(records), "file_bytes": os.path.getsize(path), "load_s": round(dt, 3), "counts": reads_last_counts()}), flush=True)
    os.remove(path)


def inflate_only(a):
    from concurrent.futures import ThreadPoolExecutor
    from bwamem_hip.lib import INFLATE_MEMBER, bgzf_scan, inflate_members
    L = B.load_library()
    nth = int(L.bmh_effective_cpus())
    n, rl = a.reads, 150
    rng = np.random.default_rng(1)
    asc = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * rl)]
    qual = rng.integers(33, 75, size=n * rl).astype(np.uint8)
    w = len(str(n))
    names = np.char.add("r", np.char.zfill(np.arange(n).astype(str), w))
    text = fastq_records(names, w, asc, qual, rl).tobytes()
    block = 65280

    def member(i):
        d = text[i:i + block]
        z = _deflate_raw(d)
        return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(z) + 25) + z + struct.pack("<II", zlib.crc32(d) & 0xFFFFFFFF, len(d))
    with ThreadPoolExecutor(nth) as ex:
        data = b"".join(ex.map(member, range(0, len(text), block)))
    tab, used, nbytes = bgzf_scan(data)
    assert used == len(data) and nbytes == len(text)
    res = {"reads": n, "text_bytes": nbytes, "compressed_bytes": len(data), "members": len(tab), "host_threads": nth, "launches": []}
    # the yardstick: zlib (inflate and crc32, what the host path runs per member) on the host's threads
    raws = [data[int(e["in_off"]):int(e["in_off"]) + int(e["in_len"])] for e in tab]

    def z_one(k):
        t = zlib.decompress(raws[k], -15)
        return zlib.crc32(t) == int(tab["crc32"][k])
    secs = []
    with ThreadPoolExecutor(nth) as ex:
        for _ in range(3):
            t0 = time.perf_counter(); ok = all(ex.map(z_one, range(len(tab)), chunksize=16)); secs.append(time.perf_counter() - t0)
            assert ok
    res["zlib_host_GBps"] = round(nbytes / sorted(secs)[1] / 1e9, 2)
    t0 = time.perf_counter(); out, st = inflate_members(data, tab, nbytes, host=True); dt = time.perf_counter() - t0
    assert not st.any() and out.tobytes() == text
    res["own_decoder_host_GBps"] = round(nbytes / dt / 1e9, 2)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_tab = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(len(tab), dtype=torch.int32, device="cuda")
    L.bmh_inflate_members_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    sizes = sorted({min(k, len(tab)) for k in (1024, 4096, 8192, 16384, 32768, len(tab))})
    for k in sizes:
        tb = int(tab["isize"][:k].sum())
        ms = []
        for it in range(a.runs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = L.bmh_inflate_members_device(d_in.data_ptr(), len(data), d_tab.data_ptr(), k, d_out.data_ptr(), nbytes, d_st.data_ptr(), stream)
            e1.record(); torch.cuda.synchronize()
            assert rc == 0
            if it:
                ms.append(e0.elapsed_time(e1))
        assert not d_st[:k].any().item()
        med = sorted(ms)[len(ms) // 2]
        res["launches"].append({"members": k, "text_bytes": tb, "ms": [round(x, 3) for x in ms], "text_GBps": round(tb / med / 1e6, 2)})
        print(json.dumps(res["launches"][-1]), flush=True)
    assert d_out[:nbytes].cpu().numpy().tobytes() == text
    res["device_over_zlib_host"] = round(res["launches"][-1]["text_GBps"] / res["zlib_host_GBps"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=3100)
    ap.add_argument("--reads", type=int, default=1_000_000, help="reads per distinct batch; a run takes four times as many")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="se,pe")
    ap.add_argument("--out", default="")
    ap.add_argument("--parent", default="", help="a built tree of the parent commit: its align_file on the same plain file, in a child process")
    ap.add_argument("--parser-only", action="store_true")
    ap.add_argument("--inflate-only", action="store_true")
    ap.add_argument("--bam-only", action="store_true")
    ap.add_argument("--collate", action="store_true", help="paired mode: the rows align_files_bam_grouped and align_files_bam_sorted_collate")
    ap.add_argument("--configs", default="", help="only these rows (comma-separated keys, e.g. align_files_bgzf,align_files_bam); default: all")
    ap.add_argument("--out-key", default="", help="with --out: the result goes into the existing JSON of that file under this key; the rest of the file stays")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)          # the plain file the --parent child aligns (mode and sizes from the other options)
    a = ap.parse_args()
    if a.parser_only:
        return parser_only(a)
    if a.inflate_only:
        return inflate_only(a)
    if a.bam_only:
        return bam_only(a)
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
    params = ExtParams.default()
    rl = 150
    result = {"genome_mbp": a.genome_mbp, "setup_s": round(time.time() - t0, 1), "runs": a.runs, "host_threads": nth, "rows": {}}
    tmp = tempfile.mkdtemp(prefix="bmh_reads_input_")
    if a.child:                                                # the --parent child: the yardstick alone, on the file the parent process wrote
        paired = a.modes == "pe"
        n4 = 4 * a.reads
        lanes, nb4 = (4, 8) if paired else (2, 4)
        nat = NativeAligner(dindex, pac_h, n_genome, contigs, None, co, params, po, pe_o)
        os.rmdir(tmp)
        print("CHILD " + json.dumps(measure(lambda: nat.run_file(a.child, paired, lambda mv: None, batch_reads=(n4 // nb4) & ~1, n_lanes=lanes, n_threads=nth), a.runs, n4)), flush=True)
        return
    from bwamem_hip.lib import reads_last_counts
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
        recs = fastq_records(names, w, asc, qual, rl)
        p = lambda s: os.path.join(tmp, mode + "." + s)  # noqa: E731
        recs.tofile(p("fq"))
        only = set(a.configs.split(",")) if a.configs else None
        write_bgzf(p("fq.bgzf"), recs.tobytes())
        if only is None or any("gzip" in k for k in only):
            write_gzip(p("fq.gz"), recs.tobytes())
        write_bgzf(p("bam"), BAM_HEADER + bam_records(names, w, asc, qual, rl, paired).tobytes())       # the same reads as unaligned BAM: half the bytes, no lines
        if only is None or any("_rg" in k for k in only):
            write_bgzf(p("rg.bam"), BAM_RG_HEADER + bam_records(names, w, asc, qual, rl, paired, 4).tobytes())
        if paired and (only is None or any("two" in k for k in only)):
            recs[0::2].tofile(p("r1.fq")); recs[1::2].tofile(p("r2.fq"))
            write_bgzf(p("r1.bgzf"), recs[0::2].tobytes()); write_bgzf(p("r2.bgzf"), recs[1::2].tobytes())
            write_gzip(p("r1.gz"), recs[0::2].tobytes()); write_gzip(p("r2.gz"), recs[1::2].tobytes())
        del recs
        lanes, nb4 = (4, 8) if paired else (2, 4)
        br = (n4 // nb4) & ~1
        nat = NativeAligner(dindex, pac_h, n_genome, contigs, None, co, params, po, pe_o)
        bytes_out = [0]

        def sink(mv):
            bytes_out[0] += len(mv)
        kw = dict(batch_reads=br, n_lanes=lanes, n_threads=nth)

        def device_inflate(fn):                # BMH_INFLATE_DEVICE=1 for one call; without it BGZF is inflated on the host, the parent commit's path
            L.bmh_tune_set.argtypes = [C.c_char_p, C.c_int, C.c_int]
            L.bmh_tune_set(b"INFLATE_DEVICE", 1, 0)
            try:
                return fn()
            finally:
                L.bmh_tune_set(b"INFLATE_DEVICE", 0, 1)
        def keep_rg(fn):                       # bmh_aligner_set_keep_rg for one call (the header callback counts the lines)
            nat.set_keep_rg(True, lambda lines, libs: None)
            try:
                return fn()
            finally:
                nat.set_keep_rg(False)
        configs = {"align_file_plain": lambda: nat.run_file(p("fq"), paired, sink, **kw),
                   "align_files_plain": lambda: nat.run_files(p("fq"), None, paired, sink, **kw),
                   "align_files_bgzf": lambda: nat.run_files(p("fq.bgzf"), None, paired, sink, **kw),
                   "align_files_bgzf_device_inflate": lambda: device_inflate(lambda: nat.run_files(p("fq.bgzf"), None, paired, sink, **kw)),
                   "align_files_gzip": lambda: nat.run_files(p("fq.gz"), None, paired, sink, **kw),
                   "align_files_bam": lambda: nat.run_files(p("bam"), None, paired, sink, **kw),
                   "align_files_bam_rg_plain": lambda: nat.run_files(p("rg.bam"), None, paired, sink, **kw),
                   "align_files_bam_keep_rg": lambda: keep_rg(lambda: nat.run_files(p("rg.bam"), None, paired, sink, **kw))}
        if paired and a.collate:
            # the aligner's own sorted BAM of these pairs (its members as the sink receives them, behind a header), and the name-grouped BAM of the same pairs
            from bwamem_hip.lib import bgzf_eof, reads_last_collate_counts
            parts = []
            nat.set_output("bam_sorted", 1)
            try:
                nat.run_files(p("bam"), None, True, lambda mv: parts.append(bytes(mv)), **kw)
            finally:
                nat.set_output("sam", 1)
            stream = b"".join(parts)
            del parts
            write_bgzf(p("sorted.bam"), BAM_HEADER)
            with open(p("sorted.bam"), "r+b") as f:
                f.seek(-28, 2); f.write(stream + bgzf_eof())
            write_bgzf(p("grouped.bam"), BAM_HEADER + grouped_records(b"".join(bgzf_members(stream))))
            del stream

            def collate(fn):
                nat.set_collate(True)
                try:
                    return fn()
                finally:
                    nat.set_collate(False)
            configs.update({"align_files_bam_grouped": lambda: nat.run_files(p("grouped.bam"), None, True, sink, **kw),
                            "align_files_bam_sorted_collate": lambda: collate(lambda: nat.run_files(p("sorted.bam"), None, True, sink, **kw))})
        if paired:
            configs.update({"align_files_two_plain": lambda: nat.run_files(p("r1.fq"), p("r2.fq"), True, sink, **kw),
                            "align_files_two_bgzf": lambda: nat.run_files(p("r1.bgzf"), p("r2.bgzf"), True, sink, **kw),
                            "align_files_two_bgzf_device_inflate": lambda: device_inflate(lambda: nat.run_files(p("r1.bgzf"), p("r2.bgzf"), True, sink, **kw)),
                            "align_files_two_gzip": lambda: nat.run_files(p("r1.gz"), p("r2.gz"), True, sink, **kw)})
        if only is not None:
            configs = {k: v for k, v in configs.items() if k in only}
        rows, sizes = {}, set()
        if a.parent:
            import subprocess
            env = dict(os.environ, BMH_RATE_TREE=a.parent, BMH_LIB=os.path.join(a.parent, "bwa-mem_gpu_amd", "libbwamem_hip.so"))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", p("fq"), "--modes", mode, "--reads", str(a.reads), "--runs", str(a.runs),
                                "--genome-mbp", str(a.genome_mbp)], env=env, stdout=subprocess.PIPE, timeout=900)
            line = [l for l in r.stdout.decode().splitlines() if l.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                raise RuntimeError("the --parent child failed")
            rows["parent_align_file_plain"] = json.loads(line[0][6:])
            print(mode, "parent_align_file_plain", json.dumps(rows["parent_align_file_plain"]), flush=True)
        for key, fn in configs.items():
            rows[key] = measure(lambda: (bytes_out.__setitem__(0, 0), fn()), a.runs, n4)
            rows[key]["sam_bytes"] = int(bytes_out[0])
            if key in ("align_files_bam_grouped", "align_files_bam_sorted_collate"):      # (the pairs in another order: the two write the same text as each other)
                rows[key]["file_bytes"] = os.path.getsize(p("grouped.bam" if key.endswith("grouped") else "sorted.bam"))
                if key.endswith("collate"):
                    rows[key]["collate"] = reads_last_collate_counts()
                    if "align_files_bam_grouped" in rows:
                        assert rows[key]["sam_bytes"] == rows["align_files_bam_grouped"]["sam_bytes"], "the collated run and the grouped run wrote different amounts of text"
            elif key != "align_files_bam_keep_rg":                 # (its records carry RG:Z tags: more text)
                sizes.add(bytes_out[0])
            if key != "align_file_plain":
                rows[key]["parser"] = reads_last_counts()
            if key == "align_files_bam_keep_rg":
                rows[key]["file_bytes"] = os.path.getsize(p("rg.bam"))
            if key == "align_files_bam":
                rows[key]["file_bytes"] = os.path.getsize(p("bam")); rows[key]["bgzf_fastq_file_bytes"] = os.path.getsize(p("fq.bgzf"))
            print(mode, key, json.dumps(rows[key]), flush=True)
        compared = [k for k in rows if k not in ("parent_align_file_plain", "align_files_bam_keep_rg", "align_files_bam_grouped", "align_files_bam_sorted_collate")]
        assert len(sizes) == (1 if compared else 0), ("the configurations wrote different amounts of text", sizes)
        nat.free()
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        result["rows"][mode] = dict(rows, reads=n4, lanes=lanes, batches=nb4)
    os.rmdir(tmp)
    line = json.dumps(result)
    print(line)
    if a.out and a.out_key:
        with open(a.out) as f:
            whole = json.loads(f.read())
        whole[a.out_key] = result
        with open(a.out, "w") as f:
            f.write(json.dumps(whole) + "\n")
    elif a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
