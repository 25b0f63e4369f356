#!/usr/bin/env python
"""What coordinate-sorted BAM output costs: reads -> unsorted BAM (the yardstick: the path before sorting existed, unchanged), reads -> sorted BAM + index with every
run in memory and with every run spilled to the temporary file -- each split into the per-batch part and the final merge (stats.format_seconds of a sorted run is
the merge: key sort, windows, compression, index pass, sink) --, and bam_sort alone in records/s -- on the bench's index and read set, in one process, medians of
--runs runs with their spreads.  Writes profiles/bam_sort.json (or --out).  The read set is the bench's two batches, each twice: every read occurs twice, so the
sorted file's size (the two copies land next to each other) and the merge's compression rate are not those of real data.

    python scripts/bam_sort_rate.py [--runs 3] [--reads 1000000] [--genome-mbp 3100] [--out FILE] [--markdup [--groups | --optical N] [--parent-json FILE]]
                                    [--coverage [--coverage-bin N] [--sort-window W] [--parent-json FILE]]
                                    [--stats [--sort-window W] [--parent-json FILE]]
                                    [--recal [--apply-recal] [--off-only] [--sort-window W] [--parent-json FILE]]

--recal: the recalibration-table leg (profiles/bam_recal.json), at the statistics leg's size: the paired rows sorted and sorted + marked from FASTA, and from FASTQ
under two quality alphabets (about 40 distinct values; 4 binned ones) the row sorted + marked and the row with the table counted beside it -- with the counting
kernels alone as the library times them (events around every window's kernel) and their share of the final merge.  --off-only: the rows without the option alone.
--recal --apply-recal: the leg of the apply step (profiles/bam_requal.json) on the 40-value FASTQ: sorted + marked without the option, with the table
counted (the counting kernel's milliseconds per window), with that table applied (the apply kernel's, on the same windows), and with both in one run.
--stats: the statistics leg (profiles/bam_stats.json), at the coverage leg's size: the sorted in-memory row, the same row with duplicates marked, the row `sorted +
marked + statistics` (reads_to_sorted_bam_in_memory_markdup_stats) -- with the statistics kernels alone as the library times them (bmh_aligner_stats_ms: events
around every window's kernel), per run and per window, and their share of the final merge -- and, on the paired set, that row with coverage beside it.
final_merge_ms of every sorted row is the merge in milliseconds: with and without the option side by side.  --parent-json FILE: as under --coverage.

--coverage: the coverage leg (profiles/bam_coverage.json): the sorted in-memory row, the same row with duplicates marked, and the row `sorted + marked + coverage`
(reads_to_sorted_bam_in_memory_markdup_coverage) -- with the depth steps alone as the library times them (bmh_aligner_coverage_ms: events around every window's
step and the last sweep), per run and per window, and their share of the final merge -- and that row once more with bins of --coverage-bin positions (default
1000).  final_merge_ms of every sorted row is the merge in milliseconds: with and without coverage side by side.  --sort-window W: the records of a merge window
(0: the library's default, about 64 MiB).  --parent-json FILE: the output of `--markdup` with the parent commit's library (BMH_LIB) in the same GPU visit; every shared row is compared as under --groups.

--markdup: the duplicate-marking leg instead (profiles/bam_markdup.json): the sorted in-memory row re-run, the same row with duplicates marked -- with the
decision alone and the windows' flag steps alone, as the library times them (bmh_aligner_markdup_times) --, the same two rows on a paired read set (FR pairs
of the same genome, each batch twice), and bam_markdup alone on one batch's records (walk, copies, heads, entries, decision, flags).  Every read of the set occurs twice, so half its templates are duplicates: the
duplicate rate says nothing about real data.

--markdup --optical N: the optical-duplicate leg (profiles/bam_markdup_optical.json): --markdup's rows re-run as they are (the option off, the parent's reads),
then the same reads under names with locations (FC:1:tile:x:y, 16 bytes longer; the second copy of every other read lies 50 pixels from the first, of the others
far away): the marked rows without and with the optical distance N -- the decision alone (it holds the optical step) and the optical step alone, as the library
times them --, and bam_markdup alone on one paired batch's records without and with the option.
--parent-json FILE: the output of `--markdup` on the parent commit in the same GPU visit; every shared row is compared as under --groups.

--markdup --groups: the read-group leg (profiles/bam_markdup_groups.json): --markdup's rows without groups (what a run paid before read groups existed:
the opt-in path must cost nothing when it is off), the sorted rows through bmh_aligner_run_files' loader (the one a run over groups reads through), and the same reads given as 4 groups -- one file per batch -- of one library and of 4 libraries
(bmh_aligner_run_groups; the marked rows, so the entries kernel walks the tags and the decision counts per library).  --parent-json FILE: the output of
`--markdup` on the parent commit in the same GPU visit; its rows are kept beside this commit's and every shared row is compared: the difference of the medians
against the larger of the two rows' own spreads.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bwa-mem_gpu_amd"))
import numpy as np
import torch

import bwamem_hip as B
from bwamem_hip import fmindex as F
from bwamem_hip.lib import ChainOpt, ExtParams, NativeAligner, PeOpt, PostOpt, bam_sort


def stats(secs, unit_count, scale):
    med = sorted(secs)[len(secs) // 2]
    return {"median": round(unit_count / med / scale, 3), "runs": [round(unit_count / s / scale, 3) for s in secs], "spread_pct": round(100 * (max(secs) - min(secs)) / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=3100)
    ap.add_argument("--reads", type=int, default=1_000_000, help="reads per distinct batch; a run takes four times as many")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--markdup", action="store_true")
    ap.add_argument("--groups", action="store_true")
    ap.add_argument("--optical", type=int, default=None, help="with --markdup: the optical distance of the optical-duplicate leg")
    ap.add_argument("--parent-json", default="")
    ap.add_argument("--coverage", action="store_true")
    ap.add_argument("--coverage-bin", type=int, default=1000)
    ap.add_argument("--sort-window", type=int, default=0)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--recal", action="store_true", help="the recalibration-table leg (profiles/bam_recal.json)")
    ap.add_argument("--apply-recal", action="store_true", help="with --recal: the leg of the apply step (profiles/bam_requal.json)")
    ap.add_argument("--off-only", action="store_true", help="with --recal: the rows without the option alone (a parent library under BMH_LIB: the file --parent-json takes)")
    a = ap.parse_args()
    if a.optical is not None and (not a.markdup or a.groups or not 0 <= a.optical <= 0x7fffffff):
        ap.error("--optical N (0 .. 2^31 - 1) goes with --markdup, without --groups")
    if a.coverage and (a.markdup or a.coverage_bin < 1 or a.sort_window < 0):
        ap.error("--coverage goes without --markdup; --coverage-bin N >= 1, --sort-window W >= 0")
    if a.recal and (a.markdup or a.coverage or a.stats or a.sort_window < 0):
        ap.error("--recal goes without --markdup, --coverage and --stats; --sort-window W >= 0")
    if a.stats and (a.markdup or a.coverage or a.sort_window < 0):
        ap.error("--stats goes without --markdup and --coverage; --sort-window W >= 0")
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
    def loc_names(tpl, per_copy):
        """names with locations for the templates tpl (ordinals in the file): copy k of template j lies 50 pixels (j even) or 60 000 (j odd) from copy 0"""
        j, copy = tpl % per_copy, tpl // per_copy
        x = 1000 + (j // 24) % 30000 + np.where(copy > 0, np.where(j % 2 == 0, 50, 60000), 0)
        parts = [np.char.zfill((1101 + j % 24).astype(str), 4), np.char.zfill(x.astype(str), 6), np.char.zfill((1000 + j // 720000).astype(str), 6)]
        s = np.char.add(np.char.add(np.char.add(">FC:1:", parts[0]), np.char.add(":", parts[1])), np.char.add(":", parts[2]))
        return np.frombuffer("".join(s.tolist()).encode(), np.uint8).reshape(len(tpl), -1)
    def write_fasta(dst, names, bases):
        k = names.shape[1]
        recs = np.empty((n4, k + 1 + rl + 1), np.uint8)
        recs[:, :k] = names; recs[:, k] = 10; recs[:, k + 1:k + 1 + rl] = bases.reshape(n4, rl); recs[:, -1] = 10
        recs.tofile(dst)
    names = np.frombuffer("".join(np.char.add(">r", np.char.zfill(np.arange(n4).astype(str), w)).tolist()).encode(), np.uint8).reshape(n4, w + 2)
    tmp = tempfile.mkdtemp(prefix="bmh_bam_sort_")
    path = os.path.join(tmp, "se.fa")
    write_fasta(path, names, asc)
    ppath = os.path.join(tmp, "pe.fa")
    if a.markdup or a.coverage or a.stats or a.recal:         # FR pairs, n reads per distinct batch, each batch twice; mates share a name
        p1 = B.synth.make_pairs(g, n // 2, rl, seed=7, holes=holes)[0]; p2 = B.synth.make_pairs(g, n // 2, rl, seed=1007, holes=holes)[0]
        pasc = B.synth.codes_to_ascii(np.concatenate([p1.reshape(-1), p2.reshape(-1), p1.reshape(-1), p2.reshape(-1)]))
        pn = np.frombuffer("".join(np.char.add(">p", np.char.zfill((np.arange(n4) // 2).astype(str), w)).tolist()).encode(), np.uint8).reshape(n4, w + 2)
        write_fasta(ppath, pn, pasc)
    nat = NativeAligner(dindex, pac_h, n_genome, contigs, None, co, ExtParams.default(), po, pe_o)
    result = {"genome_mbp": a.genome_mbp, "reads_per_run": n4, "setup_s": round(time.time() - t0, 1), "runs": a.runs, "host_threads": nth, "rows": {}}

    def run(fmt, spill=False, keep=None, markdup=False, paired=False, groups=None, files=False, optical=None, coverage=None, qc=None, recal=None, src=None, table=None):
        src = src or (ppath if paired else path)
        if fmt == "bam_sorted":
            nat.set_sorted(level=1, sort_mem=1 if spill else 64 << 30, sort_tmp=tmp, window=a.sort_window, markdup=markdup, optical_distance=optical, coverage=coverage, stats=qc,
                           **({} if recal is None else dict(recal=recal)))
        else:
            nat.set_output(fmt, 1)
        opt_ms, cov_ms, st_ms, rc_ms, ap_ms = [], [], [], [], []
        nbytes = [0]

        def sink(mv):
            nbytes[0] += len(mv)
            if keep is not None and len(keep) < 1:
                keep.append(bytes(mv))
        secs, merge, times = [], [], []
        got = {}
        for it in range(a.runs + 1):
            nbytes[0] = 0
            t1 = time.perf_counter()
            if groups is not None:
                st = nat.run_groups(groups, paired, sink, batch_reads=n4 // 4, n_lanes=3 if paired else 2, n_threads=nth)
            elif files:
                st = nat.run_files(src, None, paired, sink, batch_reads=n4 // 4, n_lanes=3 if paired else 2, n_threads=nth)
            else:
                st = nat.run_file(src, paired, sink, batch_reads=n4 // 4, n_lanes=3 if paired else 2, n_threads=nth)
            if it:
                secs.append(time.perf_counter() - t1); merge.append(st.format_seconds)
                got = nat.sorted_results() if fmt == "bam_sorted" else {}
                if markdup:
                    times.append(got["markdup_times"])
                if optical is not None:
                    opt_ms.append(got["markdup_optical_ms"])
                if coverage is not None:
                    cov_ms.append(got["coverage_ms"])
                if qc is not None:
                    st_ms.append(got["stats_ms"])
                if recal is not None and recal.get("count", True):
                    rc_ms.append(got["recal_ms"])
                if recal is not None and recal.get("apply") is not None:
                    ap_ms.append(got["recal"]["apply"]["ms"])
        row = stats(secs, n4, 1e6)
        row["unit"] = "Mreads/s"; row["bytes_out_per_read"] = round(nbytes[0] / n4, 1)
        if fmt == "bam_sorted":
            nat.sort_index(0)
            row["final_merge"] = stats(merge, n4, 1e6); row["per_batch_part"] = stats([s - m for s, m in zip(secs, merge)], n4, 1e6)
            row["final_merge_share_pct"] = round(100 * sorted(merge)[len(merge) // 2] / sorted(secs)[len(secs) // 2], 1)
            row["final_merge_ms"] = {"median": round(1e3 * sorted(merge)[len(merge) // 2], 2), "runs": [round(1e3 * m, 2) for m in merge]}
            if coverage is not None:
                ms = [t for t, _w in cov_ms]
                cov = got["coverage"]
                row["coverage_steps_alone"] = {"unit": "ms on the stream per run (events around every window's depth step and the last sweep; a step's span holds its two host reads)",
                                               "median": round(sorted(ms)[len(ms) // 2], 3), "runs": [round(t, 3) for t in ms], "windows": [w for _t, w in cov_ms],
                                               "ms_per_window": [round(t / max(w, 1), 3) for t, w in cov_ms],
                                               "share_of_final_merge_pct": round(100 * sorted(ms)[len(ms) // 2] / (1e3 * sorted(merge)[len(merge) // 2]), 2)}
                row["coverage"] = {"tile": 4096, "bin": int(coverage.get("bin", 0)), "bins": int(len(cov["bin_sum"])), "n_reads": int(cov["n_reads"].sum()),
                                   "cov_bases": int(cov["cov_bases"].sum()), "sum_depth": int(cov["sum_depth"].sum()), "max_depth": int(cov["max_depth"].max())}
            if qc is not None:
                ms = [t for t, _w in st_ms]
                row["stats_steps_alone"] = {"unit": "ms on the stream per run (events around every window's statistics kernel)",
                                            "median": round(sorted(ms)[len(ms) // 2], 3), "runs": [round(t, 3) for t in ms], "windows": [w for _t, w in st_ms],
                                            "ms_per_window": [round(t / max(w, 1), 3) for t, w in st_ms],
                                            "share_of_final_merge_pct": round(100 * sorted(ms)[len(ms) // 2] / (1e3 * sorted(merge)[len(merge) // 2]), 2)}
                qs = got["stats"]
                row["stats"] = {"insert_cap": int(qc.get("insert_cap", 65536)), "total": int(qs["flag"][:, 0].sum()), "duplicates": int(qs["flag"][:, 4].sum()), "mapped": int(qs["flag"][:, 6].sum()),
                                "pairs_counted": [int(v) for v in qs["insert_hist"].sum(axis=1)], "largest_insert_bin": int(qs["insert_hist"].max()), "edit_distance": int(qs["summary"][13])}
            if recal is not None and recal.get("apply") is not None:
                ms = [t for t, _w in ap_ms]
                row["apply_steps_alone"] = {"unit": "ms on the stream per run (events around every window's apply kernel)",
                                            "median": round(sorted(ms)[len(ms) // 2], 3), "runs": [round(t, 3) for t in ms], "windows": [w for _t, w in ap_ms],
                                            "ms_per_window": [round(t / max(w, 1), 3) for t, w in ap_ms],
                                            "share_of_final_merge_pct": round(100 * sorted(ms)[len(ms) // 2] / (1e3 * sorted(merge)[len(merge) // 2]), 2)}
                row["apply"] = {k: int(v) for k, v in got["recal"]["apply"].items() if isinstance(v, int)}
            if recal is not None and recal.get("count", True):
                ms = [t for t, _w in rc_ms]
                row["recal_steps_alone"] = {"unit": "ms on the stream per run (events around every window's counting kernel)",
                                            "median": round(sorted(ms)[len(ms) // 2], 3), "runs": [round(t, 3) for t in ms], "windows": [w for _t, w in rc_ms],
                                            "ms_per_window": [round(t / max(w, 1), 3) for t, w in rc_ms],
                                            "share_of_final_merge_pct": round(100 * sorted(ms)[len(ms) // 2] / (1e3 * sorted(merge)[len(merge) // 2]), 2)}
                rs = got["recal"]
                row["recal"] = {"records_counted": int(rs["summary"][1]), "bases_kept": int(rs["summary"][7]), "observations": int(rs["cycle_m"][..., 0].sum()), "mismatches": int(rs["cycle_m"][..., 1].sum()),
                                "qualities_seen": int(np.count_nonzero(rs["cycle_m"][0, :, :, 0].sum(axis=1))), "masked_positions": int(rs["summary"][13])}
            if table is not None:
                table["recal"] = got["recal"]
            if markdup:
                row["counts"] = got["markdup_counts"]
                tpl = row["counts"]["templates"]
                row["decision_alone"] = stats([t["decision_ms"] / 1e3 for t in times], tpl, 1e6); row["decision_alone"]["unit"] = "Mtemplates/s"
                row["decision_alone"]["ms"] = [round(t["decision_ms"], 2) for t in times]
                row["window_flags_alone"] = stats([max(t["window_flags_ms"], 1e-6) / 1e3 for t in times], n4, 1e6); row["window_flags_alone"]["unit"] = "Mrecords/s (ordinals up, flag kernel)"
                row["window_flags_alone"]["ms"] = [round(t["window_flags_ms"], 2) for t in times]
                row["entries_d2h_bytes_per_read"] = round(times[0]["entries_d2h_bytes"] / n4, 1)
                if optical is not None:
                    row["optical_counts"] = got["markdup_optical_counts"]
                    row["optical_step_alone"] = stats([max(t, 1e-6) / 1e3 for t in opt_ms], tpl, 1e6); row["optical_step_alone"]["unit"] = "Mtemplates/s (inside the decision: locations up, sets, sorts, clustering, counts)"
                    row["optical_step_alone"]["ms"] = [round(t, 2) for t in opt_ms]
                if groups is not None:
                    row["library_counts"] = got["markdup_library_counts"]
        return row
    keep = []
    if a.recal:
        # the size of the statistics leg; the reads as FASTQ under two quality alphabets -- about 40 distinct values and 4 binned ones: the kernel's dictionary of
        # (group, quality) slots in LDS fills differently under each
        result["sort_window"] = a.sort_window
        def write_fastq(dst, nm, bases, quals):
            k = nm.shape[1]
            recs = np.empty((n4, k + 1 + rl + 3 + rl + 1), np.uint8)
            recs[:, :k] = nm; recs[:, 0] = ord("@"); recs[:, k] = 10; recs[:, k + 1:k + 1 + rl] = bases.reshape(n4, rl); recs[:, k + 1 + rl] = 10; recs[:, k + 2 + rl] = ord("+"); recs[:, k + 3 + rl] = 10
            recs[:, k + 4 + rl:k + 4 + 2 * rl] = quals + 33; recs[:, -1] = 10
            recs.tofile(dst)
        result["rows"]["paired_reads_to_sorted_bam_in_memory"] = run("bam_sorted", paired=True)
        result["rows"]["paired_reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True, paired=True)
        rng = np.random.default_rng(3)
        for label, alphabet in (("q40", np.arange(2, 42)), ("q4", np.array([2, 12, 23, 37])))[:1 if a.apply_recal else 2]:
            fq = os.path.join(tmp, label + ".fq")
            write_fastq(fq, pn, pasc, alphabet[rng.integers(0, len(alphabet), (n4, rl))].astype(np.uint8))
            result["rows"]["paired_fastq_%s_to_sorted_bam_in_memory_markdup" % label] = run("bam_sorted", markdup=True, paired=True, files=True, src=fq)
            if not a.off_only:
                from bwamem_hip.lib import known_sites_mask
                mask = known_sites_mask([], contigs, l_pac=n_genome, holes=[(int(h[0]), int(h[1]) - int(h[0])) for h in holes])
                counted = {}
                result["rows"]["paired_fastq_%s_to_sorted_bam_in_memory_markdup_recal" % label] = run("bam_sorted", markdup=True, paired=True, files=True, src=fq, recal=dict(mask=mask), table=counted)
                if a.apply_recal:                                 # the table that run counted, applied to the same windows: alone, and with the "after" table counted beside it
                    result["rows"]["paired_fastq_%s_to_sorted_bam_in_memory_markdup_apply" % label] = run("bam_sorted", markdup=True, paired=True, files=True, src=fq, recal=dict(apply=counted["recal"], count=False))
                    result["rows"]["paired_fastq_%s_to_sorted_bam_in_memory_markdup_apply_recal" % label] = run("bam_sorted", markdup=True, paired=True, files=True, src=fq, recal=dict(mask=mask, apply=counted["recal"]))
            os.remove(fq)
        nat.set_output("sam", 1)
        if a.parent_json:
            with open(a.parent_json) as f:
                parent = json.load(f)
            result["parent_rows"] = {k: v for k, v in parent["rows"].items() if k in result["rows"]}
            result["option_off_vs_parent"] = {}
            for k, pr in result["parent_rows"].items():
                tr = result["rows"][k]
                diff = 100 * abs(tr["median"] - pr["median"]) / pr["median"]
                result["option_off_vs_parent"][k] = {"difference_pct": round(diff, 1), "larger_spread_pct": max(tr["spread_pct"], pr["spread_pct"]), "within_spread": diff <= max(tr["spread_pct"], pr["spread_pct"])}
        if a.apply_recal:
            result["not_measured_apply"] = ("several read groups (lane 0 then walks every record's tags and compares up to 255 IDs), real quality distributions (uniform draws here: a "
                                            "lane's histogram runs are short), tables at a large max_cycle (a group's rows are 191 KB at the default 500 and stay in L2)")
        result["not_measured"] = ("real data with deep duplicate stacks (every read occurs twice here), a mask of dbSNP's density (the holes alone here), the time to parse a large VCF, spilled runs, "
                                  "long reads whose cycles exceed the cap, the step beside the window's deflate kernel (no kernel trace was taken)")
        os.remove(ppath); os.remove(path); os.rmdir(tmp)
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_requal.json" if a.apply_recal else "bam_recal.json")
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(result))
        return
    if a.stats:
        result["sort_window"] = a.sort_window
        for pre, pk in (("", {}), ("paired_", dict(paired=True))):
            result["rows"][pre + "reads_to_sorted_bam_in_memory"] = run("bam_sorted", **pk)
            result["rows"][pre + "reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True, **pk)
            result["rows"][pre + "reads_to_sorted_bam_in_memory_markdup_stats"] = run("bam_sorted", markdup=True, qc={}, **pk)
        result["rows"]["paired_reads_to_sorted_bam_in_memory_markdup_coverage_stats"] = run("bam_sorted", markdup=True, coverage={}, qc={}, paired=True)
        nat.set_output("sam", 1)
        if a.parent_json:
            with open(a.parent_json) as f:
                parent = json.load(f)
            result["parent_rows"] = {k: v for k, v in parent["rows"].items() if k in result["rows"]}
            result["parent_genome_mbp"], result["parent_reads_per_run"] = parent.get("genome_mbp"), parent.get("reads_per_run")
            result["option_off_vs_parent"] = {}
            for k, pr in result["parent_rows"].items():
                tr = result["rows"][k]
                diff = 100 * abs(tr["median"] - pr["median"]) / pr["median"]
                result["option_off_vs_parent"][k] = {"difference_pct": round(diff, 1), "larger_spread_pct": max(tr["spread_pct"], pr["spread_pct"]), "within_spread": diff <= max(tr["spread_pct"], pr["spread_pct"])}
        result["not_measured"] = ("real data with deep duplicate stacks (every read occurs twice here), the histogram's atomics under an amplicon library, where nearly every pair has one "
                                  "size, spilled runs, an insert_cap other than the default")
        os.remove(ppath); os.remove(path); os.rmdir(tmp)
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_stats.json")
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(result))
        return
    if a.coverage:
        result["sort_window"] = a.sort_window
        for pre, pk in (("", {}), ("paired_", dict(paired=True))):
            result["rows"][pre + "reads_to_sorted_bam_in_memory"] = run("bam_sorted", **pk)
            result["rows"][pre + "reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True, **pk)
            result["rows"][pre + "reads_to_sorted_bam_in_memory_markdup_coverage"] = run("bam_sorted", markdup=True, coverage={}, **pk)
            result["rows"][pre + "reads_to_sorted_bam_in_memory_markdup_coverage_bins"] = run("bam_sorted", markdup=True, coverage=dict(bin=a.coverage_bin), **pk)
        nat.set_output("sam", 1)
        if a.parent_json:
            with open(a.parent_json) as f:
                parent = json.load(f)
            result["parent_rows"] = {k: v for k, v in parent["rows"].items() if k in result["rows"]}
            result["parent_genome_mbp"], result["parent_reads_per_run"] = parent.get("genome_mbp"), parent.get("reads_per_run")
            result["option_off_vs_parent"] = {}
            for k, pr in result["parent_rows"].items():
                tr = result["rows"][k]
                diff = 100 * abs(tr["median"] - pr["median"]) / pr["median"]
                result["option_off_vs_parent"][k] = {"difference_pct": round(diff, 1), "larger_spread_pct": max(tr["spread_pct"], pr["spread_pct"]), "within_spread": diff <= max(tr["spread_pct"], pr["spread_pct"])}
        result["not_measured"] = ("the deflate kernel of a window on its own (the final merge holds it: the depth steps' share of the merge is the comparison made here), tiles other than the "
                                  "default, spilled runs, real data (every read occurs twice here: half the records are marked and counted out, and the depth is low and even)")
        os.remove(ppath); os.remove(path); os.rmdir(tmp)
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_coverage.json")
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(result))
        return
    if a.markdup and a.groups:
        result["rows"]["reads_to_bam_unsorted"] = run("bam")
        result["rows"]["reads_to_sorted_bam_in_memory"] = run("bam_sorted")
        result["rows"]["reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True)
        result["rows"]["paired_reads_to_sorted_bam_in_memory"] = run("bam_sorted", paired=True)
        result["rows"]["paired_reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True, paired=True)
        # the group runs read through bmh_aligner_run_files' loader (windows of text cut into records on the device), the rows above through bmh_aligner_run_file's
        # (the mapped file cut by host threads): the same file through that loader, without groups, is what the group rows compare with
        result["rows"]["reads_to_sorted_bam_in_memory_files_loader"] = run("bam_sorted", files=True)
        result["rows"]["reads_to_sorted_bam_in_memory_markdup_files_loader"] = run("bam_sorted", markdup=True, files=True)
        whole = np.fromfile(path, np.uint8).reshape(4, -1)                # one file per batch: a group each
        parts = []
        for k in range(4):
            parts.append(os.path.join(tmp, "g%d.fa" % k)); whole[k].tofile(parts[-1])
        del whole
        for what, libs in (("4_groups_1_library", (0, 0, 0, 0)), ("4_groups_4_libraries", (0, 1, 2, 3))):
            groups = [("g%d" % k, libs[k], parts[k], None) for k in range(4)]
            result["rows"]["reads_to_sorted_bam_in_memory_" + what] = run("bam_sorted", groups=groups)
            result["rows"]["reads_to_sorted_bam_in_memory_markdup_" + what] = run("bam_sorted", markdup=True, groups=groups)
        nat.set_output("sam", 1)
        if a.parent_json:
            with open(a.parent_json) as f:
                parent = json.load(f)
            result["parent_rows"] = {k: v for k, v in parent["rows"].items() if k in result["rows"]}
            result["no_groups_vs_parent"] = {}
            for k, pr in result["parent_rows"].items():
                tr = result["rows"][k]
                diff = 100 * abs(tr["median"] - pr["median"]) / pr["median"]
                result["no_groups_vs_parent"][k] = {"difference_pct": round(diff, 1), "larger_spread_pct": max(tr["spread_pct"], pr["spread_pct"]), "within_spread": diff <= max(tr["spread_pct"], pr["spread_pct"])}
        result["not_measured"] = ("groups of unequal size (a group's last batch is short: up to one extra short batch per group), paired groups, BAM groups, more than 4 libraries, "
                                  "spilled runs with marking, reads with base qualities")
        for q in parts + [path, ppath]:
            os.remove(q)
        os.rmdir(tmp)
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_markdup_groups.json")
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(result))
        return
    if a.markdup:
        from bwamem_hip.lib import bam_markdup
        result["rows"]["reads_to_bam_unsorted"] = run("bam", keep=keep)
        result["rows"]["reads_to_sorted_bam_in_memory"] = run("bam_sorted")
        result["rows"]["reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True)
        result["rows"]["paired_reads_to_sorted_bam_in_memory"] = run("bam_sorted", paired=True)
        result["rows"]["paired_reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True, paired=True)
        nat.set_output("sam", 1)
        import zlib
        blob, recs, p = keep[0], [], 0
        while p < len(blob):
            bs = int.from_bytes(blob[p + 16:p + 18], "little") + 1
            recs.append(zlib.decompress(blob[p:p + bs], 31)); p += bs
        stream = b"".join(recs)
        secs = []
        for it in range(a.runs + 1):
            torch.cuda.synchronize(); t1 = time.perf_counter()
            _marked, counts = bam_markdup(stream)
            if it:
                secs.append(time.perf_counter() - t1)
        row = stats(secs, counts["templates"], 1e6); row["unit"] = "Mtemplates/s (the entry point: the host's walk, both copies, heads, entries, decision, flags)"
        row["templates"] = counts["templates"]; row["bytes"] = len(stream)
        result["rows"]["bam_markdup_device"] = row
        if a.optical is not None:
            # the rows above ran on the parent's reads (names r0000001); from here on the same reads under names with locations, 16 bytes longer each
            result["optical_distance"] = a.optical
            write_fasta(path, loc_names(np.arange(n4), 2 * n), asc)
            write_fasta(ppath, loc_names(np.arange(n4) // 2, n), pasc)
            result["rows"]["located_names_reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True)
            result["rows"]["located_names_reads_to_sorted_bam_in_memory_markdup_optical"] = run("bam_sorted", markdup=True, optical=a.optical)
            result["rows"]["located_names_paired_reads_to_sorted_bam_in_memory_markdup"] = run("bam_sorted", markdup=True, paired=True)
            result["rows"]["located_names_paired_reads_to_sorted_bam_in_memory_markdup_optical"] = run("bam_sorted", markdup=True, paired=True, optical=a.optical)
            keep2 = []
            run("bam", keep=keep2, paired=True)
            nat.set_output("sam", 1)
            blob, recs, p = keep2[0], [], 0
            while p < len(blob):
                bs = int.from_bytes(blob[p + 16:p + 18], "little") + 1
                recs.append(zlib.decompress(blob[p:p + bs], 31)); p += bs
            pstream = b"".join(recs)
            for what, kw in (("located_names_paired_bam_markdup_device", {}), ("located_names_paired_bam_markdup_device_optical", dict(optical_distance=a.optical))):
                secs = []
                for it in range(a.runs + 1):
                    torch.cuda.synchronize(); t1 = time.perf_counter()
                    _marked, counts = bam_markdup(pstream, **kw)
                    if it:
                        secs.append(time.perf_counter() - t1)
                row = stats(secs, counts["templates"], 1e6); row["unit"] = "Mtemplates/s (the entry point on one paired batch's records)"
                row["templates"] = counts["templates"]; row["bytes"] = len(pstream)
                if kw:
                    row["optical_duplicate_pairs"] = counts["optical_duplicate_pairs"]; row["located_pairs"] = counts["located_pairs"]
                result["rows"][what] = row
            if a.parent_json:
                with open(a.parent_json) as f:
                    parent = json.load(f)
                result["parent_rows"] = {k: v for k, v in parent["rows"].items() if k in result["rows"]}
                result["option_off_vs_parent"] = {}
                for k, pr in result["parent_rows"].items():
                    tr = result["rows"][k]
                    diff = 100 * abs(tr["median"] - pr["median"]) / pr["median"]
                    result["option_off_vs_parent"][k] = {"difference_pct": round(diff, 1), "larger_spread_pct": max(tr["spread_pct"], pr["spread_pct"]), "within_spread": diff <= max(tr["spread_pct"], pr["spread_pct"])}
            result["not_measured"] = ("the share of templates in sets of two and more pairs on real data (here every read occurs twice: every pair lies in a set of two), sets of thousands of pairs, "
                                      "single-end reads (they hold no pairs: the step uploads their locations and finds no member), spilled runs, reads with base qualities")
            os.remove(ppath)
            os.remove(path); os.rmdir(tmp)
            out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_markdup_optical.json")
            with open(out, "w") as f:
                json.dump(result, f, indent=1)
            print(json.dumps(result))
            return
        result["not_measured"] = "the flag kernel without the upload of its ordinals, spilled runs with marking, reads with base qualities (FASTA: every score is 0, ties go to the ordinal)"
        os.remove(ppath)
        os.remove(path); os.rmdir(tmp)
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_markdup.json")
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(result))
        return
    result["rows"]["reads_to_bam_unsorted"] = run("bam", keep=keep)
    result["rows"]["reads_to_sorted_bam_in_memory"] = run("bam_sorted")
    result["rows"]["reads_to_sorted_bam_spilled"] = run("bam_sorted", spill=True)
    nat.set_output("sam", 1)
    # ---- bam_sort alone: the first batch's records (its members inflated), host bytes in, host bytes out
    import zlib
    blob, recs, p = keep[0], [], 0
    while p < len(blob):
        bs = int.from_bytes(blob[p + 16:p + 18], "little") + 1
        recs.append(zlib.decompress(blob[p:p + bs], 31)); p += bs
    stream = b"".join(recs)
    n_rec, p = 0, 0
    while p < len(stream):
        p += int.from_bytes(stream[p:p + 4], "little") + 4; n_rec += 1
    secs = []
    for it in range(a.runs + 1):
        torch.cuda.synchronize(); t1 = time.perf_counter()
        bam_sort(stream)
        if it:
            secs.append(time.perf_counter() - t1)
    row = stats(secs, n_rec, 1e6); row["unit"] = "Mrecords/s (the entry point: the host's walk, both copies, keys, sort, gather)"; row["records"] = n_rec; row["bytes"] = len(stream)
    result["rows"]["bam_sort_device"] = row
    os.remove(path); os.rmdir(tmp)
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bam_sort.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
