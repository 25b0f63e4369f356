"""File -> SAM rate of long reads: Aligner(long_reads=True).align_file on FASTA files of 1 000, 2 500 and 8 000 bp reads and of a
150 bp + 1 000 bp mix, single-end and paired, in this tree and (--parent DIR) in a build of the parent commit, each in a child process
of its own.  Records reads/s, Mbases/s, the share of batches whose region tail the host took, and the chain + extension + merge stage
time per Mbase (the lanes' host clocks around bmh_chain_extend_merge; the parent's Python loop: not recorded) into
profiles/long_read_rate.json.

    python scripts/long_read_rate.py [--parent DIR] [--mbases 8] [--reps 3] [--out profiles/long_read_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("1000", (1000,)), ("2500", (2500,)), ("8000", (8000,)), ("150+1000", (150, 1000))]


def _reads(rng, g, lens, total, paired):
    from bwamem_hip import synth
    rows, nb = [], 0
    while nb < total:
        ln = lens[len(rows) // (2 if paired else 1) % len(lens)]
        if paired:
            ins = int(rng.integers(ln + 200, ln + 1200))
            p = int(rng.integers(0, len(g) - ins - 10))
            a, b = g[p:p + ln].copy(), g[p + ins - ln:p + ins].copy()
            for x in (a, b):
                k = rng.random(ln) < 0.01
                x[k] = (x[k] + 1) & 3
            rows += [a, synth.revcomp(b)]
            nb += 2 * ln
        else:
            p = int(rng.integers(0, len(g) - ln - 10))
            x = g[p:p + ln].copy()
            k = rng.random(ln) < 0.01
            x[k] = (x[k] + 1) & 3
            rows.append(synth.revcomp(x) if len(rows) & 1 else x)
            nb += ln
    return rows


def worker(tree: str, tmp: str, mbases: float, reps: int) -> dict:
    sys.path.insert(0, os.path.join(tree, "bwa-mem_gpu_amd"))
    import io
    import torch
    from bwamem_hip import fmindex, synth
    from bwamem_hip.aligner import Aligner
    os.makedirs(tmp, exist_ok=True)
    g = synth.make_genome(4_000_000, seed=21, repeat_frac=0.2, repeat_len=(300, 3000), repeat_copies=(5, 60), repeat_div=0.05)
    prefix = os.path.join(tmp, "g.fa")
    if not os.path.exists(prefix + ".bwt"):
        fmindex.write_index(prefix, fmindex.build_fmd_index(g)); fmindex.write_bns(prefix, g)
    al = Aligner(prefix, n_threads=16, long_reads=True)
    out = {"device": torch.cuda.get_device_name(0), "cases": {}}
    rng = np.random.default_rng(5)
    for name, lens in CASES:
        for paired in (False, True):
            rows = _reads(rng, g, lens, int(mbases * 1e6), paired)
            path = os.path.join(tmp, f"r_{name}_{'pe' if paired else 'se'}.fa")
            with open(path, "w") as f:
                for i, x in enumerate(rows):
                    f.write(f">q{i // 2 if paired else i}\n{synth.codes_to_ascii(x).tobytes().decode()}\n")
            nbases = sum(len(x) for x in rows)
            al.align_file(path, io.BytesIO(), paired=paired)             # (warm-up: workspaces, code objects)
            ts, tail, stage = [], [], []
            for _ in range(reps):
                al.host_tail_batches = 0
                t0 = time.perf_counter()
                al.align_file(path, io.BytesIO(), paired=paired)
                ts.append(time.perf_counter() - t0)
                st = getattr(al, "last_stats", None)
                nbat = int(st.n_batches) if st is not None else 0
                tail.append((int(getattr(al, "host_tail_batches", 0)), nbat))
                stage.append(float(st.chain_extend_seconds) if st is not None else None)
                al.last_stats = None
            t = float(np.median(ts))
            key = f"{name}_{'pe' if paired else 'se'}"
            out["cases"][key] = {"reads": len(rows), "mbases": round(nbases / 1e6, 3), "seconds": [round(x, 3) for x in ts],
                                 "reads_per_s": round(len(rows) / t, 1), "mbases_per_s": round(nbases / 1e6 / t, 3),
                                 "host_tail_batches": tail[-1][0], "batches": tail[-1][1] or None,
                                 "chain_extend_s_per_mbase": round(stage[-1] / (nbases / 1e6), 4) if stage[-1] is not None else None}
            print(key, json.dumps(out["cases"][key]), flush=True)
    al.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="a built tree of the parent commit (measured the same way, in its own process)")
    ap.add_argument("--mbases", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default="/tmp/long_read_rate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_read_rate.json"))
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.worker:
        print("RESULT " + json.dumps(worker(a.worker, a.tmp, a.mbases, a.reps)), flush=True)
        return
    res = {}
    for tag, tree in (("this", ROOT), ("parent", a.parent)):
        if not tree:
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", os.path.abspath(tree), "--tmp", a.tmp,
                            "--mbases", str(a.mbases), "--reps", str(a.reps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=3000)
        txt = r.stdout.decode()
        sys.stdout.write(txt)
        if r.returncode != 0:
            raise SystemExit(f"{tag}: worker failed rc={r.returncode}")
        res[tag] = json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
