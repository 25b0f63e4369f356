#!/usr/bin/env python3
"""Records the FASTA -> index fixtures of tests/golden/fasta_index/ with the reference's own `bwa index` CLI.

Writes a handful of small FASTA files that cover what real references hold (many contigs, empty and 1-base contigs, line
widths 60 / 70 / 80 and ragged lines, comments with spaces and tabs, CRLF line ends and a lone "\\r" first line, blank lines,
junk before the first header, '>' inside a line, no final newline, lowercase, N runs at contig starts / middles / ends and
across contig boundaries, `Nn` side by side, every IUPAC code, '-' and '.', an all-N contig), one repeat-rich ~200 kbp
genome with N runs, and a gzip copy of one of them; then indexes each the way the reference's build_index.sh does:

    bwa(OCC_INTV_SHIFT 7) index -s sa -r R -p P f.fa ; rm P.bwt ; bwa(OCC_INTV_SHIFT 6) index -s bwt -p P f.fa ; rm P.bwt1

The reference tree is copied twice into a scratch directory (never edited in place) and each copy is built with its
OCC_INTV_SHIFT.  Usage:  scripts/record_fasta_index.py --reference DIR [--out DIR]
"""
import argparse
import gzip
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem_gpu_amd"))
from bwamem_hip import synth  # noqa: E402

IUPAC = b"RYSWKMBDHVNryswkmbdhvn-."


def _lines(seq: bytes, widths, eol=b"\n") -> bytes:
    out, i, k = [], 0, 0
    while i < len(seq):
        w = widths[k % len(widths)]
        out.append(seq[i:i + w])
        i += w
        k += 1
    return eol.join(out) + (eol if out else b"")


def _rand_seq(rng, n, lower_frac=0.0, amb_frac=0.0) -> bytes:
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    if lower_frac:
        m = rng.random(n) < lower_frac
        s[m] += 32
    if amb_frac:
        m = np.nonzero(rng.random(n) < amb_frac)[0]
        s[m] = np.frombuffer(IUPAC, np.uint8)[rng.integers(0, len(IUPAC), m.size)]
    return s.tobytes()


def fasta_mixed(rng) -> bytes:
    """LF file: junk before the first header, 60/70/80/ragged widths, comments, lowercase, IUPAC, N runs, empty contigs"""
    parts = [b"junk line; ignored\n  also > ignored? no: the first '>' starts the record\n"[:30]]
    parts.append(b">chrA first contig\twith tab\n" + _lines(b"NNNNNNNNNN" + _rand_seq(rng, 6000, 0.2) + b"NNNNN", [60]))
    parts.append(b">empty1\n")
    parts.append(b">one base\n" + b"g\n")
    parts.append(b">chrB\n" + _lines(_rand_seq(rng, 3000) + b"N" * 250 + _rand_seq(rng, 4000, 0.0, 0.01) + b"NNNNnnnnNnNn", [70]))
    parts.append(b">chrC  two  spaces \n" + _lines(b"nnnn" + _rand_seq(rng, 5000, 0.5) + IUPAC * 3 + b"NNNN", [80]))
    parts.append(b">allN\n" + _lines(b"N" * 777, [60]))
    parts.append(b">ragged\n" + _lines(_rand_seq(rng, 7000, 0.1, 0.002), [61, 13, 1, 99, 60, 200, 7]))
    parts.append(b"\n\n>blank_lines\n\nACGT\n\nTTGCA>mid line>\n\n" + _lines(_rand_seq(rng, 900), [60]) + b"\n")
    parts.append(b">@at\n" + _lines(_rand_seq(rng, 2000) + b"N" * 30, [60]))
    parts.append(b">" + b"tail no newline\n" + _lines(b"NN" + _rand_seq(rng, 1500), [60])[:-1])
    return b"".join(parts)


def fasta_crlf(rng) -> bytes:
    """CRLF line ends, a lone "\\r" first sequence line, \\r inside lines, N runs across contig boundaries"""
    parts = [b">crlf1 comment here\r\n" + _lines(_rand_seq(rng, 4000) + b"NNNNNNN", [60], b"\r\n")]
    parts.append(b">crlf2\r\n\r\n" + _lines(b"NNNN" + _rand_seq(rng, 3000, 0.3) + b"NN", [70], b"\r\n"))
    parts.append(b">lone_cr c\r\n\r\n\r\n" + _lines(_rand_seq(rng, 2500), [80], b"\r\n"))
    parts.append(b">cr_inside\t\r\n" + b"AC\rGT\r\n\r\n" + _lines(_rand_seq(rng, 1200, 0.0, 0.01), [60], b"\r\n"))
    parts.append(b">e1\n>e2 c\r\n\r\nACGT\r\nNN\n>e3\nAC GT\tAc\n")
    parts.append(b">last \r\n" + _lines(_rand_seq(rng, 3333) + b"N" * 3, [60], b"\r\n"))
    return b"".join(parts)


def fasta_repeats() -> bytes:
    """~200 kbp repeat-rich genome (synth.make_genome) in 5 contigs with N runs, 60-column lines"""
    g = synth.make_genome(200_000, seed=11)
    s = bytearray(synth.codes_to_ascii(g).tobytes())
    rng = np.random.default_rng(5)
    for p, ln in zip(rng.integers(0, len(s) - 3000, 12), rng.integers(1, 3000, 12)):
        s[p:p + ln] = b"N" * ln
    s[:500] = b"N" * 500
    cuts = [0, 41_000, 90_000, 90_001, 150_000, len(s)]
    out = []
    for k in range(len(cuts) - 1):
        out.append(b">rep%d synthetic repeats\n" % k + _lines(bytes(s[cuts[k]:cuts[k + 1]]), [60]))
    return b"".join(out)


def build_bwa(ref: str, scratch: str, shift: int) -> str:
    d = os.path.join(scratch, f"bwa_index_shift{shift}")
    shutil.copytree(os.path.join(ref, "bwa_index"), d)
    h = os.path.join(d, "bwt.h")
    txt = open(h).read()
    open(h, "w").write(re.sub(r"#define OCC_INTV_SHIFT.*", f"#define OCC_INTV_SHIFT {shift}", txt))
    subprocess.check_call(["make", "-s", "-C", d, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-s", "-C", d, "CFLAGS=-g -Wall -Wno-unused-function -O2 -fcommon"],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(d, "bwa")


def index(bwa7: str, bwa6: str, fa: str, prefix: str, r: int) -> None:
    q = dict(stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.check_call([bwa7, "index", "-s", "sa", "-r", str(r), "-p", prefix, fa], **q)
    os.remove(prefix + ".bwt")
    subprocess.check_call([bwa6, "index", "-s", "bwt", "-p", prefix, fa], **q)
    if os.path.exists(prefix + ".bwt1"):
        os.remove(prefix + ".bwt1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference project's tree (holds bwa_index/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fasta_index"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(2024)
    fastas = {"mixed": fasta_mixed(rng), "crlf": fasta_crlf(rng), "repeats": fasta_repeats()}
    for name, data in fastas.items():
        open(os.path.join(a.out, name + ".fa"), "wb").write(data)
    with open(os.path.join(a.out, "crlf.fa.gz"), "wb") as f:
        f.write(gzip.compress(fastas["crlf"], mtime=0))
    with tempfile.TemporaryDirectory() as scratch:
        bwa7 = build_bwa(a.reference, scratch, 7)
        bwa6 = build_bwa(a.reference, scratch, 6)
        runs = [("mixed", 16), ("crlf", 16), ("repeats", 16), ("repeats", 32)]
        for name, r in runs:
            tmp = os.path.join(scratch, f"{name}_r{r}")
            index(bwa7, bwa6, os.path.join(a.out, name + ".fa"), tmp, r)
            for ext in (".bwt", ".sa", ".pac", ".ann", ".amb"):
                shutil.copy(tmp + ext, os.path.join(a.out, f"{name}_r{r}{ext}"))
            print(f"recorded {name} -r {r}")


if __name__ == "__main__":
    main()
