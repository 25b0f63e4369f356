#!/usr/bin/env python3
"""Records the read-input fixtures of tests/golden/reads_input/ with the reference's own record reader.

Writes a handful of small read files that cover what users hand the aligner (multi-line FASTA at 60 and 80 columns with a short
last line, CR LF line ends, blank lines inside and between records, headers with tabs, comments and /1 /2, lowercase and IUPAC
letters, a last record without its newline, four-line FASTQ, multi-line FASTQ with a quality line that begins with '@', an
R1 / R2 pair of files), then builds -- in a scratch directory, never in the repository -- a small driver of our own around the
reference's kseq_read (src/kseq.h, with the system zlib as the reference uses it), runs it on every fixture and stores what it
returned, record by record, in expected.npz.  The names are stored as bseq_read leaves them (trim_readno, src/bwa.c:27-31: a
trailing "/<digit>" cut), and the pair r1.fq + r2.fq additionally as bseq_read interleaves it (record i of each file -> 2i, 2i+1).

Per fixture F the archive holds F__names, F__comments (NUL-terminated, back to back), F__seq, F__qual (back to back; qual
empty for FASTA) and F__lens.  Only the fixture texts and the archive are committed.

With --cases the same driver runs on the case table of tests/reads_cases.py instead: every text of cases() and both texts of every pair of pairs() (the
refusals are texts kseq_read gives up on or this project refuses: they have no records to store).  It writes cases_expected.npz beside expected.npz, with
the same five arrays per case plus <case>__sha1, the SHA-1 of the case's text (of text1 + NUL + text2 for a pair), so that the table and the archive
cannot drift apart; a pair is stored as bseq_read interleaves it, up to the shorter file's last record.  The texts themselves are not stored: the table
generates them.  The two long-line cases are stored like the others (their sequences compress to about 20 KB each).

Usage:  scripts/record_reads_golden.py --reference DIR [--out DIR] [--cases]
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <stdio.h>
#include <stdint.h>
#include <zlib.h>
#include "kseq.h"
KSEQ_INIT(gzFile, gzread)
static void put(const char *s, size_t l) { uint32_t n = (uint32_t)l; fwrite(&n, 4, 1, stdout); if (l) fwrite(s, 1, l, stdout); }
int main(int argc, char **argv)
{
	gzFile fp = gzopen(argv[1], "r");
	if (!fp) return 2;
	kseq_t *ks = kseq_init(fp);
	int l;
	while ((l = kseq_read(ks)) >= 0) { put(ks->name.s, ks->name.l); put(ks->comment.s, ks->comment.l); put(ks->seq.s, ks->seq.l); put(ks->qual.s, ks->qual.l); }
	kseq_destroy(ks); gzclose(fp);
	return l == -1 ? 0 : 3;
}
"""

IUPAC = b"RYSWKMBDHVN"


def rand_seq(rng, n, lower=0.0, amb=0.0) -> bytes:
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    if lower:
        s[rng.random(n) < lower] += 32
    if amb:
        m = np.nonzero(rng.random(n) < amb)[0]
        s[m] = np.frombuffer(IUPAC, np.uint8)[rng.integers(0, len(IUPAC), m.size)]
    return s.tobytes()


def rand_qual(rng, n, first=None) -> bytes:
    q = (rng.integers(2, 41, n) + 33).astype(np.uint8)
    q[q == ord("@")] = ord("A")
    if first is not None and n:
        q[0] = first
    return q.tobytes()


def wrap(s: bytes, w: int, eol: bytes) -> bytes:
    return eol.join(s[i:i + w] for i in range(0, len(s), w)) + eol


HEADERS = [b"r%d", b"r%d/1", b"r%d/2", b"r%d a comment", b"r%d\ttab comment with  two blanks", b"r%d/1 BC:Z:ACGT\tXY:i:7", b"frag.%d/9 x"]


def fixtures(rng) -> dict:
    fx = {}
    lens = [37, 60, 61, 120, 150, 151, 180, 240, 399, 59, 1, 80, 160, 75]

    def hdr(i):
        return HEADERS[i % len(HEADERS)] % i
    fx["ml60.fa"] = b"".join(b">" + hdr(i) + b"\n" + wrap(rand_seq(rng, n, 0.2 if i % 3 == 0 else 0, 0.02 if i % 4 == 1 else 0), 60, b"\n") for i, n in enumerate(lens))
    body = []
    for i, n in enumerate(lens):
        w = wrap(rand_seq(rng, n, 0.1), 80, b"\r\n")
        if i % 3 == 1 and n > 80:
            w = w.replace(b"\r\n", b"\r\n\r\n", 1)                  # a blank line inside the record
        body.append(b">" + hdr(i) + b"\r\n" + w + (b"\r\n" if i % 4 == 2 else b""))       # ... and between records
    fx["ml80_crlf.fa"] = b"".join(body)[:-2]                           # the last record without its line end
    fx["single.fa"] = b"".join(b">" + hdr(i) + b"\n" + rand_seq(rng, n) + b"\n" for i, n in enumerate(lens))
    fx["four.fq"] = b"".join(b"@" + hdr(i) + b"\n" + rand_seq(rng, n, 0, 0.01) + b"\n+\n" + rand_qual(rng, n) + b"\n" for i, n in enumerate(lens))
    fx["crlf.fq"] = b"".join(b"@" + hdr(i) + b"\r\n" + rand_seq(rng, n) + b"\r\n+" + (hdr(i) if i % 2 else b"") + b"\r\n" + rand_qual(rng, n) + b"\r\n" + (b"\r\n" if i % 5 == 0 else b"")
                             for i, n in enumerate(lens))[:-2]
    fx["ml.fq"] = b"".join(b"@" + hdr(i) + b"\n" + wrap(rand_seq(rng, n), 50, b"\n") + b"+\n" + wrap(rand_qual(rng, n, first=ord("@") if i % 2 == 0 else None), 50, b"\n")
                           for i, n in enumerate(lens))
    r1, r2 = [], []
    for i, n in enumerate(lens):
        name = b"pair%d" % i
        r1.append(b"@" + name + b"/1 first\n" + rand_seq(rng, n) + b"\n+\n" + rand_qual(rng, n) + b"\n")
        m = lens[(i + 3) % len(lens)]
        r2.append(b"@" + name + b"/2\tsecond\r\n" + rand_seq(rng, m) + b"\r\n+\r\n" + rand_qual(rng, m) + b"\r\n")
    fx["r1.fq"], fx["r2.fq"] = b"".join(r1), b"".join(r2)
    return fx


def trim_readno(name: bytes) -> bytes:
    return name[:-2] if len(name) > 2 and name[-2:-1] == b"/" and name[-1:].isdigit() else name


def parse_driver_output(raw: bytes):
    recs, p = [], 0
    while p < len(raw):
        f = []
        for _ in range(4):
            (n,) = struct.unpack_from("<I", raw, p)
            f.append(raw[p + 4:p + 4 + n]); p += 4 + n
        recs.append(tuple(f))
    return recs


def pack(recs) -> dict:
    u8 = lambda b: np.frombuffer(b, np.uint8).copy()  # noqa: E731
    return dict(names=u8(b"".join(trim_readno(r[0]) + b"\0" for r in recs)), comments=u8(b"".join(r[1] + b"\0" for r in recs)),
                seq=u8(b"".join(r[2] for r in recs)), qual=u8(b"".join(r[3] for r in recs)), lens=np.array([len(r[2]) for r in recs], np.uint32))


def build_driver(reference: str, tmp: str) -> str:
    src = os.path.join(tmp, "kseq_driver.c")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "kseq_driver")
    subprocess.run(["cc", "-O1", "-I", os.path.join(reference, "src"), src, "-o", exe, "-lz"], check=True)
    return exe


def record_cases(reference: str, out: str) -> int:
    import hashlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import reads_cases
    arch, n = {}, 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(reference, tmp)

        def run(text: bytes):
            p = os.path.join(tmp, "case.txt")
            with open(p, "wb") as f:
                f.write(text)
            return parse_driver_output(subprocess.run([exe, p], check=True, stdout=subprocess.PIPE).stdout)

        def store(name, recs, digest):
            for k, v in pack(recs).items():
                arch[f"{name}__{k}"] = v
            arch[f"{name}__sha1"] = np.frombuffer(digest, np.uint8).copy()
        for name, (text, _kind, _route) in reads_cases.cases().items():
            recs = run(text)
            store(name, recs, hashlib.sha1(text).digest()); n += len(recs)
        for name, (t1, t2) in reads_cases.pairs().items():
            inter = [r for pr in zip(run(t1), run(t2)) for r in pr]
            store(name, inter, hashlib.sha1(t1 + b"\0" + t2).digest()); n += len(inter)
    path = os.path.join(out, "cases_expected.npz")
    np.savez_compressed(path, **arch)
    print(f"wrote {path}: {len(reads_cases.cases())} cases and {len(reads_cases.pairs())} pairs, {n} records, {os.path.getsize(path)} bytes")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="the reference's source tree (its src/kseq.h is compiled into the driver)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "reads_input"))
    ap.add_argument("--cases", action="store_true", help="record tests/reads_cases.py into cases_expected.npz instead of the fixtures")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.cases:
        return record_cases(a.reference, a.out)
    fx = fixtures(np.random.default_rng(20240607))
    for name, text in fx.items():
        with open(os.path.join(a.out, name), "wb") as f:
            f.write(text)
    arch = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(a.reference, tmp)
        per = {}
        for name in fx:
            raw = subprocess.run([exe, os.path.join(a.out, name)], check=True, stdout=subprocess.PIPE).stdout
            per[name] = parse_driver_output(raw)
            for k, v in pack(per[name]).items():
                arch[f"{name}__{k}"] = v
        inter = [r for pr in zip(per["r1.fq"], per["r2.fq"]) for r in pr]
        for k, v in pack(inter).items():
            arch[f"r1.fq+r2.fq__{k}"] = v
    np.savez_compressed(os.path.join(a.out, "expected.npz"), **arch)
    print(f"wrote {len(fx)} fixtures and expected.npz ({sum(len(v) for v in per.values())} records) to {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
