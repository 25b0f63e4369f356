"""Flagstat, idxstats, alignment summary and insert sizes of sorted BAM without a GPU: a Python model that follows the definition record by
record, pinned by a hand-counted table; the host form against it; the texts and insert_size_metrics by hand; the refusals word for word; the windows of the host
merge; the index's metadata words; and csrc/bam_stats_core.h with the host form under AddressSanitizer and UBSan (a stand-alone program, run as a child process)."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_sort import BamFile, parse_bai, py_sort, split_records

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ("total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped", "primary_mapped", "paired", "read1", "read2", "properly_paired",
         "both_mapped", "singletons", "mate_on_different_contig", "mate_on_different_contig_mapq5")
SUMMARY = ("reads", "bases", "reads_mapped", "bases_mapped", "reads_mq0", "max_read_length", "bases_aligned", "bases_soft_clipped", "ins_events", "ins_bases", "del_events",
           "del_bases", "reads_with_nm", "edit_distance")
FR, RF, TANDEM = 0, 1, 2
E_REF, E_TAGS, E_NM, E_PLACEHOLDER = 1, 2, 3, 4
INT32_MIN = -(1 << 31)
M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
WORDS = {E_REF: "names a reference outside the header's (refID below -1 or not below the number of contigs)",
         E_TAGS: "has tags that cannot be walked to the record's end: the statistics read NM from them",
         E_NM: "has an NM tag that is no count (a type other than c C s S i I, or a negative value)",
         E_PLACEHOLDER: "holds the long-CIGAR placeholder (its operations are in its CG tag): the statistics read the record's own operations"}


def srec(name=b"r", rid=0, pos=10, flag=0, mapq=30, ops=((50, M),), l_seq=None, nrid=-1, npos=-1, tlen=0, tag=b"") -> bytes:
    """a record built field by field (pos 0-based); l_seq None: the bases the operations read"""
    from test_bam_core import reg2bin
    if l_seq is None:
        l_seq = sum(n for n, o in ops if o in (M, I, S, EQ, X))
    rl = sum(n for n, o in ops if o in (M, D, N, EQ, X))
    bin_ = 4680 if pos < 0 else reg2bin(pos, pos + 1 if (flag & 4) or rl == 0 else pos + rl)
    body = struct.pack("<iiBBHHHIiii", rid, pos, len(name) + 1, mapq, bin_, len(ops), flag, l_seq, nrid, npos, tlen) + name + b"\0"
    body += b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + b"\x12" * ((l_seq + 1) // 2) + b"\x1e" * l_seq + tag
    return struct.pack("<I", len(body)) + body


# ---------------------------------------------------------------------------------------------------------------- the model

def walk_tags(t: bytes):
    """the tags by their types -> (status, has_nm, nm, has CG:B,I): the first NM counts"""
    p, has_nm, nm, cg = 0, False, 0, False
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p < len(t):
        if len(t) - p < 3:
            return E_TAGS, False, 0, False
        key, ty = t[p:p + 2], chr(t[p + 2])
        p += 3
        first_nm = key == b"NM" and not has_nm
        if ty in sizes:
            ln = sizes[ty]
        elif ty in "ZH":
            if first_nm:
                return E_NM, False, 0, False
            e = t.find(b"\0", p)
            if e < 0:
                return E_TAGS, False, 0, False
            ln = e + 1 - p
        elif ty == "B":
            if first_nm:
                return E_NM, False, 0, False
            if len(t) - p < 5:
                return E_TAGS, False, 0, False
            sub = chr(t[p])
            if sub not in "cCsSiIf":
                return E_TAGS, False, 0, False
            if key == b"CG" and sub == "I":
                cg = True
            ln = 5 + sizes[sub] * struct.unpack_from("<I", t, p + 1)[0]
        else:
            return E_TAGS, False, 0, False
        if ln > len(t) - p:
            return E_TAGS, False, 0, False
        if first_nm:
            if ty not in "cCsSiI":
                return E_NM, False, 0, False
            v = struct.unpack_from("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], t, p)[0]
            if v < 0:
                return E_NM, False, 0, False
            has_nm, nm = True, v
        p += ln
    return 0, has_nm, nm, cg


def model(stream: bytes, n_contigs: int, cap: int = 65536):
    """the definition, record by record: bam_stats' dict, or ("refused", index, code) for the first record refused"""
    flag = [[0] * 16, [0] * 16]
    cm, cu, unplaced = [0] * n_contigs, [0] * n_contigs, 0
    s = dict.fromkeys(SUMMARY, 0)
    mapq_h = [0] * 256
    hist = np.zeros((3, cap + 1), dtype=np.uint64)
    lo, hi = [None] * 3, [0] * 3
    for index, r in enumerate(split_records(stream)):
        rid, pos, l_name, mapq, _bin, n_ops, fl, l_seq, nrid, npos, tlen = struct.unpack_from("<iiBBHHHIiii", r, 4)
        if not -1 <= rid < n_contigs:
            return ("refused", index, E_REF)
        f = flag[1 if fl & 0x200 else 0]
        un = bool(fl & 0x4)
        f[0] += 1
        if fl & 0x100:
            f[2] += 1
        elif fl & 0x800:
            f[3] += 1
        else:
            f[1] += 1
            if fl & 0x1:
                f[8] += 1
                if fl & 0x2 and not un:
                    f[11] += 1
                if fl & 0x40:
                    f[9] += 1
                if fl & 0x80:
                    f[10] += 1
                if fl & 0x8 and not un:
                    f[13] += 1
                if not un and not fl & 0x8:
                    f[12] += 1
                    if nrid != rid:
                        f[14] += 1
                        if mapq >= 5:
                            f[15] += 1
            if not un:
                f[7] += 1
            if fl & 0x400:
                f[5] += 1
        if not un:
            f[6] += 1
        if fl & 0x400:
            f[4] += 1
        if rid < 0:
            unplaced += 1
        elif un:
            cu[rid] += 1
        else:
            cm[rid] += 1
        if fl & 0x900:
            continue
        s["reads"] += 1; s["bases"] += l_seq; s["max_read_length"] = max(s["max_read_length"], l_seq)
        if un:
            continue
        ops = [(v >> 4, v & 15) for v in struct.unpack_from("<%dI" % n_ops, r, 36 + l_name)]
        st, has_nm, nm, cg = walk_tags(r[36 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq:]) if 36 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq <= len(r) else (E_TAGS, 0, 0, 0)
        if st:
            return ("refused", index, st)
        if cg and n_ops == 2 and ops[0] == (l_seq, S) and ops[1][1] == N:
            return ("refused", index, E_PLACEHOLDER)
        s["reads_mapped"] += 1; s["bases_mapped"] += l_seq; s["reads_mq0"] += mapq == 0
        mapq_h[mapq] += 1
        s["bases_aligned"] += sum(n for n, o in ops if o in (M, EQ, X, I))
        s["bases_soft_clipped"] += sum(n for n, o in ops if o == S)
        s["ins_events"] += sum(1 for n, o in ops if o == I); s["ins_bases"] += sum(n for n, o in ops if o == I)
        s["del_events"] += sum(1 for n, o in ops if o == D); s["del_bases"] += sum(n for n, o in ops if o == D)
        if has_nm:
            s["reads_with_nm"] += 1; s["edit_distance"] += nm
        if fl & 0x1 and fl & 0x80 and not fl & (0x8 | 0x400) and rid == nrid and tlen != 0:
            size = abs(tlen)
            if bool(fl & 0x10) == bool(fl & 0x20):
                o = TANDEM
            elif not fl & 0x10:
                o = FR if tlen > 0 else RF
            else:
                o = FR if npos + 1 < pos + sum(n for n, op in ops if op in (M, EQ, X, D, N)) else RF
            hist[o][min(size, cap)] += np.uint64(1)
            lo[o] = size if lo[o] is None else min(lo[o], size); hi[o] = max(hi[o], size)
    u = lambda v: np.array(v, dtype=np.uint64)
    return dict(flag=u(flag), summary=u([s[k] for k in SUMMARY]), mapq=u(mapq_h), contig_mapped=u(cm), contig_unmapped=u(cu), unplaced=u([unplaced]), insert_hist=hist,
                insert_min=u([v or 0 for v in lo]), insert_max=u(hi))


def equal(a: dict, b: dict) -> bool:
    return set(a) == set(b) and all(a[k].dtype == np.uint64 and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------- the table

def flag_stream() -> bytes:
    """every branch of the flag walk, once without and once with 0x200"""
    rows = [dict(flag=0), dict(flag=0x100), dict(flag=0x800), dict(flag=0x900), dict(flag=0x4, rid=-1, pos=-1), dict(flag=0x400), dict(flag=0x500),
            dict(flag=0x1 | 0x2 | 0x40, nrid=0), dict(flag=0x1 | 0x2 | 0x4 | 0x80), dict(flag=0x1 | 0x40 | 0x80, nrid=0), dict(flag=0x1, nrid=0), dict(flag=0x1 | 0x8 | 0x40),
            dict(flag=0x1 | 0x8 | 0x4 | 0x80), dict(flag=0x1 | 0x40, nrid=1, mapq=4), dict(flag=0x1 | 0x80, nrid=1, mapq=5), dict(flag=0x1 | 0x40, nrid=-1), dict(flag=0, rid=-1, pos=-1)]
    return b"".join(srec(b"f%d" % k, **dict(r, flag=r["flag"] | qc)) for qc in (0, 0x200) for k, r in enumerate(rows))


def nm(ty: str, v) -> bytes:
    return b"NM" + ty.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[ty], v)


def summary_stream() -> bytes:
    every = ((5, S), (10, M), (2, I), (3, D), (100, N), (4, EQ), (1, X), (2, P), (6, H), (7, 9), (9, 15))
    return b"".join([srec(b"a", mapq=0, tag=nm("c", 3)), srec(b"b", mapq=255, ops=every, tag=nm("C", 200)), srec(b"c", ops=(), l_seq=0, tag=nm("s", 300)), srec(b"d", tag=nm("S", 60000)),
                     srec(b"e", tag=nm("i", 70000)), srec(b"f", tag=nm("I", 3000000000)), srec(b"g", tag=b"XAZab\0"),
                     srec(b"h", tag=b"XAZhello\0" + b"XBBc" + struct.pack("<I", 3) + b"\1\2\3" + nm("C", 7)), srec(b"i", flag=0x4, tag=b"NMZab"), srec(b"j", flag=0x100, tag=b"NMZab\0"),
                     srec(b"k", tag=nm("C", 1) + nm("C", 9))])


def placeholder(with_tag=True) -> bytes:
    tag = b"CGBI" + struct.pack("<I", 2) + struct.pack("<II", 50 << 4, 30 << 4) if with_tag else b""
    return srec(b"long", ops=((50, S), (80, N)), l_seq=50, tag=nm("i", 3) + b"XAZab\0" + tag)


REFUSED = [("NM of type Z", srec(b"x", tag=b"NMZ12\0"), E_NM), ("NM negative", srec(b"x", tag=nm("c", -1)), E_NM), ("NM negative, 32 bits", srec(b"x", tag=nm("i", -5)), E_NM),
           ("NM of type A", srec(b"x", tag=b"NMA7"), E_NM), ("NM of type f", srec(b"x", tag=nm("f", 1.0)), E_NM), ("NM of type B", srec(b"x", tag=b"NMBc" + struct.pack("<I", 1) + b"\1"), E_NM),
           ("a value cut short", srec(b"x", tag=b"XAi\1\2"), E_TAGS), ("two bytes of a tag", srec(b"x", tag=nm("C", 1) + b"XA"), E_TAGS), ("Z without its NUL", srec(b"x", tag=b"XAZabc"), E_TAGS),
           ("B of an unknown subtype", srec(b"x", tag=b"XBBq" + struct.pack("<I", 0)), E_TAGS), ("B past the record", srec(b"x", tag=b"XBBi" + struct.pack("<I", 9) + b"\0" * 8), E_TAGS),
           ("an unknown type", srec(b"x", tag=b"XA?1"), E_TAGS), ("bases past the record", srec(b"x")[:-20], E_TAGS), ("the placeholder", placeholder(), E_PLACEHOLDER),
           ("refID = n_contigs", srec(b"x", rid=2), E_REF), ("refID -2", srec(b"x", rid=-2, flag=0x4), E_REF)]


def cut(r: bytes) -> bytes:
    """a record shortened from behind keeps a block_size that fits"""
    return struct.pack("<I", len(r) - 4) + r[4:]


def insert_stream() -> bytes:
    fwd, rev = 0x1 | 0x80 | 0x20, 0x1 | 0x80 | 0x10
    rows = [dict(flag=fwd, tlen=0), dict(flag=fwd, tlen=1), dict(flag=fwd, tlen=-1)]
    rows += [dict(flag=fwd, tlen=t) for t in (3, 4, 5, 65535, 65536, 65537)]
    rows += [dict(flag=fwd, tlen=INT32_MIN), dict(flag=0x1 | 0x80, tlen=7), dict(flag=0x1 | 0x80 | 0x10 | 0x20, tlen=-8)]
    rows += [dict(flag=rev, pos=100, npos=149, tlen=-10), dict(flag=rev, pos=100, npos=148, tlen=-11)]               # pos + reflen = 150
    rows += [dict(flag=rev, pos=100, npos=98, tlen=12, ops=(), l_seq=50), dict(flag=rev, pos=100, npos=99, tlen=13, ops=(), l_seq=50)]
    rows += [dict(flag=fwd | 0x400, tlen=20), dict(flag=0x1 | 0x40 | 0x20, tlen=21), dict(flag=fwd | 0x8, tlen=22), dict(flag=fwd, tlen=23, nrid=1), dict(flag=fwd | 0x100, tlen=24),
             dict(flag=fwd | 0x800, tlen=25), dict(flag=0x80 | 0x20, tlen=26), dict(flag=fwd | 0x4, tlen=27)]
    return b"".join(srec(b"i%d" % k, **dict(dict(nrid=0), **r)) for k, r in enumerate(rows))


def table():
    """(what, n_contigs, stream, insert_cap, must): must = what the model's answer has to hold, counted by hand"""
    col = [17, 13, 3, 1, 2, 1, 14, 10, 9, 5, 4, 1, 6, 1, 3, 2]
    mq = {4: 2, 5: 2, 30: 16}
    ins = insert_stream()
    n_ins = len(split_records(ins))
    return [
        ("flags", 2, flag_stream(), 65536, dict(flag=[col, col], contig_mapped=[26, 0], contig_unmapped=[4, 0], unplaced=[4], mapq=mq,
                                                summary=[26, 1300, 20, 1000, 0, 50, 1000, 0, 0, 0, 0, 0, 0, 0], hist={})),
        ("summary", 1, summary_stream(), 65536, dict(summary=[10, 422, 9, 372, 1, 50, 367, 5, 1, 2, 1, 3, 8, 3000130511], mapq={0: 1, 255: 1, 30: 7}, contig_mapped=[10], contig_unmapped=[1],
                                                    unplaced=[0], hist={})),
        ("the placeholder's operations without the tag", 1, placeholder(False), 65536, dict(summary=[1, 50, 1, 50, 0, 50, 0, 50, 0, 0, 0, 0, 1, 3], hist={})),
        ("inserts, cap 65536", 2, ins, 65536, dict(hist={(FR, 1): 1, (FR, 3): 1, (FR, 4): 1, (FR, 5): 1, (FR, 11): 1, (FR, 12): 1, (FR, 65535): 1, (FR, 65536): 2, (RF, 1): 1, (RF, 10): 1, (RF, 13): 1,
                                                         (RF, 65536): 1, (TANDEM, 7): 1, (TANDEM, 8): 1}, insert_min=[1, 1, 7], insert_max=[65537, 1 << 31, 8], contig_mapped=[n_ins - 1, 0])),
        ("inserts, cap 4", 2, ins, 4, dict(hist={(FR, 1): 1, (FR, 3): 1, (FR, 4): 7, (RF, 1): 1, (RF, 4): 3, (TANDEM, 4): 2}, insert_min=[1, 1, 7], insert_max=[65537, 1 << 31, 8])),
        ("inserts, cap 2", 2, ins, 2, dict(hist={(FR, 1): 1, (FR, 2): 8, (RF, 1): 1, (RF, 2): 3, (TANDEM, 2): 2}, insert_min=[1, 1, 7], insert_max=[65537, 1 << 31, 8])),
        ("empty stream", 3, b"", 65536, dict(flag=[[0] * 16, [0] * 16], summary=[0] * 14, mapq={}, contig_mapped=[0, 0, 0], contig_unmapped=[0, 0, 0], unplaced=[0], hist={}, insert_min=[0, 0, 0],
                                             insert_max=[0, 0, 0])),
    ] + [("refused: " + what, 2, srec(b"ok") + r + srec(b"behind", tag=b"NMZ\0"), 65536, dict(refused=(1, code))) for what, r, code in REFUSED if what != "bases past the record"] + [
        ("refused: bases past the record", 2, srec(b"ok") + cut(srec(b"x")[:-20]), 65536, dict(refused=(1, E_TAGS)))]


def check_must(what, m, must: dict):
    if "refused" in must:
        assert m == ("refused",) + must["refused"], (what, m)
        return
    assert isinstance(m, dict), (what, m)
    for k, v in must.items():
        if k == "hist":
            want = np.zeros_like(m["insert_hist"])
            for (o, s), c in v.items():
                want[o][s] = c
            assert np.array_equal(m["insert_hist"], want), (what, [(o, s, int(m["insert_hist"][o][s])) for o, s in zip(*np.nonzero(m["insert_hist"]))])
        elif k == "mapq":
            assert {q: int(c) for q, c in enumerate(m["mapq"]) if c} == v, (what, k)
        else:
            assert m[k].tolist() == v, (what, k, m[k].tolist())


def synthetic(n=3000, seed=11) -> tuple:
    """about n records over three contigs and none, in no order: every kind of flag, mates near and far, operations, NM tags of every type, every mapq"""
    rng = np.random.default_rng(seed)
    shapes = [((50, M),), ((5, S), (20, M), (2, I), (23, M)), ((20, M), (7, D), (30, M)), ((15, M), (200, N), (35, M)), ((10, EQ), (1, X), (39, EQ)), ((3, H), (60, M), (4, S)),
              ((30, M), (1, D), (1, I), (2, D), (20, M)), ((120, M),), ()]
    tags = [b"", nm("C", 2), nm("c", 5), nm("s", 300), nm("S", 40000), nm("i", 9), nm("I", 77), b"XAZchr1,+5,50M,0;\0" + nm("C", 1), b"XBBs" + struct.pack("<I", 2) + b"\1\0\2\0" + nm("i", 4),
            b"ASi" + struct.pack("<i", 44), nm("C", 3) + nm("C", 250)]
    out = []
    for i in range(n):
        rid = int(rng.integers(-1, 3))
        flag = int(rng.choice([0, 0x10, 0x1 | 0x40 | 0x20, 0x1 | 0x80 | 0x10, 0x1 | 0x80 | 0x20, 0x1 | 0x80, 0x1 | 0x80 | 0x30, 0x1 | 0x2 | 0x80 | 0x20, 0x1 | 0x8 | 0x40, 0x1 | 0x4 | 0x80,
                               0x100, 0x800, 0x900, 0x4, 0x1 | 0x40 | 0x80 | 0x20]))
        if i % 7 == 0:
            flag |= 0x200
        if i % 11 == 0:
            flag |= 0x400
        pos = int(rng.integers(0, 2000)) if rid >= 0 else -1
        nrid = rid if rng.random() < 0.8 else int(rng.integers(-1, 3))
        tlen = int(rng.choice([0, 1, -1, 3, 4, 5, -4, 300, -300, 65535, 65536, 65537, INT32_MIN, (1 << 31) - 1])) if rng.random() < 0.4 else int(rng.integers(-600, 600))
        ops = shapes[int(rng.integers(0, len(shapes)))]
        out.append(srec(b"x%04d" % i, rid, pos, flag, int(rng.integers(0, 256)) if i % 5 == 0 else int(rng.integers(0, 61)), ops, None if ops else int(rng.integers(0, 80)), nrid,
                        pos + int(rng.integers(-60, 60)) if rid >= 0 else -1, tlen, tags[int(rng.integers(0, len(tags)))]))
    return 3, b"".join(out)


_MODEL = {}


def cached_model(what, stream, n_contigs, cap):
    """the model's answer, computed once per case and shared (test_bam_stats_gpu.py reads it too)"""
    if (what, cap) not in _MODEL:
        _MODEL[(what, cap)] = model(stream, n_contigs, cap)
    return _MODEL[(what, cap)]


def corpus():
    """(what, n_contigs, stream, cap) of the table and of the synthetic stream at both caps"""
    n, s = synthetic()
    return [(w, nc, st, cap) for w, nc, st, cap, _m in table()] + [("synthetic", n, s, 65536), ("synthetic", n, s, 4)]


def refusal_words(fn: str, index: int, code: int) -> str:
    return "%s: record %d %s" % (fn, index, WORDS[code])


# ---------------------------------------------------------------------------------------------------------------- the texts, formatted here

def pct(a, b):
    return "%.2f%%" % (100.0 * a / b) if b else "N/A"


def flagstat_by_model(m) -> str:
    p, f = m["flag"].tolist()
    rows = []
    for k, words in enumerate(("in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary", "duplicates", "primary duplicates", "mapped", "primary mapped",
                               "paired in sequencing", "read1", "read2", "properly paired", "with itself and mate mapped", "singletons", "with mate mapped to a different chr",
                               "with mate mapped to a different chr (mapQ>=5)")):
        over = {6: 0, 7: 1, 11: 8, 13: 8}.get(k)
        rows.append("%d + %d %s" % (p[k], f[k], words) + ("" if over is None else " (%s : %s)" % (pct(p[k], p[over]), pct(f[k], f[over]))))
    return "\n".join(rows) + "\n"


def idxstats_by_model(m, contigs) -> str:
    return "".join("%s\t%d\t%d\t%d\n" % (nm_, ln, m["contig_mapped"][c], m["contig_unmapped"][c]) for c, (nm_, ln) in enumerate(contigs)) + "*\t0\t0\t%d\n" % m["unplaced"][0]


def metrics_by_model(hist, lo, hi):
    """insert_size_metrics the slow way: every value written out"""
    cap = len(hist) - 1
    xs = sorted(s for s in range(cap + 1) for _ in range(int(hist[s])))
    if not xs:
        return None
    med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
    median = med(xs)
    mad = med(sorted(abs(x - median) for x in xs))
    kept = [x for x in xs if x <= min(median + 10 * mad, cap - 1)]
    mean = sum(kept) / len(kept) if kept else 0.0
    sd = (sum((x - mean) ** 2 for x in kept) / (len(kept) - 1)) ** 0.5 if len(kept) > 1 else 0.0
    counts = [int(hist[s]) for s in range(cap + 1)]
    return dict(pairs=len(xs), median=median, mad=mad, mode=counts.index(max(counts)), min=int(lo), max=int(hi), mean=mean, sd=sd)


def stats_by_model(m, contigs) -> str:
    rows = ["FS\t%s\t%d\t%d" % (nm_, m["flag"][0][k], m["flag"][1][k]) for k, nm_ in enumerate(FLAGS)]
    rows += ["IX\t" + l for l in idxstats_by_model(m, contigs).split("\n")[:-1]]
    s = dict(zip(SUMMARY, m["summary"].tolist()))
    rows += ["SN\t%s\t%d" % (k, s[k]) for k in SUMMARY]
    rows.append("SN\terror_rate\t" + ("%.6e" % (s["edit_distance"] / s["bases_aligned"]) if s["bases_aligned"] else "0"))
    rows += ["MQ\t%d\t%d" % (q, c) for q, c in enumerate(m["mapq"].tolist()) if c]
    h = m["insert_hist"]
    cap = h.shape[1] - 1
    rows += ["IS\t%s\t%d\t%d\t%d" % ("%d+" % cap if sz == cap else sz, h[0][sz], h[1][sz], h[2][sz]) for sz in range(cap + 1) if h[:, sz].any()]
    for o, nm_ in enumerate(("FR", "RF", "TANDEM")):
        x = metrics_by_model(h[o], m["insert_min"][o], m["insert_max"][o]) if cap <= 1024 or h[o].sum() < 100000 else None
        if x:
            rows.append("IM\t%s\t%d\t%.1f\t%.1f\t%d\t%d\t%d\t%.2f\t%.2f" % (nm_, x["pairs"], x["median"], x["mad"], x["mode"], x["min"], x["max"], x["mean"], x["sd"]))
    return "".join(r + "\n" for r in rows)


# ---------------------------------------------------------------------------------------------------------------- tests

def test_model_on_the_table():
    for what, nc, stream, cap, must in table():
        assert must, what
        check_must(what, model(stream, nc, cap), must)
    nc, s = synthetic()
    m = model(s, nc)
    assert 2900 <= len(split_records(s)) <= 3100 and all(int(v) > 50 for v in m["flag"][0]) and all(int(v) for v in m["flag"][1])
    assert all(int(v) for v in m["summary"]) and (m["insert_hist"].sum(axis=1) > 20).all() and int(m["insert_hist"][:, 65536].sum()) > 5 and int(m["insert_max"].max()) == 1 << 31
    assert int(np.count_nonzero(m["mapq"])) > 100 and int(m["unplaced"][0]) > 100 and all(int(v) for v in m["contig_unmapped"])


def test_host_equals_model():
    from bwamem_hip.aligner import flagstat_text, idxstats_text, stats_text
    from bwamem_hip.lib import bam_stats
    for what, nc, stream, cap in corpus():
        want = cached_model(what, stream, nc, cap)
        if isinstance(want, tuple):
            with pytest.raises(ValueError) as e:
                bam_stats(stream, nc, cap, host=True)
            assert str(e.value) == "bmh_bam_stats: " + refusal_words("bmh_bam_stats_host", want[1], want[2]), what
            continue
        got = bam_stats(stream, nc, cap, host=True)
        assert equal(got, want), what
        contigs = [("c%d" % i, 1000 * (i + 1)) for i in range(nc)]
        assert flagstat_text(got) == flagstat_by_model(want) and idxstats_text(got, contigs) == idxstats_by_model(want, contigs) and stats_text(got, contigs) == stats_by_model(want, contigs), what
    # no result depends on the order of the records
    nc, s = synthetic()
    assert equal(bam_stats(py_sort(s), nc, 4, host=True), cached_model("synthetic", s, nc, 4))
    assert equal(bam_stats(b"".join(reversed(split_records(s))), nc, 4, host=True), cached_model("synthetic", s, nc, 4))


def test_records_that_are_not_walked():
    """an unmapped, a secondary and a supplementary record with damaged tags, an NM of type Z and the placeholder's shape are counted, not refused"""
    from bwamem_hip.lib import bam_stats
    bad = [b"NMZab", b"XA", b"NMZ1\0", b"CGBI" + struct.pack("<I", 2) + b"\0" * 8]
    s = b"".join(srec(b"n%d%d" % (k, j), flag=fl, ops=((50, S), (80, N)), l_seq=50, tag=t) for k, fl in enumerate((0x4, 0x100, 0x800, 0x904)) for j, t in enumerate(bad))
    got = bam_stats(s, 1, host=True)
    assert equal(got, model(s, 1)) and got["flag"][0][:4].tolist() == [16, 4, 8, 4] and got["summary"][:4].tolist() == [4, 200, 0, 0]


def test_empty_stream_and_texts_by_hand(tmp_path):
    from bwamem_hip.aligner import flagstat_text, idxstats_text, stats_text
    from bwamem_hip.lib import bam_stats
    contigs = [("chrA", 1000), ("chrB", 30)]
    got = bam_stats(b"", 2, host=True)
    assert all(not v.any() for v in got.values()) and got["insert_hist"].shape == (3, 65537)
    assert flagstat_text(got).split("\n")[6:8] == ["0 + 0 mapped (N/A : N/A)", "0 + 0 primary mapped (N/A : N/A)"] and flagstat_text(got).count("N/A") == 8
    assert idxstats_text(got, contigs) == "chrA\t1000\t0\t0\nchrB\t30\t0\t0\n*\t0\t0\t0\n"
    assert stats_text(got, contigs).split("\n")[-3:] == ["SN\tedit_distance\t0", "SN\terror_rate\t0", ""]
    fwd = 0x1 | 0x80 | 0x20
    s = b"".join([srec(b"p", flag=0x1 | 0x2 | 0x40 | 0x20, nrid=0, tlen=200, mapq=60, tag=nm("C", 2)), srec(b"p", pos=160, flag=0x1 | 0x2 | 0x80 | 0x10, nrid=0, npos=10, tlen=-200, mapq=60, tag=nm("C", 1)),
                  srec(b"q", flag=fwd | 0x2, nrid=0, tlen=3, mapq=0), srec(b"q", rid=1, pos=0, flag=0x1 | 0x4 | 0x40 | 0x200, nrid=1), srec(b"u", rid=-1, pos=-1, flag=0x4),
                  srec(b"w", flag=fwd, nrid=0, tlen=-9), srec(b"s", flag=0x800 | 0x400)])
    got = bam_stats(s, 2, insert_cap=4, host=True)
    assert flagstat_text(got) == ("6 + 1 in total (QC-passed reads + QC-failed reads)\n5 + 1 primary\n0 + 0 secondary\n1 + 0 supplementary\n1 + 0 duplicates\n0 + 0 primary duplicates\n"
                                  "5 + 0 mapped (83.33% : 0.00%)\n4 + 0 primary mapped (80.00% : 0.00%)\n4 + 1 paired in sequencing\n1 + 1 read1\n3 + 0 read2\n3 + 0 properly paired (75.00% : 0.00%)\n"
                                  "4 + 0 with itself and mate mapped\n0 + 0 singletons (0.00% : 0.00%)\n0 + 0 with mate mapped to a different chr\n0 + 0 with mate mapped to a different chr (mapQ>=5)\n")
    assert idxstats_text(got, contigs) == "chrA\t1000\t5\t0\nchrB\t30\t0\t1\n*\t0\t0\t1\n"
    text = stats_text(got, contigs)
    assert [l for l in text.split("\n") if l[:2] in ("IS", "IM", "MQ")] == ["MQ\t0\t1", "MQ\t30\t1", "MQ\t60\t2", "IS\t3\t1\t0\t0", "IS\t4+\t1\t1\t0",
                                                                            "IM\tFR\t2\t3.5\t0.5\t3\t3\t200\t3.00\t0.00", "IM\tRF\t1\t4.0\t0.0\t4\t9\t9\t0.00\t0.00"]
    assert "FS\ttotal\t6\t1\n" in text and "IX\tchrB\t30\t0\t1\n" in text and "SN\tbases_aligned\t200\n" in text and "SN\tedit_distance\t3\n" in text and "SN\terror_rate\t1.500000e-02\n" in text
    assert text == stats_by_model(model(s, 2, 4), contigs)
    out = io.StringIO()
    from bwamem_hip.aligner import write_flagstat, write_idxstats, write_stats, write_stats_texts
    write_stats_texts(dict(flagstat=out, idxstats=None, stats=None), got, contigs)
    assert out.getvalue() == flagstat_text(got)
    paths = [str(tmp_path / n) for n in ("f.txt", "i.txt", "s.txt")]                # the three writers take a path or a file object
    write_flagstat(got, paths[0]); write_idxstats(got, contigs, paths[1]); write_stats(got, contigs, paths[2])
    assert [open(p).read() for p in paths] == [flagstat_text(got), idxstats_text(got, contigs), text]
    out = io.StringIO()
    write_stats(got, contigs, out)
    assert out.getvalue() == text


def test_insert_size_metrics_by_hand():
    import bwamem_hip
    from bwamem_hip.aligner import insert_size_metrics
    assert bwamem_hip.insert_size_metrics([0, 0, 1, 0], 2, 2) == insert_size_metrics([0, 0, 1, 0], 2, 2)
    h = np.zeros(11, dtype=np.uint64)
    h[[2, 3, 7]] = [1, 3, 1]                                                   # 2 3 3 3 7: odd
    assert insert_size_metrics(h, 2, 7) == dict(pairs=5, median=3.0, mad=0.0, mode=3, min=2, max=7, mean=2.75, sd=0.5)      # the trim at 3 + 10 * 0 cuts the 7
    h[:] = 0; h[[1, 2, 4, 9]] = 1                                              # 1 2 4 9: even -- median 3, deviations 2 1 1 6 -> 1.5
    m = insert_size_metrics(h, 1, 9)
    assert (m["median"], m["mad"], m["mode"], m["pairs"]) == (3.0, 1.5, 1, 4) and m["mean"] == 4.0 and abs(m["sd"] - (38 / 3) ** 0.5) < 1e-12
    h[:] = 0; h[5] = 1                                                         # one value
    assert insert_size_metrics(h, 5, 5) == dict(pairs=1, median=5.0, mad=0.0, mode=5, min=5, max=5, mean=5.0, sd=0.0)
    h[:] = 0; h[[3, 10]] = [1, 4]                                              # the median inside the overflow bin: taken as the cap; mean and SD over the sizes below it
    assert insert_size_metrics(h, 3, 70000) == dict(pairs=5, median=10.0, mad=0.0, mode=10, min=3, max=70000, mean=3.0, sd=0.0)
    h[:] = 0; h[[3, 4, 10]] = [1, 1, 6]
    m = insert_size_metrics(h, 3, 12)
    assert (m["median"], m["mad"], m["mean"], m["sd"]) == (10.0, 0.0, 3.5, 0.5 ** 0.5)
    h[:] = 0; h[[2, 3, 4, 9]] = [2, 2, 2, 1]                                   # the trim keeps median + 10 MAD = 3 + 10 = 13 -> the cap - 1 = 9 bounds it: all kept
    m = insert_size_metrics(h, 2, 9)
    assert (m["median"], m["mad"], m["mean"]) == (3.0, 1.0, 27 / 7)
    assert insert_size_metrics(np.zeros(5, dtype=np.uint64), 0, 0)["pairs"] == 0
    for what, nc, stream, cap in corpus():
        m = cached_model(what, stream, nc, cap)
        if isinstance(m, dict) and cap == 4:
            for o in range(3):
                want = metrics_by_model(m["insert_hist"][o], m["insert_min"][o], m["insert_max"][o])
                if want:
                    got = insert_size_metrics(m["insert_hist"][o], m["insert_min"][o], m["insert_max"][o])
                    assert all(abs(got[k] - want[k]) < 1e-9 for k in want), (what, o)


def test_refusals_and_keywords(capsys):
    from bwamem_hip.lib import bam_sorted_file, bam_stats
    ok = srec(b"ok")
    for what, r, code in REFUSED:
        r = cut(r) if what == "bases past the record" else r
        with pytest.raises(ValueError) as e:
            bam_stats(ok + ok + r + srec(b"late", rid=5), 2, host=True)                  # the first refused record is the one named, whatever its kind
        assert str(e.value) == "bmh_bam_stats: bmh_bam_stats_host: record 2 " + WORDS[code], what
    with pytest.raises(ValueError, match="begin no whole BAM record"):
        bam_stats(ok[:-1], 2, host=True)
    for cap in (1, 0, 65537, -1, True, 2.5):
        with pytest.raises(ValueError, match="insert_cap"):
            bam_stats(b"", 1, insert_cap=cap, host=True)
        with pytest.raises(ValueError, match="insert_cap"):
            bam_sorted_file("@CO\tx\n", [("c", 100)], b"", host=True, stats=dict(insert_cap=cap))
    assert bam_stats(b"", 1, insert_cap=2, host=True)["insert_hist"].shape == (3, 3)
    with pytest.raises(ValueError, match="bmh_bam_sorted_file_host: record 1 has an NM tag that is no count"):
        bam_sorted_file("@CO\tx\n", [("c", 1000)], srec(b"b", pos=20, tag=b"NMZ1\0") + ok, host=True, stats={})       # (the index in the sorted file)
    from bwamem_hip import bam, mem
    capsys.readouterr()
    for argv, msg in ((["--flagstat", "f.txt", "p", "r.fa"], "need --sort"), (["--idxstats", "i.txt", "p", "r.fa"], "need --sort"), (["--stats", "s.txt", "p", "r.fa"], "need --sort"),
                      (["--sort", "--stats"], "option --stats needs a value")):
        assert mem.main(argv) == 2, argv
        assert msg in capsys.readouterr().err, argv
    assert bam.main(["--flagstat"]) == 2 and "option --flagstat needs a value" in capsys.readouterr().err
    from bwamem_hip.aligner import Aligner
    al = Aligner.__new__(Aligner)                                         # the keyword checks come before anything touches an index or a device
    al.profile = False
    for call in (lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", flagstat=io.StringIO()),                                   # the statistics need sort
                 lambda: al.align_files("r.fa", out=io.BytesIO(), idxstats=io.StringIO()),
                 lambda: al.align_groups([("@RG\tID:a", "r.fa")], out=io.BytesIO(), stats=io.StringIO()),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, insert_cap=100),                           # a modifier without an output
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, stats=io.StringIO(), insert_cap=1),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, stats=io.StringIO(), insert_cap=65537),
                 lambda: bam.bam_post_file("x.bam", io.BytesIO(), host=True, flagstat=io.StringIO(), insert_cap=0),
                 lambda: bam.bam_post_file("x.bam", io.BytesIO(), host=True, insert_cap=100)):
        with pytest.raises(ValueError):
            call()
    assert getattr(al, "_stats_req", None) is None and getattr(al, "_out_fmt", ("sam", 1)) == ("sam", 1)


@pytest.mark.parametrize("window", [0, 1, 7, 25])
def test_windows_of_the_host_merge(window):
    """the file and its index are those of the run without statistics; the statistics are the model's over the records of the file just written -- with markdup,
    over its final 0x400 flags; the contig counts are the index's metadata words"""
    from bwamem_hip.lib import bam_sorted_file
    from test_bam_dup import one_key
    nc, s = synthetic(400, 5)
    contigs = [("c%d" % i, 3000) for i in range(nc)]
    plain = bam_sorted_file("@CO\tx\n", contigs, s, 1, window, host=True)
    for cap in (4, 65536):
        bam, bai, got = bam_sorted_file("@CO\tx\n", contigs, s, 1, window, host=True, stats=dict(insert_cap=cap))
        assert (bam, bai) == plain and BamFile(bam).stream == py_sort(s)
        assert equal(got, model(BamFile(bam).stream, nc, cap)), (window, cap)
    refs, no_coor = parse_bai(bai)
    for c, (bins, _lin) in enumerate(refs):
        words = bins[37450][1] if 37450 in bins else (0, 0)
        assert (int(got["contig_mapped"][c]), int(got["contig_unmapped"][c])) == tuple(words), c
    assert no_coor == int(got["unplaced"][0]) > 0
    dups = one_key(40)
    contigs = [("a", 1000), ("b", 2000)]
    plain = bam_sorted_file("@CO\tx\n", contigs, dups, 1, window, host=True, markdup=True, coverage={})
    bam, bai, counts, cov, got = bam_sorted_file("@CO\tx\n", contigs, dups, 1, window, host=True, markdup=True, coverage={}, stats={})
    assert (bam, bai, counts) == plain[:3] and all(np.array_equal(cov[k], plain[3][k]) for k in cov)
    assert counts["records_flagged"] > 0 and int(got["flag"][0][4]) == counts["records_flagged"] and equal(got, model(BamFile(bam).stream, 2))
    unmarked = bam_sorted_file("@CO\tx\n", contigs, dups, 1, window, host=True, stats={})[2]
    assert int(unmarked["flag"][0][4]) == 0 and int(got["flag"][0][5]) > 0


def test_bam_post_file_on_the_host(tmp_path):
    """python -m bwamem_hip.bam --host with the three options: the texts are the model's over the records of the file it wrote, which is the file without them"""
    from bwamem_hip import bam
    from bwamem_hip.lib import bam_stats, bgzf_compress
    from test_bam_dup import one_key
    recs = one_key(40)
    header = "@SQ\tSN:a\tLN:1000\n@SQ\tSN:b\tLN:2000\n"
    raw = b"BAM\1" + struct.pack("<I", len(header)) + header.encode() + struct.pack("<I", 2) + b"".join(struct.pack("<I", len(n) + 1) + n + b"\0" + struct.pack("<I", l) for n, l in ((b"a", 1000), (b"b", 2000)))
    src = tmp_path / "in.bam"
    src.write_bytes(bgzf_compress(raw + recs, host=True))
    paths = [str(tmp_path / n) for n in ("f.txt", "i.txt", "s.txt")]
    assert bam.main(["--host", "--markdup", "--flagstat", paths[0], "--idxstats", paths[1], "--stats", paths[2], str(src), "-o", str(tmp_path / "out.bam")]) == 0
    assert bam.main(["--host", "--markdup", str(src), "-o", str(tmp_path / "plain.bam")]) == 0
    out = (tmp_path / "out.bam").read_bytes()
    assert out == (tmp_path / "plain.bam").read_bytes() and (tmp_path / "out.bam.bai").read_bytes() == (tmp_path / "plain.bam.bai").read_bytes()
    want = model(BamFile(out).stream, 2)
    contigs = [("a", 1000), ("b", 2000)]
    assert int(want["flag"][0][4]) > 0
    assert [open(p).read() for p in paths] == [flagstat_by_model(want), idxstats_by_model(want, contigs), stats_by_model(want, contigs)]
    assert equal(bam_stats(BamFile(out).stream, 2, host=True), want)


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_stats_core_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_stats_core_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_stats_core.h", "bam_stats.h", "bam_stats_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(tmp_path, cases):
    """cases: (n_contigs, stream, cap, window) -> (status, refused index, code, results or None) each"""
    fi, fo = str(tmp_path / "stats_case.bin"), str(tmp_path / "stats_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for nc, s, cap, window in cases:
            f.write(struct.pack("<IIIQ", nc, cap, window, len(s)) + s)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    res = np.fromfile(fo, dtype=np.uint8).tobytes()
    out, p = [], 0
    for nc, _s, cap, _w in cases:
        rc, index, code = struct.unpack_from("<iQi", res, p); p += 16
        if rc != 0:
            out.append((rc, index, code, None))
            continue
        w = np.frombuffer(res, dtype=np.uint64, count=309 + 2 * nc + 3 * (cap + 1), offset=p).copy(); p += 8 * len(w)
        d = dict(flag=w[:32].reshape(2, 16), summary=w[32:46], mapq=w[46:302], insert_min=w[302:305], insert_max=w[305:308], unplaced=w[308:309], contig_mapped=w[309:309 + nc],
                 contig_unmapped=w[309 + nc:309 + 2 * nc], insert_hist=w[309 + 2 * nc:].reshape(3, cap + 1))
        out.append((0, 0, 0, d))
    assert p == len(res)
    return out


def test_core_under_sanitizers(tmp_path):
    cases, want = [], []
    for what, nc, stream, cap in corpus():
        for window in (0, 1, 7):
            cases.append((nc, stream, cap, window)); want.append(cached_model(what, stream, nc, cap))
    for case, w, (rc, index, code, got) in zip(cases, want, run_core(tmp_path, cases)):
        if isinstance(w, tuple):
            assert (rc, index, code) == (-2, w[1], w[2]), case[2:]
        else:
            assert rc == 0 and equal(got, w), case[2:]
    bad = [(2, srec(b"a")[:-1], 4, 0), (2, srec(b"a"), 1, 0), (2, srec(b"a"), 65537, 0)]
    assert [rc for rc, *_r in run_core(tmp_path, bad)] == [-2] * len(bad)
    # 1500 damaged streams: bytes of a synthetic stream overwritten or the stream cut -- refused or counted, never out of bounds (tags walked, operations read)
    rng = np.random.default_rng(3)
    nc, s = synthetic(150, 8)
    base = [s, srec(b"a") + placeholder() + placeholder(False) + summary_stream()]
    damaged = []
    for k in range(1500):
        t = bytearray(base[k & 1])
        for _ in range(int(rng.integers(1, 6))):
            t[int(rng.integers(0, len(t)))] = int(rng.integers(0, 256))
        if k % 5 == 0:
            t = t[:int(rng.integers(0, len(t)))]
        damaged.append((nc, bytes(t), 4 if k & 2 else 65536, int(rng.integers(0, 9))))
    res = run_core(tmp_path, damaged)
    assert len(res) == 1500 and all(rc in (0, -2) for rc, *_r in res) and any(rc == 0 for rc, *_r in res) and any(rc == -2 for rc, *_r in res)


_FAILED_CALL = r"""
import ctypes as C, sys
import bwamem_hip
from bwamem_hip.lib import BamStats, BamStatsOpt, Coverage, CoverageOpt, SortedOpt, SortedResults, _sorted_file_api, _u64p
L = _sorted_file_api(bwamem_hip.load_library())
names, lens = (C.c_char_p * 1)(b"c"), (C.c_int32 * 1)(100)
bad_rec = bytes.fromhex(sys.argv[1])
for device in (False, True):
    for header, recs, co, so in ((b"@CO\tx\n", b"", CoverageOpt(0, 0, 0, 0), BamStatsOpt(1)), (b"@CO\tx\n", b"", CoverageOpt(0, 0, 0, 0), BamStatsOpt(65537)), (b"@CO\tx\n", b"", CoverageOpt(0, 0, 0, 5000), BamStatsOpt(4)),
                                 (None, b"", CoverageOpt(0, 0, 0, 0), BamStatsOpt(4)), (b"@CO\tx\n", bad_rec, CoverageOpt(0, 0, 0, 0), BamStatsOpt(4))):
        if device and recs:
            continue                                                # (a refused record is met on the device: test_bam_stats_gpu.py)
        bam, bai, nb, ni, cov, st = C.c_void_p(0xdeadbee0), C.c_void_p(0xdeadbee0), C.c_uint64(7), C.c_uint64(7), Coverage(), BamStats()
        st.flag = C.cast(0xdeadbee0, _u64p); cov.hist = C.cast(0xdeadbee0, _u64p)
        fo, res = SortedOpt(1, 0, 0, 14, 0, None, None, C.pointer(co), C.pointer(so)), SortedResults(None, C.pointer(cov), C.pointer(st))
        head = [header, 1, names, C.addressof(lens), recs, len(recs), C.byref(fo)] + ([None] if device else [])
        rc = (L.bmh_bam_sorted_file_device if device else L.bmh_bam_sorted_file_host)(*head, C.byref(bam), C.byref(nb), C.byref(bai), C.byref(ni), C.byref(res))
        assert rc == -2 and bam.value is None and bai.value is None and not cov.hist and not st.flag and not st.insert_hist and not st.mapq, (device, rc, bam.value, bai.value)
    st = BamStats(); st.flag = C.cast(0xdeadbee0, _u64p)
    L.bmh_bam_stats_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(BamStatsOpt), C.POINTER(BamStats)]
    L.bmh_bam_stats_device.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(BamStatsOpt), C.c_void_p, C.POINTER(BamStats)]
    so = BamStatsOpt(70000)
    rc = L.bmh_bam_stats_device(b"", 0, 1, C.byref(so), None, C.byref(st)) if device else L.bmh_bam_stats_host(b"", 0, 1, C.byref(so), C.byref(st))
    assert rc == -2 and not st.flag
st = BamStats(); st.flag = C.cast(0xdeadbee0, _u64p)
assert L.bmh_bam_stats_host(bad_rec, len(bad_rec), 1, None, C.byref(st)) == -2 and not st.flag and not st.summary
print("ok")
"""


def test_a_failed_call_leaves_null_outputs():
    """a C caller's pointers are not initialised: a call refused before the file exists (an insert_cap out of range, a tile beyond 4096, no header text) or by a
    record must free nothing it did not allocate and leave bam, index and every array of the coverage and the statistics NULL.  The option refusals come before
    anything touches a device, so the device form is called with them as well; a child process, since a free() of such a pointer ends the process"""
    import sys
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(HERE, "..", "bwa-mem_gpu_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-c", _FAILED_CALL, srec(b"x", tag=b"NMZ1\0").hex()], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stdout.decode().strip() == "ok", r.stderr.decode(errors="replace")[-2000:]
