"""Coverage depth of sorted BAM without a GPU: a per-position Python model pinned by a hand-made table, the host form against it at every
(tile, bin), the invariance of the results under tiles and under the windows of the host merge, the refusals word for word, and csrc/bam_cov_core.h with the host
form under AddressSanitizer and UBSan (a stand-alone program, run as a child process)."""
import hashlib
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_dup import rec
from test_bam_sort import make_record, py_sort, split_records

HERE = os.path.dirname(os.path.abspath(__file__))
HIST = 1001
BIG = (1 << 31) - 1
GRID = [(64, 100), (256, 1), (4096, 7), (0, 0)]                 # (tile, bin); tile 0: the default
MAX_BINS = 1 << 28
NAMES = ("n_reads", "cov_bases", "sum_depth", "max_depth", "sum_mapq")


def with_mapq(r: bytes, q: int) -> bytes:
    return r[:13] + bytes([q]) + r[14:]


# ---------------------------------------------------------------------------------------------------------------- the model

def depths(stream: bytes, lens, min_mapq=0, deletions=False):
    """the definition, position by position: ({(contig, position): depth}, counted reads per contig, their mapq sums)"""
    depth, n_reads, sum_mapq = {}, [0] * len(lens), [0] * len(lens)
    for r in split_records(stream):
        rid, pos, l_name, mapq, _bin, n_ops, flag = struct.unpack_from("<iiBBHHH", r, 4)
        if not 0 <= rid < len(lens) or flag & (0x4 | 0x100 | 0x200 | 0x400) or mapq < min_mapq:
            continue
        n_reads[rid] += 1; sum_mapq[rid] += mapq
        x = pos
        for v in struct.unpack_from("<%dI" % n_ops, r, 36 + l_name):
            n, op = v >> 4, v & 15
            if op in (0, 7, 8) or (op == 2 and deletions):
                for p in range(x, min(x + n, lens[rid])):
                    depth[(rid, p)] = depth.get((rid, p), 0) + 1
                x += n
            elif op in (2, 3):
                x += n
    return depth, n_reads, sum_mapq


_MODEL = {}


def model(what, stream, lens, min_mapq=0, deletions=False, bin=0) -> dict:
    """the results as bam_coverage returns them; the depths of (stream, contigs, min_mapq, deletions) are computed once and shared (`what` only names the case)"""
    key = (hashlib.sha256(stream).digest(), tuple(lens), min_mapq, bool(deletions))
    if key not in _MODEL:
        _MODEL[key] = depths(stream, lens, min_mapq, deletions)
    depth, n_reads, sum_mapq = _MODEL[key]
    n = len(lens)
    out = {k: np.zeros(n, dtype=np.uint64) for k in NAMES}
    out["n_reads"][:] = n_reads; out["sum_mapq"][:] = sum_mapq
    hist = [0] * HIST
    bin_off = [0]
    for l in lens:
        bin_off.append(bin_off[-1] + ((l + bin - 1) // bin if bin else 0))
    bins = np.zeros(bin_off[-1], dtype=np.uint64)
    cov, tot, mx = [0] * n, [0] * n, [0] * n
    for (c, p), d in depth.items():
        cov[c] += 1; tot[c] += d; mx[c] = max(mx[c], d)
        hist[min(d, HIST - 1)] += 1
        if bin:
            bins[bin_off[c] + p // bin] += np.uint64(d)
    hist[0] = sum(lens) - len(depth)
    out["cov_bases"][:] = cov; out["sum_depth"][:] = tot; out["max_depth"][:] = mx
    out["hist"] = np.array(hist, dtype=np.uint64); out["bin_sum"] = bins
    return out


def n_bins(lens, bin) -> int:
    return sum((l + bin - 1) // bin for l in lens) if bin else 0


# ---------------------------------------------------------------------------------------------------------------- the table

def table():
    """(what, contig lengths, stream, keywords, must): must = what the model's answer has to hold, spelled out -- {name: list} compared whole, ("hist", d): a bin"""
    M, D, N, S, I, H, EQ, X = 0, 2, 3, 4, 1, 5, 7, 8
    flags = b"".join(rec(b"f%x" % f, 0, 10 * k, f) for k, f in enumerate((0x4, 0x100, 0x200, 0x400, 0x800)))
    mq = with_mapq(rec(b"q", 0, 5, 0), 37)
    stack = b"".join(rec(b"s%04d" % i, 0, 100, 0) for i in range(1100))
    ends = rec(b"first", 0, 0, 0) + rec(b"last", 0, BIG - 50, 0)
    two = rec(b"a", 1, 20, 0, ops=((30, M),)) + rec(b"b", 4, 0, 16, ops=((40, M),))
    return [
        ("one 50M read", [100], rec(b"r", 0, 10, 0), {}, dict(n_reads=[1], cov_bases=[50], sum_depth=[50], max_depth=[1], sum_mapq=[30], h0=50, h1=50)),
        ("10M5D10M, deletions off", [100], rec(b"r", 0, 0, 0, ops=((10, M), (5, D), (10, M))), {}, dict(cov_bases=[20], sum_depth=[20], h0=80)),
        ("10M5D10M, deletions on", [100], rec(b"r", 0, 0, 0, ops=((10, M), (5, D), (10, M))), dict(deletions=True), dict(cov_bases=[25], sum_depth=[25], h0=75)),
        ("10M100N10M", [200], rec(b"r", 0, 5, 0, ops=((10, M), (100, N), (10, M))), dict(deletions=True), dict(cov_bases=[20], sum_depth=[20], max_depth=[1], h0=180)),
        ("5S10M3I10M5H", [100], rec(b"r", 0, 0, 0, ops=((5, S), (10, M), (3, I), (10, M), (5, H))), {}, dict(cov_bases=[20], sum_depth=[20], h1=20)),
        ("= and X", [100], rec(b"r", 0, 3, 0, ops=((10, EQ), (5, X), (10, EQ))), {}, dict(cov_bases=[25], max_depth=[1])),
        ("flags 0x4 0x100 0x200 0x400 out, 0x800 in", [200], flags, {}, dict(n_reads=[1], cov_bases=[50], sum_depth=[50], sum_mapq=[30])),
        ("min_mapq at the record's", [100], mq, dict(min_mapq=37), dict(n_reads=[1], cov_bases=[50], sum_mapq=[37])),
        ("min_mapq below the record's", [100], mq, dict(min_mapq=36), dict(n_reads=[1], cov_bases=[50])),
        ("min_mapq above the record's", [100], mq, dict(min_mapq=38), dict(n_reads=[0], cov_bases=[0], sum_mapq=[0], h0=100)),
        ("no CIGAR", [100], rec(b"r", 0, 7, 0, ops=(), l_seq=50), {}, dict(n_reads=[1], cov_bases=[0], sum_depth=[0], max_depth=[0], h0=100)),
        ("clamped at the contig's end", [100], rec(b"r", 0, 80, 0), {}, dict(n_reads=[1], cov_bases=[20], sum_depth=[20], h0=80)),
        ("the last base of contig 0 beside base 0 of contig 1", [100, 100], rec(b"a", 0, 50, 0) + rec(b"b", 1, 0, 0), {},
         dict(cov_bases=[50, 50], max_depth=[1, 1], sum_depth=[50, 50], h0=100, h1=100, h2=0)),
        ("clamped at the end of contig 0, reads at base 0 and in the middle of contig 1", [100, 300], rec(b"a", 0, 80, 0) + rec(b"b", 1, 0, 0) + rec(b"c", 1, 200, 0), {},
         dict(n_reads=[1, 2], cov_bases=[20, 100], sum_depth=[20, 100], max_depth=[1, 1], h0=280, h1=120, h2=0)),
        ("empty first contig, contigs of no bases and of no reads in the middle", [70, 100, 0, 60, 100], two, {},
         dict(n_reads=[0, 1, 0, 0, 1], cov_bases=[0, 30, 0, 0, 40], max_depth=[0, 1, 0, 0, 1], h0=260)),
        ("empty stream", [100, 50], b"", {}, dict(n_reads=[0, 0], cov_bases=[0, 0], sum_depth=[0, 0], max_depth=[0, 0], sum_mapq=[0, 0], h0=150, h1=0)),
        ("1100 identical reads", [1000], stack, {}, dict(n_reads=[1100], cov_bases=[50], sum_depth=[55000], max_depth=[1100], h0=950, h999=0, h1000=50)),
        ("one 1000M read, tile 64", [2000], rec(b"r", 0, 3, 0, ops=((1000, M),)), dict(tile=64), dict(cov_bases=[1000], sum_depth=[1000], max_depth=[1], h0=1000)),
        ("the two ends of 2^31 - 1 bases", [BIG], ends, {}, dict(n_reads=[2], cov_bases=[100], sum_depth=[100], max_depth=[1], h0=BIG - 100, h1=100)),
    ]


def synthetic(n=2000, seed=5) -> tuple:
    """about 2000 records over three contigs in coordinate order: mixed operations, a quarter filtered by flag, some marked 0x400, every mapq, reads over the ends"""
    rng = np.random.default_rng(seed)
    lens = [3000, 1200, 2500]
    M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
    shapes = [((50, M),), ((5, S), (20, M), (2, I), (25, M)), ((20, M), (7, D), (30, M)), ((15, M), (200, N), (35, M)), ((10, EQ), (1, X), (39, EQ)), ((3, H), (60, M), (4, S)),
              ((30, M), (1, D), (1, I), (2, D), (20, M)), ((120, M),), ()]
    out = []
    for i in range(n):
        rid = int(rng.integers(0, 3))
        pos = int(rng.integers(0, lens[rid]))
        if i % 3 == 0:
            pos = int(rng.integers(0, 300))                                     # dense: deep stacks, equal starts
        flag = int(rng.choice([0, 16, 0x800, 0x810])) if i % 4 else int(rng.choice([0x4, 0x100, 0x200, 0x104]))
        if i % 11 == 0:
            flag |= 0x400
        ops = shapes[int(rng.integers(0, len(shapes)))]
        out.append(with_mapq(rec(b"x%04d" % i, rid, pos, flag, ops=ops, l_seq=None if ops else 30), int(rng.integers(0, 61))))
    out.append(rec(b"noref", -1, -1, 4, ops=(), l_seq=20))
    return lens, py_sort(b"".join(out))


_CORPUS = []


def corpus():
    if not _CORPUS:
        _CORPUS.extend(table())
        lens, s = synthetic()
        _CORPUS.append(("synthetic", lens, s, {}, {}))
    return _CORPUS


def check_must(what, m: dict, must: dict):
    for k, v in must.items():
        if k[0] == "h" and k[1:].isdigit():
            assert int(m["hist"][int(k[1:])]) == v, (what, k, int(m["hist"][int(k[1:])]))
        else:
            assert [int(x) for x in m[k]] == v, (what, k, m[k])
    assert int(m["hist"].sum()) == sum(int(x) for x in m["cov_bases"]) + int(m["hist"][0])


def equal(a: dict, b: dict) -> bool:
    return set(a) == set(b) and all(a[k].dtype == np.uint64 and np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------- the texts, formatted here

def table_text(m, contigs):
    def row(name, ln, reads, covb, sumd, maxd, mapq):
        return "\t".join([name, "1", str(ln), str(reads), str(covb), "%.6g" % (100.0 * covb / ln if ln else 0), "%.6g" % (sumd / ln if ln else 0), str(maxd), "%.6g" % (mapq / reads if reads else 0)])
    rows = ["#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmaxdepth\tmeanmapq"]
    rows += [row(nm, ln, *(int(m[k][c]) for k in ("n_reads", "cov_bases", "sum_depth", "max_depth", "sum_mapq"))) for c, (nm, ln) in enumerate(contigs)]
    rows.append(row("total", sum(l for _n, l in contigs), int(m["n_reads"].sum()), int(m["cov_bases"].sum()), int(m["sum_depth"].sum()), int(m["max_depth"].max()) if len(contigs) else 0,
                    int(m["sum_mapq"].sum())))
    return "\n".join(rows) + "\n"


def hist_text(m):
    h = [int(v) for v in m["hist"]]
    rows = ["depth\tbases\tfraction_at_or_above"]
    for d in range(HIST):
        rows.append("%s\t%d\t%.6f" % ("1000+" if d == 1000 else d, h[d], sum(h[d:]) / sum(h) if sum(h) else 0))
    return "\n".join(rows) + "\n"


def bed_text(m, contigs, bin):
    rows, k = [], 0
    for nm, ln in contigs:
        for a in range(0, ln, bin):
            rows.append("%s\t%d\t%d\t%.2f\n" % (nm, a, min(a + bin, ln), int(m["bin_sum"][k]) / (min(a + bin, ln) - a))); k += 1
    return "".join(rows)


# ---------------------------------------------------------------------------------------------------------------- tests

def test_model_on_the_table():
    for what, lens, stream, kw, must in table():
        assert must, what
        check_must(what, model(what, stream, lens, kw.get("min_mapq", 0), kw.get("deletions", False), 7 if sum(lens) < 10_000 else 0), must)
    lens, s = synthetic()
    m = model("synthetic", s, lens)
    recs = split_records(s)
    assert 1900 <= len(recs) <= 2100 and 0.2 < sum(1 for r in recs if struct.unpack_from("<H", r, 18)[0] & 0x304) / len(recs) < 0.3
    assert sum(1 for r in recs if struct.unpack_from("<H", r, 18)[0] & 0x400) > 100 and all(int(v) for v in m["n_reads"]) and int(m["max_depth"].max()) >= 30
    assert not equal(m, model("synthetic", s, lens, 20, False)) and not equal(m, model("synthetic", s, lens, 0, True))


def test_host_equals_model():
    from bwamem_hip.aligner import coverage_bed_text, coverage_hist_text, coverage_table_text
    from bwamem_hip.lib import bam_coverage
    for what, lens, stream, kw, must in corpus():
        contigs = [("c%d" % i, l) for i, l in enumerate(lens)]
        mq, dl = kw.get("min_mapq", 0), kw.get("deletions", False)
        check_must(what, bam_coverage(stream, contigs, host=True, **kw), must)
        for tile, bin in GRID:
            if n_bins(lens, bin) >= MAX_BINS:
                with pytest.raises(ValueError, match="fewer than 2\\^28"):
                    bam_coverage(stream, contigs, host=True, min_mapq=mq, deletions=dl, bin=bin, tile=tile)
                continue
            want = model(what, stream, lens, mq, dl, bin)
            got = bam_coverage(stream, lens, host=True, min_mapq=mq, deletions=dl, bin=bin, tile=tile)
            assert equal(got, want), (what, tile, bin)
            assert coverage_table_text(got, contigs) == table_text(want, contigs) and coverage_hist_text(got) == hist_text(want), (what, tile, bin)
            if bin and n_bins(lens, bin) < 100_000:
                assert coverage_bed_text(got, contigs, bin) == bed_text(want, contigs, bin), (what, tile, bin)
    lens, s = synthetic()
    for mq, dl in ((20, False), (0, True), (20, True)):
        assert equal(bam_coverage(s, lens, host=True, min_mapq=mq, deletions=dl, bin=100, tile=64), model("synthetic", s, lens, mq, dl, 100))


def test_texts_by_hand():
    from bwamem_hip.aligner import coverage_bed_text, coverage_hist_text, coverage_table_text
    from bwamem_hip.lib import bam_coverage
    contigs = [("chrA", 100), ("none", 0), ("chrB", 30)]
    got = bam_coverage(rec(b"a", 0, 10, 0) + rec(b"b", 0, 20, 0, ops=((10, 0), (5, 2), (10, 0))), contigs, host=True, bin=50)
    assert coverage_table_text(got, contigs) == ("#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmaxdepth\tmeanmapq\n"
                                                  "chrA\t1\t100\t2\t50\t50\t0.7\t2\t30\nnone\t1\t0\t0\t0\t0\t0\t0\t0\nchrB\t1\t30\t0\t0\t0\t0\t0\t0\ntotal\t1\t130\t2\t50\t38.4615\t0.538462\t2\t30\n")
    lines = coverage_hist_text(got).split("\n")
    assert lines[:4] == ["depth\tbases\tfraction_at_or_above", "0\t80\t1.000000", "1\t30\t0.384615", "2\t20\t0.153846"] and lines[1001] == "1000+\t0\t0.000000" and len(lines) == 1003
    assert coverage_bed_text(got, contigs, 50) == "chrA\t0\t50\t1.20\nchrA\t50\t100\t0.20\nchrB\t0\t30\t0.00\n"


def test_invariance():
    """no result depends on the tile, nor on where the merge of the sorted file cuts its windows (the host merge of bam_sorted_file)"""
    from bwamem_hip.lib import bam_coverage, bam_sorted_file
    lens, s = synthetic()
    contigs = [("c%d" % i, l) for i, l in enumerate(lens)]
    for dl in (False, True):
        want = model("synthetic", s, lens, 0, dl, 100)
        for tile in (1, 3, 64, 256, 4096, 0):
            assert equal(bam_coverage(s, contigs, host=True, deletions=dl, bin=100, tile=tile), want), tile
        plain = bam_sorted_file("@CO\tx\n", contigs, s, 1, 7, host=True)
        for window in (1, 7, 25, 0):
            for tile in (64, 0):
                bam, bai, got = bam_sorted_file("@CO\tx\n", contigs, s, 1, window, host=True, coverage=dict(deletions=dl, bin=100, tile=tile))
                assert equal(got, want), (window, tile)
                assert window != 7 or (bam, bai) == plain
    # the table's streams window by window: a carry over every window edge, the stack of 1100 cut inside, the contig edge between two windows
    for what, lens, stream, kw, _must in table():
        if max(lens) >= 1 << 29:
            continue                                                            # (a BAI index holds no such contig: the stand-alone program below cuts it)
        contigs = [("c%d" % i, l) for i, l in enumerate(lens)]
        opt = dict(min_mapq=kw.get("min_mapq", 0), deletions=kw.get("deletions", False), bin=7, tile=kw.get("tile", 64))
        for window in (1, 7, 25):
            assert equal(bam_sorted_file("@CO\tx\n", contigs, stream, 1, window, host=True, coverage=opt)[2], model(what, stream, lens, opt["min_mapq"], opt["deletions"], 7)), (what, window)


def test_marked_duplicates_are_counted_out_on_the_host():
    from bwamem_hip.lib import bam_sorted_file
    from test_bam_dup import one_key
    contigs = [("a", 1000), ("b", 2000)]
    s = one_key(40)
    _b, _i, counts, marked = bam_sorted_file("@CO\tx\n", contigs, s, 1, 7, host=True, markdup=True, coverage={})
    _b, _i, plain = bam_sorted_file("@CO\tx\n", contigs, s, 1, 7, host=True, coverage={})
    assert counts["records_flagged"] > 0 and int(plain["n_reads"].sum()) - int(marked["n_reads"].sum()) == counts["records_flagged"]
    assert int(marked["sum_depth"].sum()) == int(plain["sum_depth"].sum()) - 50 * counts["records_flagged"]


def placeholder(with_tag=True, pos=10) -> bytes:
    tag = b"CGBI" + struct.pack("<I", 2) + struct.pack("<II", 50 << 4, 30 << 4) if with_tag else b""
    return make_record(0, pos, 0, b"long", ops=((50, 4), (80, 3)), l_seq=50, tag=b"NMi" + struct.pack("<i", 3) + b"XAZab\0" + tag)


def test_refusals(capsys):
    from bwamem_hip.lib import bam_coverage
    a, b = rec(b"a", 0, 10, 0), rec(b"b", 0, 9, 0)
    with pytest.raises(ValueError, match="bmh_bam_coverage_host: record 1 lies before record 0: coverage takes records in coordinate order"):
        bam_coverage(a + b, [100], host=True)
    with pytest.raises(ValueError, match="record 2 lies before record 1"):
        bam_coverage(rec(b"a", 1, 10, 0) + rec(b"u", -1, -1, 4, ops=(), l_seq=5) + rec(b"b", 1, 20, 0), [100, 100], host=True)
    with pytest.raises(ValueError, match=r"bmh_bam_coverage_host: record 1 begins outside its contig \(pos is negative or not below the contig's length\)"):
        bam_coverage(a + rec(b"b", 0, 100, 0), [100], host=True)
    with pytest.raises(ValueError, match="record 0 begins outside its contig"):
        bam_coverage(rec(b"b", 0, -1, 0), [100], host=True)
    assert int(bam_coverage(rec(b"b", 0, 100, 0x400), [100], host=True)["n_reads"][0]) == 0        # (a record that does not count is not checked)
    with pytest.raises(ValueError, match=r"bmh_bam_coverage_host: record 1 holds the long-CIGAR placeholder \(its operations are in its CG tag\): coverage reads the record's own operations"):
        bam_coverage(a + placeholder(), [200], host=True)
    got = bam_coverage(a + placeholder(False), [200], host=True)                                  # (kSmN without the tag is a read that covers nothing)
    assert [int(got["n_reads"][0]), int(got["cov_bases"][0])] == [2, 50]
    # two refusals in one stream: the first record refused is the one named, whatever its kind
    with pytest.raises(ValueError, match="record 1 begins outside its contig"):
        bam_coverage(a + rec(b"b", 0, 100, 0) + rec(b"c", 0, 5, 0), [100], host=True)
    with pytest.raises(ValueError, match="record 1 lies before record 0"):
        bam_coverage(a + rec(b"c", 0, 5, 0) + rec(b"b", 0, 100, 0), [100], host=True)
    with pytest.raises(ValueError, match=r"bmh_bam_coverage_host: 2147483647 bins of 1 bases \(fewer than 2\^28\): choose a larger bin"):
        bam_coverage(b"", [BIG], host=True, bin=1)
    with pytest.raises(ValueError, match="268435456 bins of 8 bases"):                              # (2^28 exactly)
        bam_coverage(b"", [BIG], host=True, bin=8)
    assert len(bam_coverage(b"", [1 << 20, 5], host=True, bin=1)["bin_sum"]) == (1 << 20) + 5
    for kw in (dict(min_mapq=256), dict(min_mapq=-1), dict(tile=4097), dict(bin=-1), dict(bin=1 << 32), dict(tile=True)):
        with pytest.raises(ValueError):
            bam_coverage(b"", [100], host=True, **kw)
    with pytest.raises(ValueError, match="begin no whole BAM record"):
        bam_coverage(a[:-1], [100], host=True)
    from bwamem_hip import mem
    capsys.readouterr()
    for argv, msg in ((["--coverage", "c.txt", "p", "r.fa"], "need --sort"), (["--coverage-hist", "h.txt", "p", "r.fa"], "need --sort"),
                      (["--coverage-bed", "b", "--coverage-bin", "10", "p", "r.fa"], "need --sort"), (["--coverage-min-mapq", "3", "p", "r.fa"], "need --sort"),
                      (["--coverage-deletions", "p", "r.fa"], "need --sort"),
                      (["--sort", "--coverage-bed", "b.bed", "p", "r.fa"], "--coverage-bed and --coverage-bin go together"),
                      (["--sort", "--coverage", "c", "--coverage-bin", "10", "p", "r.fa"], "--coverage-bed and --coverage-bin go together"),
                      (["--sort", "--coverage-min-mapq", "3", "p", "r.fa"], "--coverage-min-mapq and --coverage-deletions need --coverage, --coverage-hist or --coverage-bed"),
                      (["--sort", "--coverage-deletions", "p", "r.fa"], "--coverage-min-mapq and --coverage-deletions need --coverage, --coverage-hist or --coverage-bed"),
                      (["--sort", "--coverage", "c", "--coverage-min-mapq", "256", "p", "r.fa"], "option --coverage-min-mapq needs a whole number, 0 .. 255"),
                      (["--sort", "--coverage", "c", "--coverage-min-mapq", "-1", "p", "r.fa"], "option --coverage-min-mapq needs a whole number, 0 .. 255"),
                      (["--sort", "--coverage-bed", "b", "--coverage-bin", "0", "p", "r.fa"], "option --coverage-bin needs a whole number of positions, 1 .. 2^32 - 1"),
                      (["--sort", "--coverage"], "option --coverage needs a value")):
        assert mem.main(argv) == 2, argv
        assert msg in capsys.readouterr().err, argv


def test_python_keywords():
    from bwamem_hip.aligner import Aligner
    al = Aligner.__new__(Aligner)                                         # the keyword checks come before anything touches an index or a device
    al.profile = False
    for call in (lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", coverage=io.StringIO()),                                  # coverage needs sort
                 lambda: al.align_files("r.fa", out=io.BytesIO(), coverage_hist=io.StringIO()),
                 lambda: al.align_groups([("@RG\tID:a", "r.fa")], out=io.BytesIO(), coverage_deletions=True),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, coverage_bed=io.StringIO()),             # bed and bin go together
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, coverage=io.StringIO(), coverage_bin=10),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, coverage_min_mapq=3),                    # a modifier without an output
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, coverage=io.StringIO(), coverage_min_mapq=256),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, coverage_bed=io.StringIO(), coverage_bin=0)):
        with pytest.raises(ValueError):
            call()
    assert getattr(al, "_cov_req", None) is None and getattr(al, "_out_fmt", ("sam", 1)) == ("sam", 1)


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_cov_core_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_cov_core_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_cov_core.h", "bam_cov.h", "bam_cov_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(tmp_path, cases):
    """cases: (lens, stream, min_mapq, deletions, bin, tile, window) -> (status, results or None) each"""
    fi, fo = str(tmp_path / "cov_case.bin"), str(tmp_path / "cov_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for lens, s, mq, dl, bin, tile, window in cases:
            f.write(struct.pack("<iiIIII", mq, int(dl), bin, tile, window, len(lens)) + struct.pack("<%di" % len(lens), *lens) + struct.pack("<Q", len(s)) + s)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    res = np.fromfile(fo, dtype=np.uint8).tobytes()
    out, p = [], 0
    for lens, *_rest in cases:
        rc = struct.unpack_from("<i", res, p)[0]; p += 4
        if rc != 0:
            out.append((rc, None))
            continue
        nb = struct.unpack_from("<Q", res, p)[0]; p += 8
        d = {}
        for k, n in [(k, len(lens)) for k in NAMES] + [("hist", HIST), ("bin_sum", nb)]:
            d[k] = np.frombuffer(res, dtype=np.uint64, count=n, offset=p).copy(); p += 8 * n
        out.append((0, d))
    assert p == len(res)
    return out


def test_core_under_sanitizers(tmp_path):
    cases, want = [], []
    for what, lens, stream, kw, _must in corpus():
        mq, dl = kw.get("min_mapq", 0), kw.get("deletions", False)
        for tile, bin in GRID:
            if n_bins(lens, bin) >= 1 << 22:
                bin = 0                                                         # (the bins of 2^31 - 1 bases are the library's test, above)
            for window in (0, 1, 7):
                if window and len(stream) > 100_000 and tile != 64:
                    continue
                cases.append((lens, stream, mq, dl, bin, tile, window)); want.append(model(what, stream, lens, mq, dl, bin))
    res = run_core(tmp_path, cases)
    for case, w, (rc, got) in zip(cases, want, res):
        assert rc == 0 and equal(got, w), case[2:]
    a = rec(b"a", 0, 10, 0)
    bad = [([100], a + rec(b"b", 0, 9, 0), 0, 0, 0, 0, 1), ([100], rec(b"b", 0, 100, 0), 0, 0, 0, 0, 0), ([200], a + placeholder(), 0, 0, 0, 0, 0), ([BIG], b"", 0, 0, 1, 0, 0),
           ([100], a[:-1], 0, 0, 0, 0, 0), ([100], a, 256, 0, 0, 0, 0), ([100], a, 0, 0, 0, 5000, 0)]
    assert [rc for rc, _d in run_core(tmp_path, bad)] == [-2] * len(bad)
    # 1500 damaged streams: bytes of the synthetic stream overwritten or the stream cut -- refused or counted, never out of bounds (tags walked, operations read)
    rng = np.random.default_rng(3)
    lens, s = synthetic(300, 8)
    base = [s, a + placeholder() + placeholder(False)]
    damaged = []
    for k in range(1500):
        t = bytearray(base[k & 1])
        for _ in range(int(rng.integers(1, 6))):
            t[int(rng.integers(0, len(t)))] = int(rng.integers(0, 256))
        if k % 5 == 0:
            t = t[:int(rng.integers(0, len(t)))]
        damaged.append((lens, bytes(t), 0, k & 2, 7, 64, int(rng.integers(0, 9))))
    res = run_core(tmp_path, damaged)
    assert len(res) == 1500 and all(rc in (0, -2) for rc, _d in res) and any(rc == 0 for rc, _d in res) and any(rc == -2 for rc, _d in res)


_FAILED_CALL = r"""
import ctypes as C, sys
import bwamem_hip
from bwamem_hip.lib import Coverage, CoverageOpt, SortedOpt, SortedResults, _sorted_file_api
L = _sorted_file_api(bwamem_hip.load_library())
names, lens = (C.c_char_p * 1)(b"c"), (C.c_int32 * 1)(100)
for device in (False, True):
    for header, opt in ((b"@CO\tx\n", CoverageOpt(0, 0, 0, 5000)), (b"@CO\tx\n", CoverageOpt(300, 0, 0, 0)), (b"@CO\tx\n", CoverageOpt(0, 0, 1, 0)), (None, CoverageOpt(0, 0, 0, 0))):
        bam, bai, nb, ni, cov = C.c_void_p(0xdeadbee0), C.c_void_p(0xdeadbee0), C.c_uint64(7), C.c_uint64(7), Coverage()
        n = 1 if opt.bin == 0 else (1 << 31) - 1                    # (bin 1 on 2^31 - 1 bases: 2^28 bins and more)
        lens[0] = 100 if n == 1 else n
        fo, res = SortedOpt(1, 0, 0, 14, 0, None, None, C.pointer(opt), None), SortedResults(None, C.pointer(cov), None)
        head = [header, 1, names, C.addressof(lens), b"", 0, C.byref(fo)] + ([None] if device else [])
        rc = (L.bmh_bam_sorted_file_device if device else L.bmh_bam_sorted_file_host)(*head, C.byref(bam), C.byref(nb), C.byref(bai), C.byref(ni), C.byref(res))
        assert rc == -2 and bam.value is None and bai.value is None and not cov.hist, (device, rc, bam.value, bai.value)
print("ok")
"""


def test_a_refused_sorted_file_call_leaves_null_outputs():
    """a C caller's bam / index pointers are not initialised: a call refused before the file exists (a tile beyond 4096, min_mapq 300, 2^28 bins, no header text)
    must free nothing and leave them NULL.  The refusals come before anything touches a device, so the device form is called here as well; a child process, since
    a free() of such a pointer ends the process"""
    import sys
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(HERE, "..", "bwa-mem_gpu_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-c", _FAILED_CALL], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stdout.decode().strip() == "ok", r.stderr.decode(errors="replace")[-2000:]
