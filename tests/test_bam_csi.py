"""The CSI index of coordinate-sorted BAM, host forms: the binning scheme of csrc/bam_sort_core.h as plain C++ under AddressSanitizer and UBSan
(tests/bam_csi_core_host.cpp) and the library's host entry points, against a CSI builder, reader and region query written here from the layout alone:

    "CSI\\1"  int32 min_shift  int32 depth  int32 l_aux = 0  int32 n_ref
    per reference: int32 n_bin, per bin (ascending, the pseudo-bin last): uint32 bin  uint64 loffset  int32 n_chunk  n_chunk x (uint64 beg, uint64 end)
    uint64 n_no_coor                                             -- the whole as BGZF members and the end-of-file member

The same cases run on the device in test_bam_csi_gpu.py."""
import bisect
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_sort import BamFile, corpus, fields, make_record, parse_bai, py_sort, split_records

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:1\n"
BIG = (1 << 31) - 1
W = (1 << 30) + (1 << 14)                      # a boundary between two of the deepest bins (depth 6, min_shift 14) that no bin above them shares


# ---------------------------------------------------------------------------------------------------------------- the scheme, from its rules

def depth_of(longest: int, shift: int) -> int:
    """the smallest d >= 0 with 2^(shift + 3 d) >= the longest contig"""
    d = 0
    while (1 << (shift + 3 * d)) < longest:
        d += 1
    return d


def level_first(depth: int, l: int) -> int:
    return ((1 << 3 * (depth - l)) - 1) // 7


def meta_bin(depth: int) -> int:
    return ((1 << 3 * (depth + 1)) - 1) // 7 + 1


def windows(pos: int, end: int, length: int, shift: int):
    """the record's first and last window of 2^shift bases: pos < 0 as 0, clamped to the contig's last window"""
    nw = ((length - 1) >> shift) + 1 if length > 0 else 1
    p0 = max(pos, 0); e0 = max(end, p0 + 1)
    hi = min((e0 - 1) >> shift, nw - 1)
    return min(p0 >> shift, hi), hi


def bin_of(lo: int, hi: int, depth: int) -> int:
    for l in range(depth + 1):
        if lo >> 3 * l == hi >> 3 * l:
            return level_first(depth, l) + (lo >> 3 * l)
    return 0


def rec_bin(rec: bytes, refs, shift: int, depth: int) -> int:
    rid, pos, _b, _fl, end = fields(rec)
    return bin_of(*windows(pos, end, refs[rid][1], shift), depth)


# ---------------------------------------------------------------------------------------------------------------- builder, reader, query

def build_csi(f: BamFile, shift: int) -> bytes:
    """the uncompressed index from the finished file: chunks are maximal runs of records of one (refID, CSI bin); a bin's loffset is the smallest begin offset among
    the records overlapping its first window, or the next window that has one"""
    n_ref = len(f.refs)
    depth = depth_of(max([l for _n, l in f.refs] or [0]), shift)
    bins = [dict() for _ in range(n_ref)]; lin = [dict() for _ in range(n_ref)]; cnt = [[0, 0] for _ in range(n_ref)]; span = [None] * n_ref
    no_coor, prev = 0, None
    for i, rec in enumerate(f.recs):
        rid, pos, _bin, flag, end = fields(rec)
        b, e = f.voff(f.upos[i]), f.voff(f.upos[i + 1])
        if rid < 0:
            no_coor += 1; prev = None
            continue
        lo, hi = windows(pos, end, f.refs[rid][1], shift)
        k = bin_of(lo, hi, depth)
        if prev == (rid, k):
            bins[rid][k][-1][1] = e
        else:
            bins[rid].setdefault(k, []).append([b, e])
        prev = (rid, k)
        cnt[rid][1 if flag & 4 else 0] += 1
        span[rid] = [b, e] if span[rid] is None else [span[rid][0], e]
        for w in range(lo, hi + 1):
            lin[rid][w] = min(lin[rid].get(w, b), b)
    out = [b"CSI\1", struct.pack("<iiii", shift, depth, 0, n_ref)]
    for r in range(n_ref):
        if span[r] is None:
            out.append(struct.pack("<i", 0))
            continue
        have = sorted(lin[r])
        out.append(struct.pack("<i", len(bins[r]) + 1))
        for k in sorted(bins[r]):
            l = next(l for l in range(depth + 1) if k >= level_first(depth, l))
            w0 = (k - level_first(depth, l)) << 3 * l
            nxt = have[bisect.bisect_left(have, w0)]                         # (an existing bin always has one)
            out.append(struct.pack("<IQi", k, lin[r][nxt], len(bins[r][k])) + b"".join(struct.pack("<QQ", *c) for c in bins[r][k]))
        out.append(struct.pack("<IQiQQQQ", meta_bin(depth), 0, 2, span[r][0], span[r][1], cnt[r][0], cnt[r][1]))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def parse_csi(raw: bytes):
    """-> (min_shift, depth, [per reference {bin: (loffset, [(beg, end), ...])}], n_no_coor)"""
    assert raw[:4] == b"CSI\1"
    shift, depth, l_aux, n_ref = struct.unpack_from("<iiii", raw, 4)
    assert l_aux == 0
    p = 20
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", raw, p)[0]; p += 4
        bins = {}
        for _b in range(n_bin):
            k, lo, nc = struct.unpack_from("<IQi", raw, p); p += 16
            bins[k] = (lo, [struct.unpack_from("<QQ", raw, p + 16 * c) for c in range(nc)]); p += 16 * nc
        refs.append(bins)
    no_coor = struct.unpack_from("<Q", raw, p)[0]
    assert p + 8 == len(raw)
    return shift, depth, refs, no_coor


def inflate_csi(csi: bytes) -> bytes:
    """the .csi file -> its uncompressed bytes: BGZF members, the last one the end-of-file member"""
    from bwamem_hip.lib import bgzf_eof, inflate_bgzf
    assert csi[-28:] == bgzf_eof() and csi[:4] == b"\x1f\x8b\x08\x04"
    return inflate_bgzf(csi, host=True)


def reg2bins(lo: int, hi: int, depth: int) -> list:
    """every bin that holds a window of lo .. hi or contains one that does"""
    out = []
    for l in range(depth + 1):
        out += range(level_first(depth, l) + (lo >> 3 * l), level_first(depth, l) + (hi >> 3 * l) + 1)
    return out


def query(f: BamFile, raw: bytes, rid: int, beg: int, end: int) -> list:
    """the ordinals of the records of reference rid overlapping [beg, end): the region's bins, the loffset of the deepest existing bin above the region's first window
    as the lower bound, a seek into the members, a filter"""
    shift, depth, refs, _n = parse_csi(raw)
    bins = refs[rid]
    lo, hi = windows(beg, end, f.refs[rid][1], shift)
    lower = 0
    for l in range(depth + 1):
        k = level_first(depth, l) + (lo >> 3 * l)
        if k in bins:
            lower = bins[k][0]
            break
    out = set()
    for k in reg2bins(lo, hi, depth):
        for cb, ce in bins.get(k, (0, ()))[1]:
            if ce <= lower:
                continue
            for i in f.read_chunk(cb, ce):
                r, pos, _bin, _flag, e = fields(f.recs[i])
                if r == rid and pos < end and e > beg:
                    out.add(i)
    return sorted(out)


def brute(f: BamFile, rid: int, beg: int, end: int) -> list:
    return [k for k, r in enumerate(f.recs) if fields(r)[0] == rid and fields(r)[1] < end and fields(r)[4] > beg]


def check_csi(bam: bytes, csi: bytes, contigs, stream: bytes, shift: int = 14, what="", n_regions=50) -> BamFile:
    f = BamFile(bam)
    assert f.refs == [(n, l) for n, l in contigs] and f.stream == py_sort(stream), what
    raw = inflate_csi(csi)
    assert raw == build_csi(f, shift), what
    got_shift, depth, refs, no_coor = parse_csi(raw)
    assert (got_shift, depth) == (shift, depth_of(max([l for _n, l in contigs] or [0]), shift)), what
    assert no_coor == sum(1 for r in f.recs if fields(r)[0] < 0), what
    for bins in refs:
        assert list(bins) == sorted(set(bins) - {meta_bin(depth)}) + ([meta_bin(depth)] if bins else []), what      # ascending, the pseudo-bin last
    with_ref = [i for i, r in enumerate(f.recs) if fields(r)[0] >= 0 and fields(r)[4] > 0]
    if not with_ref or not n_regions:
        return f
    rng = np.random.default_rng(5)
    for i in rng.choice(with_ref, n_regions):                              # every region is centred on a record of the file, so each returns at least one
        rid, pos, _b, _fl, end = fields(f.recs[int(i)])
        w = int(rng.choice([1, 100, 20_000, 300_000]))
        mid = (max(pos, 0) + end) // 2
        beg, fin = max(mid - w, 0), mid + w
        got = query(f, raw, rid, beg, fin)
        assert got == brute(f, rid, beg, fin) and int(i) in got, (what, rid, beg, fin)
    return f


# ---------------------------------------------------------------------------------------------------------------- the cases beyond BAI

def twelve_records() -> tuple:
    """one contig of 2^31 - 1 bases and twelve hand-placed records (in no order): 0, 2^14 - 1, 2^29 - 1, 2^29, 2^30 + 5, 2^31 - 60, a record over 2^29 (a boundary
    at every level but the top: it lands in bin 0), one over W (a boundary of the sixth level down, the deepest, alone: it lands one level up), one running off the
    contig, and the three kinds without a place of their own"""
    recs = [make_record(0, 1 << 30 | 5, 0, b"p30"), make_record(0, 0, 0, b"p0"), make_record(0, (1 << 14) - 1, 16, b"w0_last", ops=((1, 0),), l_seq=1),
            make_record(0, (1 << 29) - 1, 0, b"below29", ops=((1, 0),), l_seq=1), make_record(0, 1 << 29, 0, b"at29"), make_record(0, BIG + 1 - 60, 0, b"near_end"),
            make_record(0, (1 << 29) - 20, 0, b"over29"),                                                       # 50M: 2^29 - 20 .. 2^29 + 30
            make_record(0, W - 3000, 0, b"over_w", ops=((10, 4), (2000, 0), (3000, 3), (1000, 0)), l_seq=3010),  # crosses 2^30 + 2^14: a boundary of the deepest bins only
            make_record(0, BIG - 30, 16, b"off_end"),                                                           # 50M from 2^31 - 31: runs 19 bases off the contig
            make_record(0, 1 << 30, 4 | 1 | 8, b"unmapped_placed", ops=(), l_seq=50),
            make_record(0, -1, 4, b"no_pos", ops=(), l_seq=50),
            make_record(-1, -1, 4, b"no_ref", ops=(), l_seq=50)]
    assert len(recs) == 12
    return [("big", BIG)], b"".join(recs)


def boundary_regions():
    """regions on both sides of every boundary the twelve records sit at"""
    out = []
    for b in (1 << 14, 1 << 29, 1 << 30, W, BIG - 11):
        out += [(b - 1, b), (b, b + 1), (b - 1, b + 1), (b - 40, b - 1), (b + 1, b + 40), (b - 100_000, b + 100_000)]
    return out + [(0, 1), (0, 1 << 14), (0, BIG), (W - 3000, W - 2999), (W - 1001, W + 1), (W + 1000, W + 2000), (W - 900, W + 1900), (BIG - 1, BIG)]


def check_twelve(bam: bytes, csi: bytes, shift: int = 14):
    contigs, stream = twelve_records()
    f = check_csi(bam, csi, contigs, stream, shift, "twelve records", n_regions=20)
    raw = inflate_csi(csi)
    hits = 0
    for beg, end in boundary_regions():
        got = query(f, raw, 0, beg, end)
        assert got == brute(f, 0, beg, end), (beg, end)
        hits += len(got)
    assert hits > 20
    depth = parse_csi(raw)[1]
    assert depth == depth_of(BIG, shift) and (shift != 14 or depth == 6)
    names = {r[36:36 + r[12] - 1]: rec_bin(r, contigs, shift, depth) for r in f.recs if fields(r)[0] == 0}
    if shift == 14:
        # depth 6: level 0 begins at 37449, level 5 (2^29 bases a bin) at 1, level 6 is bin 0
        assert names[b"p0"] == 37449 and names[b"below29"] == 37449 + (1 << 15) - 1 and names[b"at29"] == 37449 + (1 << 15)
        assert names[b"over29"] == 0 and names[b"over_w"] == 4681 + (W >> 17) and names[b"no_pos"] == 37449
        assert names[b"off_end"] == names[b"near_end"] == 37449 + (BIG - 1 >> 14)
        assert names[b"unmapped_placed"] == 37449 + (1 << 16)
    return f


# ---------------------------------------------------------------------------------------------------------------- the tests

@pytest.mark.parametrize("window", [0, 1, 7, 100])
def test_sorted_file_csi_host(window):
    from bwamem_hip.lib import bam_sorted_file
    for what, contigs, stream in corpus():
        bam, csi = bam_sorted_file(HDR, contigs, stream, 1, window, host=True, index_format="csi")
        check_csi(bam, csi, contigs, stream, 14, (what, window))
        assert bam == bam_sorted_file(HDR, contigs, stream, 1, window, host=True)[0], (what, window)      # the record's own bin field stays: the same file under either index


def test_depth_rule():
    from bwamem_hip.lib import bam_sorted_file
    lens = [1, 1 << 14, (1 << 14) + 1, (1 << 17) + 1, (1 << 26) + 1, 1 << 29, (1 << 29) + 1, BIG]
    assert [depth_of(l, 14) for l in lens] == [0, 0, 1, 2, 5, 5, 6, 6]
    for shift in (14, 10, 24):
        for l in lens:
            bam, csi = bam_sorted_file(HDR, [("small", 1), ("c", l)], b"", host=True, index_format="csi", csi_min_shift=shift)
            got_shift, depth, refs, no_coor = parse_csi(inflate_csi(csi))
            assert (got_shift, depth, refs, no_coor) == (shift, depth_of(l, shift), [{}, {}], 0), (shift, l)
            assert depth <= 7 and meta_bin(depth) < 1 << 32
    assert depth_of(BIG, 10) == 7 and depth_of(BIG, 24) == 3 and depth_of(1 << 24, 24) == 0
    for shift in (9, 25, -1, 0):
        with pytest.raises(ValueError):
            bam_sorted_file(HDR, [("c", 1000)], b"", host=True, index_format="csi", csi_min_shift=shift)
    with pytest.raises(ValueError):
        bam_sorted_file(HDR, [("c", 1000)], b"", host=True, csi_min_shift=12)             # a shift without "csi"
    with pytest.raises(ValueError):
        bam_sorted_file(HDR, [("c", 1000)], b"", host=True, index_format="tbi")
    with pytest.raises(ValueError):
        bam_sorted_file(HDR, [("c", 1 << 31)], b"", host=True, index_format="csi")


def test_csi_at_depth_5_holds_what_the_bai_holds():
    from bwamem_hip.lib import bam_sorted_file
    n = 0
    for what, contigs, stream in corpus():
        contigs = [(contigs[0][0], (1 << 29) - 1)] + list(contigs[1:])
        recs = [fields(r) for r in split_records(stream)]
        if not all(rid < 0 or (0 <= pos and end <= contigs[rid][1]) for rid, pos, _b, _f, end in recs):      # records inside their contigs: both indexes bin them alike
            continue
        n += 1
        for window in (0, 7):
            bam, bai = bam_sorted_file(HDR, contigs, stream, 1, window, host=True)
            bam2, csi = bam_sorted_file(HDR, contigs, stream, 1, window, host=True, index_format="csi")
            shift, depth, refs, no_coor = parse_csi(inflate_csi(csi))
            brefs, bno = parse_bai(bai)
            assert (shift, depth, no_coor, bam2) == (14, 5, bno, bam) and meta_bin(depth) == 37450, what
            for bins, (bbins, _ioff) in zip(refs, brefs):
                assert {k: list(v[1]) for k, v in bins.items()} == {k: list(v) for k, v in bbins.items()} and list(bins) == list(bbins), what
    assert n >= 6


def test_beyond_bai():
    from bwamem_hip.lib import bam_sorted_file
    contigs, stream = twelve_records()
    for window in (0, 1, 5):
        bam, csi = bam_sorted_file(HDR, contigs, stream, 1, window, host=True, index_format="csi")
        f = check_twelve(bam, csi)
    assert [fields(r)[1] for r in f.recs][:3] == [-1, 0, (1 << 14) - 1] and fields(f.recs[-1])[0] == -1 and fields(f.recs[-2])[1] == BIG - 30
    for shift in (10, 24):
        bam2, csi = bam_sorted_file(HDR, contigs, stream, 1, 0, host=True, index_format="csi", csi_min_shift=shift)
        assert bam2 == bam_sorted_file(HDR, contigs, stream, 1, 0, host=True, index_format="csi")[0]
        check_twelve(bam2, csi, shift)
    with pytest.raises(ValueError, match="2\\^29"):
        bam_sorted_file(HDR, contigs, stream, 1, 0, host=True, index_format="bai")
    with pytest.raises(ValueError, match="2\\^29"):
        bam_sorted_file(HDR, contigs, stream, 1, 0, host=True)


def dup_pairs(base: int) -> bytes:
    """two duplicate pairs at base + 1000 (the better one last), a pair that shares one end only, and a fragment on a pair's end -- in the writer's order"""
    from test_bam_dup import pair, rec
    rs = pair(b"a", 0, base + 1000, False, 0, base + 1300, True, q=20) + pair(b"b", 0, base + 1000, False, 0, base + 1300, True, q=30) + \
        pair(b"c", 0, base + 1000, False, 0, base + 1400, True) + [rec(b"f", 0, base + 1000, 0)] + pair(b"d", 0, base + 1000, False, 0, base + 1300, True, q=25, ops1=((5, 4), (45, 0)))
    return b"".join(rs)


def test_markdup_limit_and_large_positions():
    from bwamem_hip.lib import bam_sorted_file
    from test_bam_dup import flag_of, name_of
    top = (1 << 30) - (1 << 24)
    bam, csi, counts = bam_sorted_file(HDR, [("wheat_3B", top)], dup_pairs(1 << 29), 1, 0, host=True, markdup=True, index_format="csi")
    f = BamFile(bam)
    with pytest.raises(ValueError, match="wheat_3B"):
        bam_sorted_file(HDR, [("ok", 1000), ("wheat_3B", top + 1)], dup_pairs(0), 1, 0, host=True, markdup=True, index_format="csi")
    bam_sorted_file(HDR, [("ok", 1000), ("wheat_3B", top + 1)], b"", 1, 0, host=True, index_format="csi")          # refused for marking only
    small, _bai, counts_small = bam_sorted_file(HDR, [("short", 1 << 20)], dup_pairs(0), 1, 0, host=True, markdup=True)
    g = BamFile(small)
    flags = [(name_of(r), flag_of(r)) for r in f.recs]
    assert flags == [(name_of(r), flag_of(r)) for r in g.recs] and counts == counts_small
    assert [fields(r)[1] - (1 << 29) for r in f.recs] == [fields(r)[1] for r in g.recs]
    dup = {n for n, fl in flags if fl & 0x400}
    assert dup == {b"a", b"f"} and counts["duplicate_pairs"] == 1 and counts["duplicate_fragments"] == 1      # d's unclipped end is 5 to the left: not a duplicate
    raw = inflate_csi(csi)
    assert raw == build_csi(f, 14) and query(f, raw, 0, (1 << 29) + 1000, (1 << 29) + 1001) == brute(f, 0, (1 << 29) + 1000, (1 << 29) + 1001)


def test_python_keywords_refuse_bad_values(tmp_path):
    from bwamem_hip.aligner import Aligner
    al = Aligner.__new__(Aligner)                                         # the keyword checks come before anything touches an index or a device
    al.profile = False
    al.rg_line = ""
    grp = [("@RG\\tID:a", "r.fa")]
    for call in (lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", index_format="csi"),                                     # "csi" needs sort=True
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", index_format="csi", index=str(tmp_path / "x.csi")),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), index_format="csi"),
                 lambda: al.align_groups(grp, out=io.BytesIO(), fmt="bam", index_format="csi"),
                 lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", sort=True, csi_min_shift=12),                             # a shift needs "csi"
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, index_format="bai", csi_min_shift=15),
                 lambda: al.align_groups(grp, out=io.BytesIO(), fmt="bam", sort=True, csi_min_shift=10),
                 lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", sort=True, index_format="csi", csi_min_shift=9),          # 10 .. 24
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, index_format="csi", csi_min_shift=25),
                 lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", sort=True, index_format="tbi"),
                 lambda: al.align_file("r.fa", io.BytesIO(), sort=True, index_format="csi")):                                    # sort needs fmt="bam"
        with pytest.raises(ValueError):
            call()
    assert not os.path.exists(tmp_path / "x.csi") and getattr(al, "_native", None) is None
    assert getattr(al, "_index_format", ("bai", 14)) == ("bai", 14)


def test_mem_command_refuses_a_shift_without_csi(capsys):
    from bwamem_hip import mem
    assert mem.main(["--sort", "--csi-min-shift", "12", "idx", "r.fa"]) == 2 and "--csi" in capsys.readouterr().err
    assert mem.main(["--csi", "--csi-min-shift", "9", "idx", "r.fa"]) == 2 and "10 .. 24" in capsys.readouterr().err
    assert "--csi" in mem.__doc__ and "--csi-min-shift" in mem.__doc__


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_csi_core_host")
    src = [os.path.join(HERE, "bam_csi_core_host.cpp"), os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(tmp_path, contigs, shift: int, stream: bytes) -> bytes:
    fi, fo = str(tmp_path / "csi_case.bin"), str(tmp_path / "csi_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(contigs)) + b"".join(struct.pack("<i", l) for _n, l in contigs) + struct.pack("<iQ", shift, len(stream)) + stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        return f.read()


def test_core_under_sanitizers(tmp_path):
    cases = [(w, c, s, 14) for w, c, s in corpus()] + [("twelve", *twelve_records(), sh) for sh in (14, 10, 24)]
    what, contigs, stream = [c for c in corpus() if c[0] == "mixed"][0]
    cases += [(what, contigs, stream, 10), (what, contigs, stream, 24)]
    for what, contigs, stream, shift in cases:
        res = run_core(tmp_path, contigs, shift, stream)
        recs = split_records(py_sort(stream))
        depth = depth_of(max(l for _n, l in contigs), shift)
        assert struct.unpack_from("<IiI", res, 0) == (len(recs), depth, meta_bin(depth)), (what, shift)
        assert list(struct.unpack_from("<%dI" % (depth + 1), res, 12)) == [level_first(depth, l) for l in range(depth + 1)], (what, shift)
        p, prev = 12 + 4 * (depth + 1), None
        for rec in recs:
            lo, hi, k, head = struct.unpack_from("<IIII", res, p); p += 16
            rid, pos, _bin, _fl, end = fields(rec)
            if rid >= 0:
                assert (lo, hi) == windows(pos, end, contigs[rid][1], shift) and k == bin_of(lo, hi, depth), (what, shift, rid, pos)
                assert hi < (((contigs[rid][1] - 1) >> shift) + 1 if contigs[rid][1] > 0 else 1)
            cur = (rid, k) if rid >= 0 else (-1, None)
            assert head == (prev is None or (prev[0] >= 0 if rid < 0 else prev != cur)), (what, shift)
            prev = cur
        assert p == len(res), (what, shift)
    assert struct.unpack_from("<I", run_core(tmp_path, corpus()[0][1], 14, corpus()[0][2][:-1]), 0)[0] == 0xFFFFFFFF
