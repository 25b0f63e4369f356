"""Coordinate-sorted BAM and its BAI index, host forms: csrc/bam_sort_core.h as plain C++ under AddressSanitizer and UBSan (tests/bam_sort_core_host.cpp) and the
library's host entry points, against checkers written here from the SAM specification (sections 4.2, 5.2) and independent of the C sources: a sorter (`sorted` on
(key, ordinal)), a BAI builder that reads the finished file, a BAI / BGZF reader that answers region queries.  The same corpora run on the device in
test_bam_sort_gpu.py."""
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_bam_core import PIECE, encode_text, golden_sam_texts, split_members

HERE = os.path.dirname(os.path.abspath(__file__))
CONTIGS = [("chr1", 400_000_000), ("chr2", 40_000), ("chr1_alt", 150), ("empty", 50_000), ("HLA-A*01:01", 70)]
META_BIN = 37450


# ---------------------------------------------------------------------------------------------------------------- records and their order

def split_records(stream: bytes) -> list:
    out, p = [], 0
    while p < len(stream):
        n = struct.unpack_from("<I", stream, p)[0] + 4
        assert p + n <= len(stream)
        out.append(stream[p:p + n]); p += n
    return out


def fields(rec: bytes):
    """(refID, pos, bin, flag, end): end = pos + the CIGAR's reference length, pos + 1 when that is 0 or the read is unmapped"""
    rid, pos, l_name, _mq, bin_, n_ops, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    ops = struct.unpack_from("<%dI" % n_ops, rec, 36 + l_name)
    rl = sum(v >> 4 for v in ops if v & 15 in (0, 2, 3, 7, 8))
    return rid, pos, bin_, flag, pos + 1 if (flag & 4) or rl == 0 else pos + rl


def key(rec: bytes) -> int:
    rid, pos, _b, flag, _e = fields(rec)
    return (rid & 0xFFFFFFFF) << 32 | ((pos + 1) & 0xFFFFFFFF) << 1 | (flag >> 4 & 1)


def py_sort(stream: bytes) -> bytes:
    recs = split_records(stream)
    return b"".join(recs[i] for i in sorted(range(len(recs)), key=lambda i: (key(recs[i]), i)))


def make_record(rid, pos, flag=0, name=b"r", ops=((50, 0),), l_seq=50, bin_=None, tag=b"") -> bytes:
    """a record built field by field (pos 0-based)"""
    from test_bam_core import reg2bin
    rl = sum(n for n, o in ops if o in (0, 2, 3, 7, 8))
    if bin_ is None:
        bin_ = 4680 if pos < 0 else reg2bin(pos, pos + 1 if (flag & 4) or rl == 0 else pos + rl)
    body = struct.pack("<iiBBHHHIiii", rid, pos, len(name) + 1, 30, bin_, len(ops), flag, l_seq, -1, -1, 0) + name + b"\0"
    body += b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + b"\x12" * ((l_seq + 1) // 2) + b"\x1e" * l_seq + tag
    return struct.pack("<I", len(body)) + body


def golden_streams():
    """(name, contigs, record stream) of the SAM texts under tests/golden: single-end, paired and the multi-contig ALT sets"""
    out = []
    for what, full, body in golden_sam_texts():
        contigs = [(l.split(b"\t")[1][3:].decode(), int(l.split(b"\t")[2][3:])) for l in full.split(b"\n") if l.startswith(b"@SQ")]
        if not contigs:
            contigs = sorted({(l.split(b"\t")[k].decode(), (1 << 29) - 1) for l in body.split(b"\n") if l for k in (2, 6) if l.split(b"\t")[k] not in (b"*", b"=")})
        recs, st = encode_text(body, contigs)
        assert not st.any(), what
        out.append((what, contigs, recs))
    assert len(out) >= 3 and any(len(c) > 1 for _w, c, _r in out)
    return out


def synthetic_streams():
    rng = np.random.default_rng(11)
    same = b"".join(make_record(1, 700, 0, b"s%03d" % i) for i in range(300))                                             # all keys equal: only stability orders them
    norefs = b"".join(make_record(-1, -1, 4, b"u%03d" % i, ops=(), l_seq=int(rng.integers(1, 90))) for i in range(200))
    mates = b"".join(make_record(1, int(p), f, b"m%03d" % i, ops=((50, 0),) if not f & 4 else ()) for i, (p, f) in
                     enumerate((int(rng.integers(0, 39_000)), int(rng.choice([0, 16, 4, 20]))) for _ in range(400)))      # unmapped reads placed at a mate's position
    strands = make_record(0, 999, 16, b"rev") + make_record(0, 999, 0, b"fwd") + make_record(0, 998, 16, b"before") + make_record(0, 999, 16, b"rev2")
    mixed = []
    for i in range(1500):
        rid = int(rng.choice([-1, 0, 1, 2, 4]))
        ln = [400_000_000, 40_000, 150, 0, 70][rid] if rid >= 0 else 0
        span = int(rng.choice([1, 30, 50, 20_000, 70_000])) if rid == 0 else 20
        pos = int(rng.integers(0, max(ln - span, 1))) if rid >= 0 else -1
        if rid == 0 and i % 3:
            pos = int(rng.integers(0, 200_000))                                                                        # dense: windows shared by many records
        fl = int(rng.choice([0, 16, 4])) if rid >= 0 else 4
        mixed.append(make_record(rid, pos, fl, b"x%04d" % i, ops=((10, 4), (span, 0), (3, 1)) if rid >= 0 else (), l_seq=int(rng.integers(1, 150))))
    boundary = b"".join(make_record(1, 10 * i, 0, b"r%03d" % i) for i in range(600))                                     # 120 bytes each: record 544 begins member 2
    assert len(make_record(1, 0, 0, b"r000")) == 120 and PIECE % 120 == 0
    # 500 records of 120 bytes, then one of 75 000: it begins in the first member, fills the second and ends in the third
    big = b"".join(make_record(0, i, 0, b"b%03d" % i) for i in range(500)) + make_record(0, 1003, 0, b"huge", ops=((50_000, 0),), l_seq=50_000) + \
        b"".join(make_record(0, 2000 + i, 16, b"c%d" % i) for i in range(5))
    assert max(len(r) for r in split_records(big)) >= 70_000
    return [("equal keys", CONTIGS, same), ("no references", CONTIGS, norefs), ("placed mates", CONTIGS, mates), ("two strands", CONTIGS, strands),
            ("mixed", CONTIGS, b"".join(mixed)), ("empty", CONTIGS, b""), ("one record", CONTIGS, make_record(2, 5, 0, b"only")),
            ("record on a member boundary", CONTIGS, boundary), ("a record over three members", CONTIGS, big)]


_CORPUS = []


def corpus():
    if not _CORPUS:
        _CORPUS.extend(golden_streams() + synthetic_streams())
    return _CORPUS


# ---------------------------------------------------------------------------------------------------------------- the file: BGZF, header, BAI

class BamFile:
    """a BAM file read member by member with zlib: the header, the records with their virtual offsets"""

    def __init__(self, blob: bytes):
        from bwamem_hip.lib import bgzf_eof
        ms = split_members(blob)
        assert ms[-1] == bgzf_eof()
        self.coff, self.ustart, self.text = [], [], []
        c = u = 0
        for m in ms:
            t = zlib.decompress(m, 31)
            assert m is ms[-1] or len(t) > 0
            self.coff.append(c); self.ustart.append(u); self.text.append(t)
            c += len(m); u += len(t)
        self.data = b"".join(self.text)
        d = self.data
        assert d[:4] == b"BAM\1"
        l_text = struct.unpack_from("<I", d, 4)[0]
        self.header_text = d[8:8 + l_text]
        p = 8 + l_text
        n_ref = struct.unpack_from("<I", d, p)[0]; p += 4
        self.refs = []
        for _ in range(n_ref):
            l = struct.unpack_from("<I", d, p)[0]
            self.refs.append((d[p + 4:p + 4 + l - 1].decode(), struct.unpack_from("<I", d, p + 4 + l)[0])); p += 8 + l
        self.first = p
        self.stream = d[p:]
        self.recs, self.upos = [], []
        for r in split_records(self.stream):
            self.recs.append(r); self.upos.append(p); p += len(r)
        self.upos.append(p)
        assert self.first in self.ustart, "the records begin a member of their own"

    def voff(self, u: int) -> int:
        """the virtual offset of uncompressed byte u: the member that holds it; behind the last record, byte 0 of the member that follows"""
        for i in range(len(self.coff) - 1, -1, -1):
            if self.ustart[i] <= u and (u < self.ustart[i] + len(self.text[i]) or i == len(self.coff) - 1):
                return self.coff[i] << 16 | (u - self.ustart[i])
        raise AssertionError(u)

    def seek(self, v: int) -> int:
        """virtual offset -> uncompressed position; the file offset must begin a member"""
        i = self.coff.index(v >> 16)
        assert (v & 0xFFFF) < max(len(self.text[i]), 1)
        return self.ustart[i] + (v & 0xFFFF)

    def read_chunk(self, beg: int, end: int) -> list:
        """the ordinals of the records from virtual offset beg up to end"""
        a, b = self.seek(beg), self.seek(end)
        i = self.upos.index(a)
        out = []
        while self.upos[i] < b:
            out.append(i); i += 1
        assert self.upos[i] == b
        return out


def n_windows(length: int) -> int:
    return ((length - 1) >> 14) + 1 if length > 0 else 1


def build_bai(f: BamFile) -> bytes:
    """the index of section 5.2 from the finished file, by the rules of the issue: chunks are maximal runs of records of one (refID, bin); the pseudo-bin 37450 last;
    the linear index up to the highest window, holes filled from the left; windows clamped to the contig's last (a record that runs off its contig indexes there)"""
    n_ref = len(f.refs)
    bins = [dict() for _ in range(n_ref)]; lin = [dict() for _ in range(n_ref)]; cnt = [[0, 0] for _ in range(n_ref)]; span = [None] * n_ref
    no_coor, prev = 0, None
    for i, rec in enumerate(f.recs):
        rid, pos, bin_, flag, end = fields(rec)
        b, e = f.voff(f.upos[i]), f.voff(f.upos[i + 1])
        if rid < 0:
            no_coor += 1; prev = None
            continue
        if prev == (rid, bin_):
            bins[rid][bin_][-1][1] = e
        else:
            bins[rid].setdefault(bin_, []).append([b, e])
        prev = (rid, bin_)
        cnt[rid][1 if flag & 4 else 0] += 1
        span[rid] = [b, e] if span[rid] is None else [span[rid][0], e]
        nw = n_windows(f.refs[rid][1])
        p0 = max(pos, 0); e0 = max(end, p0 + 1)
        hi = min((e0 - 1) >> 14, nw - 1); lo = min(p0 >> 14, hi)
        for w in range(lo, hi + 1):
            lin[rid][w] = min(lin[rid].get(w, b), b)
    out = [b"BAI\1", struct.pack("<I", n_ref)]
    for r in range(n_ref):
        if span[r] is None:
            out.append(struct.pack("<II", 0, 0))
            continue
        out.append(struct.pack("<I", len(bins[r]) + 1))
        for b in sorted(bins[r]):
            out.append(struct.pack("<II", b, len(bins[r][b])) + b"".join(struct.pack("<QQ", *c) for c in bins[r][b]))
        out.append(struct.pack("<IIQQQQ", META_BIN, 2, span[r][0], span[r][1], cnt[r][0], cnt[r][1]))
        n_intv = max(lin[r]) + 1
        out.append(struct.pack("<I", n_intv))
        last = 0
        for w in range(n_intv):
            last = lin[r].get(w, last)
            out.append(struct.pack("<Q", last))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def parse_bai(bai: bytes):
    assert bai[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<I", bai, 4)[0]; p = 8
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<I", bai, p)[0]; p += 4
        bins = {}
        for _b in range(n_bin):
            b, nc = struct.unpack_from("<II", bai, p); p += 8
            bins[b] = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(nc)]; p += 16 * nc
        n_intv = struct.unpack_from("<I", bai, p)[0]; p += 4
        refs.append((bins, struct.unpack_from("<%dQ" % n_intv, bai, p))); p += 8 * n_intv
    no_coor = struct.unpack_from("<Q", bai, p)[0]
    assert p + 8 == len(bai)
    return refs, no_coor


def reg2bins(beg: int, end: int) -> list:
    end -= 1
    out = [0]
    for sh, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(base + (beg >> sh), base + (end >> sh) + 1)
    return out


def query(f: BamFile, bai: bytes, rid: int, beg: int, end: int) -> list:
    """the ordinals of the records of reference rid overlapping [beg, end): the region's bins, the linear index's lower bound, a seek into the members, a filter"""
    bins, ioff = parse_bai(bai)[0][rid]
    lower = ioff[min(beg >> 14, len(ioff) - 1)] if len(ioff) else 0
    out = set()
    for b in reg2bins(beg, end):
        for cb, ce in bins.get(b, ()):
            if ce <= lower:
                continue
            for i in f.read_chunk(cb, ce):
                r, pos, _bin, _flag, e = fields(f.recs[i])
                if r == rid and pos < end and e > beg:
                    out.add(i)
    return sorted(out)


def check_file(bam: bytes, bai: bytes, header_text: str, contigs, stream: bytes, what="", n_regions=50):
    f = BamFile(bam)
    assert f.header_text == header_text.encode() and f.refs == [(n, l) for n, l in contigs], what
    assert f.stream == py_sort(stream), what
    assert bai == build_bai(f), what
    refs, no_coor = parse_bai(bai)
    assert no_coor == sum(1 for r in f.recs if fields(r)[0] < 0)
    for bins, _io in refs:
        assert list(bins) == sorted(set(bins) - {META_BIN}) + ([META_BIN] if bins else []), what          # ascending, the pseudo-bin last
    with_ref = [i for i, r in enumerate(f.recs) if fields(r)[0] >= 0]
    if not with_ref:
        return f
    rng = np.random.default_rng(5)
    for i in rng.choice(with_ref, n_regions):                              # every region is centred on a record of the file, so each returns at least one
        rid, pos, _b, _fl, end = fields(f.recs[int(i)])
        w = int(rng.choice([1, 100, 20_000, 300_000]))
        beg, fin = max((pos + end) // 2 - w, 0), (pos + end) // 2 + w
        brute = [k for k, r in enumerate(f.recs) if fields(r)[0] == rid and fields(r)[1] < fin and fields(r)[4] > beg]
        got = query(f, bai, rid, beg, fin)
        assert got == brute and len(got) >= 1 and int(i) in got, (what, rid, beg, fin)
    return f


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_sort_core_host")
    src = [os.path.join(HERE, "bam_sort_core_host.cpp"), os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(tmp_path, contigs, stream: bytes):
    fi, fo = str(tmp_path / "sort_case.bin"), str(tmp_path / "sort_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(contigs)) + b"".join(struct.pack("<i", l) for _n, l in contigs) + struct.pack("<Q", len(stream)) + stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        return f.read()


def test_core_under_sanitizers(tmp_path):
    for what, contigs, stream in corpus():
        res = run_core(tmp_path, contigs, stream)
        want = py_sort(stream)
        recs = split_records(want)
        assert struct.unpack_from("<I", res, 0)[0] == len(recs), what
        assert res[4:4 + len(want)] == want, what
        p, u, prev = 4 + len(want), 0, None
        n_members = (len(want) + PIECE - 1) // PIECE

        def voff(u):
            return (1000 + 100 * n_members) << 16 if u >= len(want) else (1000 + 100 * (u // PIECE)) << 16 | u % PIECE
        for rec in recs:
            k, end, lo, hi, head, v = struct.unpack_from("<QqIIIQ", res, p); p += 36
            rid, pos, bin_, _fl, e = fields(rec)
            assert (k, end, v) == (key(rec), e, voff(u)), what
            if rid >= 0:
                nw = n_windows(contigs[rid][1]); h = min((max(e, max(pos, 0) + 1) - 1) >> 14, nw - 1)
                assert (lo, hi) == (min(max(pos, 0) >> 14, h), h), what
            assert head == (prev is None or (prev[0] >= 0 if rid < 0 else prev != (rid, bin_))), what
            prev = (rid, bin_); u += len(rec)
        assert struct.unpack_from("<Q", res, p)[0] == voff(u) and p + 8 == len(res), what
    cut = corpus()[0][2][:-1]
    assert struct.unpack_from("<I", run_core(tmp_path, corpus()[0][1], cut), 0)[0] == 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------- the host entry points

def test_sort_host():
    from bwamem_hip.lib import bam_sort
    for what, _contigs, stream in corpus():
        got = bam_sort(stream, host=True)
        assert got == py_sort(stream), what
        assert bam_sort(got, host=True) == got, what
    same = dict((w, s) for w, _c, s in corpus())["equal keys"]
    assert bam_sort(same, host=True) == same                               # stability: nothing but the order they came in
    for cut in (same[:-1], same[:len(same) - 120 + 20], same + b"\x10\0\0\0"):
        with pytest.raises(ValueError):
            bam_sort(cut, host=True)


@pytest.mark.parametrize("window", [0, 1, 7, 100])
def test_sorted_file_host(window):
    from bwamem_hip.lib import bam_sorted_file
    hdr = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:1\n"
    for what, contigs, stream in corpus():
        for level in ((0, 1) if window == 7 else (1,)):
            bam, bai = bam_sorted_file(hdr, contigs, stream, level, window, host=True)
            f = check_file(bam, bai, hdr, contigs, stream, (what, window, level))
        if what == "record on a member boundary" and window == 0:
            assert f.voff(f.upos[544]) & 0xFFFF == 0 and f.voff(f.upos[544]) >> 16 == f.coff[f.ustart.index(f.upos[544])]
        if what == "a record over three members" and window == 0:
            i = [len(r) for r in f.recs].index(max(len(r) for r in f.recs))
            assert (f.voff(f.upos[i + 1]) >> 16) > (f.voff(f.upos[i]) >> 16) and f.coff.index(f.voff(f.upos[i + 1]) >> 16) - f.coff.index(f.voff(f.upos[i]) >> 16) == 2


def test_region_on_a_contig_without_reads():
    from bwamem_hip.lib import bam_sorted_file
    what, contigs, stream = [c for c in corpus() if c[0] == "mixed"][0]
    bam, bai = bam_sorted_file("@CO\tx\n", contigs, stream, 1, 100, host=True)
    f = BamFile(bam)
    refs, _n = parse_bai(bai)
    assert refs[3] == ({}, ()) and query(f, bai, 3, 100, 20_000) == []
    assert struct.pack("<QQ", *refs[1][0][META_BIN][1]) == struct.pack("<QQ", sum(1 for r in f.recs if fields(r)[0] == 1 and not fields(r)[3] & 4),
                                                                        sum(1 for r in f.recs if fields(r)[0] == 1 and fields(r)[3] & 4))


def test_contig_beyond_bai_is_refused():
    from bwamem_hip.lib import bam_sorted_file
    with pytest.raises(ValueError, match="2\\^29"):
        bam_sorted_file("", [("big", 1 << 29)], b"", host=True)
    with pytest.raises(ValueError):
        bam_sorted_file("", [("a", 100)], make_record(1, 5), host=True)    # a reference the table does not have


def test_python_keywords_refuse_bad_values(tmp_path):
    from bwamem_hip.aligner import Aligner
    al = Aligner.__new__(Aligner)                                         # the keyword checks come before anything touches an index or a device
    al.profile = False
    for call in (lambda: al.align_file("r.fa", io.BytesIO(), sort=True),                                # sort needs fmt="bam"
                 lambda: al.align_file("r.fa", io.BytesIO(), fmt="sam", sort=True),
                 lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", index=str(tmp_path / "x.bai")),  # index needs sort
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", index=io.BytesIO()),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), sort=True),
                 lambda: al.align_batch(["r"], ["ACGT"], sort=True),
                 lambda: al.align_batch(["r"], ["ACGT"], fmt="bam", sort=True)):
        with pytest.raises(ValueError):
            call()
    assert not os.path.exists(tmp_path / "x.bai")


def test_a_refused_sort_leaves_the_aligner_as_it_was(monkeypatch):
    from bwamem_hip.aligner import Aligner
    al = Aligner.__new__(Aligner)
    al.profile = True                                                     # a profile run writes batch after batch: sort=True is refused ...
    with pytest.raises(NotImplementedError):
        al.align_file("r.fa", io.BytesIO(), fmt="bam", sort=True)
    assert getattr(al, "_out_fmt", ("sam", 1)) == ("sam", 1)              # ... and the next SAM or BAM call of the same object is not a sorted one
    al.profile = False
    monkeypatch.setenv("BMH_ALIGNER_NATIVE", "0")
    with pytest.raises(NotImplementedError):
        al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, index=io.BytesIO())
    assert getattr(al, "_out_fmt", ("sam", 1)) == ("sam", 1)
