"""BAM as read input, the host form (csrc/bam_in_core.h, csrc/reads_io.cpp: bmh_bam_host_run) through read_reads_files(host=True) and bam_to_reads(host=True).

The BAM bytes are written here with struct (bam_record, bam_file); nothing the library produces defines its own expectation: the expected reads are the lists
the records were made from, or what the FASTQ loader (pinned to the reference elsewhere) gave for the FASTQ the records were made from.  A FASTQ comment is
free text and a BAM comment is made of tags, so a read's FASTQ comment c travels as the tag CO:Z:c and is expected back as "CO:Z:" + c.
CASES (well-formed) and REFUSALS are shared with test_bam_input_gpu.py, where the kernels must equal this form at every window size.
The per-record core also runs as a stand-alone program under AddressSanitizer and UBSan (tests/bam_in_core_host.cpp)."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from bwamem_hip.aligner import ReadSet, bam_to_reads, read_reads_files
from bwamem_hip.lib import reads_last_bam_counts
from test_reads_input import FIX, bgzf, same_read_sets

HERE = os.path.dirname(os.path.abspath(__file__))
NT16 = b"=ACMGRSVTWYHKDBN"
COMP = bytes.maketrans(b"=ACMGRSVTWYHKDBN", b"=TGKCYSBAWRDMHVN")        # samtools' table: = N S W stay, A<->T C<->G M<->K R<->Y V<->B H<->D
FASTQ = ["four.fq", "crlf.fq", "ml.fq", "r1.fq", "r2.fq"]


# ---------------------------------------------------------------------------------------------------------------- a BAM encoder (SAM spec 4.2)

def tag(name: bytes, ty: bytes, value) -> bytes:
    fmt = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I", b"f": "<f"}
    if ty == b"A":
        return name + b"A" + value
    if ty in (b"Z", b"H"):
        return name + ty + value + b"\0"
    if ty == b"B":
        sub, vals = value
        return name + b"B" + sub + struct.pack("<I", len(vals)) + b"".join(struct.pack(fmt[sub], v) for v in vals)
    return name + ty + struct.pack(fmt[ty], value)


def bam_record(name: bytes, seq: bytes, qual=None, flag: int = 4, tags: bytes = b"", cigar=(), block_size=None, l_read_name=None, nul: bytes = b"\0") -> bytes:
    """seq: letters of NT16; qual: Phred + 33 bytes of its length, or None (0xff); the keyword arguments behind `cigar` damage the record"""
    nib = [NT16.index(c) for c in seq] + [0]
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))
    q = b"\xff" * len(seq) if qual is None else bytes(c - 33 for c in qual)
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(name) + len(nul) if l_read_name is None else l_read_name, 0, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += name + nul + b"".join(struct.pack("<I", c) for c in cigar) + packed + q + tags
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def bam_header(text: bytes = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrUn_random\tLN:77\n", refs=((b"chr1", 1000), (b"chrUn_random", 77))) -> bytes:
    return b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs)) + b"".join(struct.pack("<I", len(n) + 1) + n + b"\0" + struct.pack("<I", l) for n, l in refs)


def bam_file(records: bytes, block: int = 777, eof: bool = True) -> bytes:
    z = bgzf(bam_header() + records, block)
    return z if eof else z[:-28]


def revcomp(seq: bytes) -> bytes:
    return seq.translate(COMP)[::-1]


def stored(name, seq, qual, flag=4, tags=b"", rev=False):
    """the record of a read given in sequencing orientation; rev: stored reverse-complemented under flag 0x10"""
    if rev:
        return bam_record(name, revcomp(seq), None if qual is None else qual[::-1], flag | 0x10, tags)
    return bam_record(name, seq, qual, flag, tags)


# ---------------------------------------------------------------------------------------------------------------- expectations

def _codes(ascii_):
    table = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        table[c] = i
    return table[np.asarray(ascii_, np.uint8)]


def expect(names, seqs, quals, comments) -> ReadSet:
    rs = ReadSet.from_lists([n.decode("latin-1") for n in names], [np.frombuffer(s, np.uint8) for s in seqs], quals=quals, comments=None)
    ce = [c + b"\0" for c in comments]
    rs.comments = (np.frombuffer(b"".join(ce), np.uint8), np.concatenate([[0], np.cumsum([len(e) for e in ce])[:-1]]).astype(np.uint64))
    rs.codes = _codes(rs.ascii)
    return rs


def reads_of(rs: ReadSet):
    """(name, seq, qual, comment) of every read"""
    out, cb, co = [], rs.comments[0].tobytes(), rs.comments[1]
    nb = rs.name_blob.tobytes()
    for i in range(len(rs)):
        o, l = int(rs.offs[i]), int(rs.lens[i])
        n0 = int(rs.name_off[i])
        c0 = int(co[i])
        out.append((nb[n0:nb.index(b"\0", n0)], rs.ascii[o:o + l].tobytes(), None if rs.qual is None else rs.qual[o:o + l].tobytes(), cb[c0:cb.index(b"\0", c0)]))
    return out


def co_tag(c: bytes) -> bytes:
    return tag(b"CO", b"Z", c) if c else b""


def with_tag_comments(rs: ReadSet) -> ReadSet:
    """the same reads with every non-empty comment c as CO:Z:c"""
    rd = reads_of(rs)
    e = expect([r[0] for r in rd], [r[1] for r in rd], None if rs.qual is None else [r[2] for r in rd], [b"CO:Z:" + r[3] if r[3] else b"" for r in rd])
    same_read_sets(ReadSet(e.ascii, e.offs, e.lens, e.name_blob, e.name_off, codes=e.codes, qual=e.qual), ReadSet(rs.ascii, rs.offs, rs.lens, rs.name_blob, rs.name_off, codes=rs.codes, qual=rs.qual), "expect()")
    return e


ALL16 = NT16 * 62 + NT16[:8]                             # 1000 bases, every letter


def _tag_case():
    every = tag(b"a1", b"A", b"q") + tag(b"c1", b"c", -128) + tag(b"C1", b"C", 255) + tag(b"s1", b"s", -32768) + tag(b"S1", b"S", 65535) + \
        tag(b"i1", b"i", -2147483648) + tag(b"I1", b"I", 4294967295) + tag(b"f1", b"f", 1.5) + tag(b"z1", b"Z", b"some text, with blanks") + tag(b"h1", b"H", b"1AE301") + \
        tag(b"b1", b"B", (b"c", [1, -2, 3])) + tag(b"b2", b"B", (b"S", [])) + tag(b"b3", b"B", (b"f", [0.5, 2.0])) + tag(b"z2", b"Z", b"") + tag(b"i2", b"C", 0)
    every_text = b"a1:A:q\tc1:i:-128\tC1:i:255\ts1:i:-32768\tS1:i:65535\ti1:i:-2147483648\tI1:i:4294967295\tz1:Z:some text, with blanks\th1:H:1AE301\tz2:Z:\ti2:i:0"
    listed = b"".join(tag(n, b"Z", b"x") for n in (b"NM", b"MD", b"AS", b"XS", b"SA", b"XA", b"pa", b"RG", b"MC", b"MQ"))
    recs = [(b"every", b"ACGTN", b"IIIII", every, every_text), (b"none", b"ACG", b"III", b"", b""), (b"listed", b"AC", b"II", listed + tag(b"BC", b"Z", b"ACGT") + tag(b"NM", b"C", 3), b"BC:Z:ACGT"),
            (b"onlyf", b"A", b"I", tag(b"f2", b"f", 0.25), b""), (b"rev", b"ACGTT", b"ABCDE", tag(b"RX", b"Z", b"AAC-GGT") + tag(b"QX", b"Z", b"II II"), b"RX:Z:AAC-GGT\tQX:Z:II II")]
    data = b"".join(stored(n, s, q, tags=t, rev=(n == b"rev")) for n, s, q, t, _ in recs)
    return data, expect([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], [r[4] for r in recs]), dict(records_skipped=0, tags_left_out=5)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name -> (records, expected ReadSet (comments=True), expected bam counts or None)"""
    out = {}
    for name in FASTQ:
        orig = read_reads_files(os.path.join(FIX, name), comments=True, host=True)
        rd, e = reads_of(orig), with_tag_comments(orig)
        assert all(set(r[1]) <= set(NT16) for r in rd), name                     # (a BAM holds these sixteen letters; the fixtures use no other)
        out[name] = (b"".join(stored(n, s, q, tags=co_tag(c)) for n, s, q, c in rd), e, None)
        out[name + " 0x10"] = (b"".join(stored(n, s, q, tags=co_tag(c), rev=bool(i & 1)) for i, (n, s, q, c) in enumerate(rd)), e, None)
    two = read_reads_files(os.path.join(FIX, "r1.fq"), os.path.join(FIX, "r2.fq"), comments=True, host=True)
    rd, recs = reads_of(two), []
    for i in range(0, len(rd), 2):
        a = stored(*rd[i][:3], flag=0x4D, tags=co_tag(rd[i][3]), rev=bool(i & 2))
        b = stored(*rd[i + 1][:3], flag=0x8D, tags=co_tag(rd[i + 1][3]), rev=bool(i & 4))
        recs += [a, b] if (i // 2) % 3 != 1 else [b, a]                          # both orders within a pair
    out["pairs"] = (b"".join(recs), with_tag_comments(two), dict(records_skipped=0, tags_left_out=0))
    # the padding nibble, an odd length mirrored
    short = [(b"s%d%s" % (l, b"r" if rev else b"f"), ALL16[3:3 + l], bytes(range(40, 40 + l)), rev) for l in (1, 2, 3, 4, 5) for rev in (False, True)]
    out["lengths 1-5"] = (b"".join(stored(n, s, q, rev=r) for n, s, q, r in short), expect([x[0] for x in short], [x[1] for x in short], [x[2] for x in short], [b""] * len(short)), None)
    q1000 = bytes(33 + (i * 7) % 94 for i in range(1000))
    long_ = [(b"long%d" % k, ALL16[k:] + ALL16[:k], q1000[k:] + q1000[:k], bool(k & 1)) for k in range(6)]
    out["1000 bases, 16 letters"] = (b"".join(stored(n, s, q, rev=r) for n, s, q, r in long_), expect([x[0] for x in long_], [x[1] for x in long_], [x[2] for x in long_], [b""] * len(long_)), None)
    # secondary and supplementary records between and inside pairs: skipped (also without bases, as aligners write secondary lines) and counted
    sk = [bam_record(b"p0", b"ACGT", b"IIII", 0x900 | 0x41), bam_record(b"other", b"", None, 0x100)]
    pr = [(b"p%d" % (i // 2), ALL16[i:i + 7], bytes([50 + i]) * 7) for i in range(4)]
    recs = [sk[0]]
    for i in (0, 2):
        recs += [stored(*pr[i], flag=0x41), sk[1], bam_record(pr[i][0], b"AC", None, 0x800 | 0x81), stored(*pr[i + 1], flag=0x81, rev=True), sk[0]]
    out["skipped"] = (b"".join(recs), expect([x[0] for x in pr], [x[1] for x in pr], [x[2] for x in pr], [b""] * 4), dict(records_skipped=7, tags_left_out=0))
    single_sk = [stored(b"a", b"ACG", b"III"), bam_record(b"a", b"ACGTA", b"IIIII", 0x800), stored(b"b", b"TTGA", b"ABCD", flag=0x10 | 0), bam_record(b"b", b"", None, 0x100)]
    out["skipped, single-end"] = (b"".join(single_sk), expect([b"a", b"b"], [b"ACG", b"TCAA"], [b"III", b"DCBA"], [b"", b""]), dict(records_skipped=2, tags_left_out=0))
    nq = [(b"n%d" % i, ALL16[i:i + 1 + 3 * i], None, bool(i & 1)) for i in range(5)]
    out["no qualities"] = (b"".join(stored(n, s, q, rev=r) for n, s, q, r in nq), expect([x[0] for x in nq], [x[1] for x in nq], None, [b""] * 5), None)
    out["tags"] = _tag_case()
    return out


def _good(n=b"ok", flag=4):
    return bam_record(n, b"ACGT", b"IIII", flag)


def refusals() -> dict:
    """name -> (records, the index the message must name, a piece of the message)"""
    g = _good()
    return {
        "block_size too small": (g + bam_record(b"bad", b"ACGT", b"IIII", block_size=32 + 4 + 2 + 4 - 1)[:4 + 41], 1, "block_size is too small"),
        "block_size below the fixed fields": (g + g + struct.pack("<I", 8) + b"\0" * 8 + g, 2, "block_size is too small"),
        "l_read_name 0": (g + bam_record(b"", b"ACGT", b"IIII", l_read_name=0, nul=b""), 1, "l_read_name is 0"),
        "name without NUL": (g + g + g + bam_record(b"name", b"ACGT", b"IIII", nul=b"!"), 3, "does not end with NUL"),
        "tag past the record": (g + bam_record(b"t", b"ACGT", b"IIII", tags=tag(b"XY", b"Z", b"runs on")[:-1]), 1, "a tag runs past the end"),
        "B tag past the record": (g + bam_record(b"t", b"ACGT", b"IIII", tags=b"XYBi" + struct.pack("<I", 1 << 30) + b"\0" * 8), 1, "a tag runs past the end"),
        "two bytes of a tag": (bam_record(b"t", b"ACGT", b"IIII", tags=b"XY"), 0, "a tag runs past the end"),
        "unknown tag type": (g + bam_record(b"t", b"ACGT", b"IIII", tags=b"XYq\0\0\0\0"), 1, "a tag of unknown type"),
        "cut inside a record": (g + g + _good(b"cut")[:-3], 2, "ends inside BAM record 2"),
        "two names": (_good(b"a", 0x41) + _good(b"a", 0x81) + _good(b"b", 0x41) + _good(b"c", 0x81), 2, "different names (b and c): is the file grouped by read name"),
        "both first": (_good(b"a", 0x41) + _good(b"a", 0x41), 0, "both carry flag 0x40"),
        "both last": (_good(b"a", 0x81) + _good(b"a", 0x81), 0, "both carry flag 0x80"),
        "lone 0x1": (_good(b"a", 0x41) + _good(b"a", 0x81) + bam_record(b"x", b"", None, 0x100) + _good(b"b", 0x41), 3, "flag 0x1 and no partner"),
        "0x1 mixed": (_good(b"a") + _good(b"b", 0x41) + _good(b"b", 0x81), 1, "mixes records with and without flag 0x1"),
        "l_seq 0": (g + bam_record(b"empty", b"", None, 4), 1, "BAM record 1 (empty): a read without bases"),
        "quality 94": (g + g + bam_record(b"q", b"ACGT", b"III" + bytes([33 + 94])), 2, "BAM record 2 (q): a base quality above 93"),
        "qualities mixed": (g + bam_record(b"nq", b"ACGT", None), 1, "BAM record 1 (nq)"),
    }


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


# ---------------------------------------------------------------------------------------------------------------- the host form

CASE_NAMES = [n for f in FASTQ for n in (f, f + " 0x10")] + ["pairs", "lengths 1-5", "1000 bases, 16 letters", "skipped", "skipped, single-end", "no qualities", "tags"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_form_gives_the_reads(tmp_path, name):
    records, want, counts = cases()[name]
    same_read_sets(bam_to_reads(records, comments=True, host=True), want, (name, "records"))
    if counts is not None:
        assert reads_last_bam_counts() == counts, name
    for block in (777, 60000):                             # records and the header straddle members
        got = read_reads_files(_write(tmp_path, f"b{block}.bam", bam_file(records, block)), comments=True, host=True)
        same_read_sets(got, want, (name, block))
        if counts is not None:
            assert reads_last_bam_counts() == counts, (name, block)
    plain = read_reads_files(_write(tmp_path, "noeof.bam", bam_file(records, 777, eof=False)), host=True)      # without the end-of-file member, without comments
    assert plain.comments is None and np.array_equal(plain.ascii, want.ascii) and np.array_equal(plain.name_blob, want.name_blob)
    if name == "no qualities":
        assert want.qual is None and plain.qual is None


def test_all_cases_are_listed():
    assert sorted(cases()) == sorted(CASE_NAMES)


def test_a_pipe_loads(tmp_path):
    import threading
    records, want, _ = cases()["pairs"]
    fifo = str(tmp_path / "fifo")
    os.mkfifo(fifo)

    def feed():
        with open(fifo, "wb") as f:
            f.write(bam_file(records))
    t = threading.Thread(target=feed); t.start()
    try:
        same_read_sets(read_reads_files(fifo, comments=True, host=True), want, "pipe")
    finally:
        t.join()


@pytest.mark.parametrize("name", list(refusals()))
def test_refusals_name_the_record(tmp_path, name):
    records, index, piece = refusals()[name]
    for what, call in (("records", lambda: bam_to_reads(records, comments=True, host=True)),
                       ("file", lambda: read_reads_files(_write(tmp_path, "bad.bam", bam_file(records)), comments=True, host=True))):
        with pytest.raises(ValueError) as e:
            call()
        msg = str(e.value)
        assert piece in msg and (f"record {index}" in msg or f"records {index} and {index + 1}" in msg), (name, what, msg)


def test_other_refusals(tmp_path):
    records = cases()["four.fq"][0]
    bam = _write(tmp_path, "ok.bam", bam_file(records))
    with pytest.raises(ValueError, match="no mates file is taken beside it"):
        read_reads_files(bam, os.path.join(FIX, "r2.fq"), host=True)
    with pytest.raises(ValueError, match="no mates file is taken beside it"):
        read_reads_files(os.path.join(FIX, "r1.fq"), bam, host=True)
    import zlib
    raw = bam_header() + records
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with pytest.raises(ValueError, match="plain gzip stream"):
        read_reads_files(_write(tmp_path, "gz.bam", c.compress(raw) + c.flush()), host=True)
    whole = bam_header() + records
    with pytest.raises(ValueError, match="ends inside the BAM header"):
        read_reads_files(_write(tmp_path, "hdr.bam", bgzf(whole[:40])), host=True)
    # the reads before the damage are not lost to the message: it names a record behind them
    with pytest.raises(ValueError, match=f"ends inside BAM record {len(split_records(records)) - 1}$"):
        read_reads_files(_write(tmp_path, "cut.bam", bgzf(whole[:-5])), host=True)


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

@pytest.fixture(scope="module")
def core_exe():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_in_core_host")
    src = [os.path.join(HERE, "bam_in_core_host.cpp"), os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc", "bam_in_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def split_records(data: bytes) -> list:
    out, p = [], 0
    while len(data) - p >= 4:
        e = p + 4 + struct.unpack_from("<I", data, p)[0]
        if e > len(data):
            break
        out.append(data[p:e]); p = e
    return out


def test_core_under_sanitizers(core_exe, tmp_path):
    """every record of the well-formed cases decodes to its read, every damaged record is refused with its status, and no byte outside a record is touched"""
    good, want = [], []
    for name, (records, rs, _) in cases().items():
        if name in ("pairs", "skipped", "skipped, single-end"):
            continue                                         # (one record per read, in order, in every other case)
        rd = reads_of(rs)
        recs = split_records(records)
        assert len(recs) == len(rd), name
        good += recs; want += rd
    status = {"block_size too small": 1, "block_size below the fixed fields": 1, "l_read_name 0": 2, "name without NUL": 3, "tag past the record": 4, "B tag past the record": 4,
              "two bytes of a tag": 4, "unknown tag type": 5, "l_seq 0": 6, "quality 94": 7}
    bad = [(split_records(refusals()[n][0])[refusals()[n][1]], st) for n, st in status.items()]
    # a few hundred records with one byte changed: any status, but every access inside the record (the sanitizers say)
    rng = np.random.default_rng(5)
    fuzz = []
    for r in good[:40]:
        for _ in range(8):
            b = bytearray(r); b[4 + int(rng.integers(len(b) - 4))] = int(rng.integers(256)); fuzz.append(bytes(b))
    fi, fo = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    allc = good + [b for b, _ in bad] + fuzz
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(allc)) + b"".join(struct.pack("<I", len(c)) + c for c in allc))
    subprocess.check_call([core_exe, fi, fo])
    with open(fo, "rb") as f:
        res = f.read()
    p = 0

    def u32():
        nonlocal p
        p += 4
        return struct.unpack_from("<I", res, p - 4)[0]

    def take(n):
        nonlocal p
        p += n
        return res[p - n:p]

    def one():
        st = u32()
        if st != 0:
            return (st,)
        role = u32()
        if role not in (1, 2):
            return (0, role)
        sk = u32()
        if sk != 0:
            return (sk,)
        flag, l = u32(), u32()
        seq = take(l)
        hq = u32()
        q = take(l) if hq else None
        name = take(u32())
        cm = take(u32())
        return (0, role, name[:-1], seq, q, cm, u32())
    for k, (n, s, q, c) in enumerate(want):
        r = one()
        assert r[0] == 0 and r[2:6] == (n, s, q, c), (k, r)
    for b, st in bad:
        assert one() == (st,), st
    for _ in fuzz:
        one()
    assert p == len(res)
