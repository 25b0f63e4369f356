"""Read input as users have it (bmh_reads_load_files, host walker): multi-line records, CR LF, gzip / concatenated gzip / BGZF, two files, pipes --
against what the reference's kseq_read returned for the same files (tests/golden/reads_input/expected.npz, scripts/record_reads_golden.py), against
today's loader where both take the file, and the refusals with their messages.  The device parser has the same checks in test_reads_input_gpu.py.

Not tested: zlib missing at run time (the message of csrc/reads_src.cpp's dlopen) -- it cannot be simulated without changing how the process starts."""
import os
import struct
import threading
import zlib

import numpy as np
import pytest

from bwamem_hip.aligner import read_reads, read_reads_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "reads_input")
FIXTURES = ["ml60.fa", "ml80_crlf.fa", "single.fa", "four.fq", "crlf.fq", "ml.fq", "r1.fq", "r2.fq"]


# ---------------------------------------------------------------------------------------------------------------- compressed forms, written here

def _deflate_raw(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def gzip_member(data: bytes) -> bytes:
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + _deflate_raw(data) + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def bgzf(data: bytes, block: int = 777) -> bytes:
    """BGZF: gzip members with the 'BC' extra field (BSIZE = member size - 1), payloads of `block` bytes, and the empty end-of-file member"""
    out = []
    for i in list(range(0, len(data), block)) + [None]:
        d = b"" if i is None else data[i:i + block]
        z = _deflate_raw(d)
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(z) + 25) + z + struct.pack("<II", zlib.crc32(d) & 0xFFFFFFFF, len(d)))
    return b"".join(out)


def forms(tmp_path, name: str, text: bytes) -> dict:
    """the text as a plain file, one gzip member, two concatenated members and BGZF with blocks that records straddle"""
    cut = len(text) // 2 + 7
    out = {}
    for tag, data in (("plain", text), ("gz", gzip_member(text)), ("gz2", gzip_member(text[:cut]) + gzip_member(text[cut:])), ("bgzf", bgzf(text))):
        p = str(tmp_path / f"{name}.{tag}")
        with open(p, "wb") as f:
            f.write(data)
        out[tag] = p
    return out


def fixture_text(name: str) -> bytes:
    with open(os.path.join(FIX, name), "rb") as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------- comparisons

def check_expected(E, key: str, rs):
    """rs (comments=True) against the reference's records of fixture `key`, field for field"""
    lens = E[key + "__lens"]
    assert np.array_equal(rs.lens, lens), key
    nb = int(lens.sum())
    assert np.array_equal(rs.offs, np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)), key
    assert bytes(rs.ascii[:nb]) == bytes(E[key + "__seq"]), key
    assert bytes(rs.name_blob) == bytes(E[key + "__names"]), key
    assert bytes(rs.comments[0]) == bytes(E[key + "__comments"]), key
    if len(E[key + "__qual"]):
        assert bytes(rs.qual[:nb]) == bytes(E[key + "__qual"]), key
    else:
        assert rs.qual is None, key
    table = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        table[c] = table[c + 32] = i
    assert np.array_equal(rs.codes[:nb], table[E[key + "__seq"]]), key


def same_read_sets(a, b, what=""):
    for k in ("ascii", "codes", "offs", "lens", "name_blob", "name_off", "qual"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)), (what, k)
    assert (a.comments is None) == (b.comments is None), what
    if a.comments is not None:
        assert np.array_equal(a.comments[0], b.comments[0]) and np.array_equal(a.comments[1], b.comments[1]), (what, "comments")


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(FIX, "expected.npz"))


# ---------------------------------------------------------------------------------------------------------------- the host walker

@pytest.mark.parametrize("name", FIXTURES)
def test_host_walker_equals_the_reference_in_every_form(tmp_path, expected, name):
    for tag, p in forms(tmp_path, name, fixture_text(name)).items():
        check_expected(expected, name, read_reads_files(p, comments=True, host=True))
    rs = read_reads_files(os.path.join(FIX, name), host=True)              # without comments: none kept
    assert rs.comments is None and np.array_equal(rs.lens, expected[name + "__lens"])


def test_host_walker_two_files_in_every_form(tmp_path, expected):
    f1, f2 = forms(tmp_path, "r1.fq", fixture_text("r1.fq")), forms(tmp_path, "r2.fq", fixture_text("r2.fq"))
    for t1, t2 in (("plain", "plain"), ("gz", "plain"), ("bgzf", "gz2"), ("bgzf", "bgzf")):
        check_expected(expected, "r1.fq+r2.fq", read_reads_files(f1[t1], f2[t2], comments=True, host=True))


@pytest.mark.parametrize("name", ["single.fa", "four.fq"])
def test_host_walker_equals_todays_loader(name):
    p = os.path.join(FIX, name)
    for cm in (False, True):
        same_read_sets(read_reads_files(p, comments=cm, host=True), read_reads(p, comments=cm), name)


def _records_of(text: bytes):
    recs, lines = [], text.split(b"\n")
    for k in range(0, len(lines) - 1, 4):
        recs.append(lines[k:k + 4])
    return recs


def test_two_files_equal_the_interleaved_file(tmp_path):
    r1, r2 = _records_of(fixture_text("r1.fq")), _records_of(fixture_text("r2.fq"))
    p = str(tmp_path / "interleaved.fq")
    with open(p, "wb") as f:
        for a, b in zip(r1, r2):
            f.write(b"\n".join(a) + b"\n" + b"\n".join(b) + b"\n")
    two = read_reads_files(os.path.join(FIX, "r1.fq"), os.path.join(FIX, "r2.fq"), comments=True, host=True)
    same_read_sets(two, read_reads_files(p, comments=True, host=True), "interleaved")
    same_read_sets(two, read_reads(p, comments=True), "interleaved, today's loader")


def test_a_pipe_loads(tmp_path, expected):
    for name in ("ml60.fa", "four.fq"):
        for data in (fixture_text(name), bgzf(fixture_text(name)), gzip_member(fixture_text(name))):
            fifo = str(tmp_path / "fifo")
            os.mkfifo(fifo)

            def feed():
                with open(fifo, "wb") as f:
                    f.write(data)
            t = threading.Thread(target=feed)
            t.start()
            try:
                check_expected(expected, name, read_reads_files(fifo, comments=True, host=True))
            finally:
                t.join()
                os.unlink(fifo)


# ---------------------------------------------------------------------------------------------------------------- refusals

def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def test_refusals(tmp_path, expected):
    fa, r1, r2 = os.path.join(FIX, "single.fa"), os.path.join(FIX, "r1.fq"), os.path.join(FIX, "r2.fq")
    with pytest.raises(ValueError, match="holds FASTQ records and .* FASTA records"):
        read_reads_files(r1, fa, host=True)
    other = _write(tmp_path, "renamed.fq", fixture_text("r2.fq").replace(b"@pair5/2", b"@other5/2"))
    with pytest.raises(ValueError, match="pair 5 has different names in the two files: pair5 and other5"):
        read_reads_files(r1, other, host=True)
    short = _write(tmp_path, "short.fq", b"\n".join(fixture_text("r2.fq").split(b"\n")[:4 * 9]) + b"\n")
    for a, b, who in ((r1, short, "short.fq ends before .*r1.fq"), (short, r2, "short.fq ends before .*r2.fq")):
        with pytest.raises(ValueError, match=who + r" \(after 9 pairs\)") as ei:
            read_reads_files(a, b, comments=True, host=True)
        part = ei.value.partial                                     # the complete pairs come with the refusal
        assert len(part) == 18
        if a == r1:
            assert bytes(part.name_blob) == bytes(expected["r1.fq+r2.fq__names"])[:len(part.name_blob)]
    gz = gzip_member(fixture_text("four.fq"))
    with pytest.raises(ValueError, match="the gzip stream is truncated"):
        read_reads_files(_write(tmp_path, "cut.gz", gz[:len(gz) // 2]), host=True)
    # bytes behind the last member that begin no member (zero padding) are ignored, as gzread ignores them
    check_expected(expected, "four.fq", read_reads_files(_write(tmp_path, "pad.gz", gz + b"\0" * 512), comments=True, host=True))
    # a gzip member whose extra field is not BGZF's is a gzip stream
    text = fixture_text("four.fq")
    other = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 24) + b"XY" + struct.pack("<H", 20) + b"x" * 20 + gzip_member(text)[10:]
    check_expected(expected, "four.fq", read_reads_files(_write(tmp_path, "extra.gz", other), comments=True, host=True))
    bz = bgzf(fixture_text("four.fq"))
    with pytest.raises(ValueError, match="truncated"):
        read_reads_files(_write(tmp_path, "cut.bgzf", bz[:len(bz) // 2 + 5]), host=True)
    with pytest.raises(ValueError, match="quality line whose length differs"):
        read_reads_files(_write(tmp_path, "q.fq", b"@a\nACGT\n+\nIIIII\n@b\nAC\n+\nII\n"), host=True)
    with pytest.raises(ValueError, match="last record is truncated"):
        read_reads_files(_write(tmp_path, "t.fq", b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nII"), host=True)
    with pytest.raises(ValueError, match="empty sequence"):
        read_reads_files(_write(tmp_path, "e.fq", b"@a\n\n+\n\n"), host=True)
    with pytest.raises(ValueError, match="FASTA and FASTQ records mixed"):
        read_reads_files(_write(tmp_path, "m.fq", b"@a\nACGT\n+\nIIII\n>b\nACGT\n"), host=True)
    with pytest.raises(ValueError, match="cannot open"):
        read_reads_files(str(tmp_path / "absent.fq"), host=True)


def test_existing_loaders_keep_their_refusals(tmp_path):
    """the new entry points take multi-line records; the old ones refuse them as before"""
    with pytest.raises(ValueError, match="multi-line"):
        read_reads(os.path.join(FIX, "ml.fq"))
    assert len(read_reads_files(os.path.join(FIX, "ml.fq"), host=True)) == 14
