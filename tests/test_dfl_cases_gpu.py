"""The one-wave DEFLATE kernel (csrc/deflate_kernels.hip) and the inflate kernel on the case table of tests/dfl_cases.py: the device's members are the host's
bytes, twice in a row, meet the musts of their cases and inflate with zlib; the 41 pieces of the last case also go through bam_sorted_file as BAM records;
every member of the table goes through inflate_members at every launch size."""
import struct
import zlib

import numpy as np
import pytest

import dfl_cases as D

NAMES = [c.name for c in D.cases()]


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_case_on_the_device(hip, name):
    from bwamem_hip.lib import bgzf_compress
    c = next(c for c in D.cases() if c.name == name)
    pieces = [c.data[p:p + D.PIECE] for p in range(0, len(c.data), D.PIECE)]
    assert bgzf_compress(c.data, 0) == bgzf_compress(c.data, 0, host=True) == b"".join(D.stored_member(pc) for pc in pieces)
    host = bgzf_compress(c.data, 1, host=True)
    dev = bgzf_compress(c.data, 1)
    assert dev == host, name
    assert bgzf_compress(c.data, 1) == dev, "twice the same"
    r = D.evaluate(c.data, dev)
    for x, pc in zip(r.pieces, pieces):
        assert zlib.decompress(x.member, 31) == pc == x.text
        if x.form == "dynamic":
            assert [t[2] for t in x.tokens] == x.model
    bad = [k for k, v in c.must.items() if not v(r)]
    assert not bad, (name, bad)


def _records(data: bytes) -> bytes:
    """Unmapped BAM records (no contig, no position: the sort keeps their order) that carry `data` in their sequence and quality fields, 20 000 bytes a record:
    the record stream has the statistics of the data, piece by piece"""
    out = []
    for k, p in enumerate(range(0, len(data), 20000)):
        chunk = data[p:p + 20000]
        l_seq = len(chunk) * 2 // 3
        seq, qual = chunk[:(l_seq + 1) // 2], chunk[(l_seq + 1) // 2:]
        qual = qual[:l_seq] + b"\xff" * (l_seq - len(qual))
        name = b"r%d\0" % k
        body = struct.pack("<iiBBHHHIiii", -1, -1, len(name), 0, 4680, 0, 4, l_seq, -1, -1, 0) + name + seq + qual
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out)


@pytest.mark.gpu
def test_many_pieces_through_the_sorted_file(hip):
    """the 41-piece case as a record stream through bam_sorted_file, one window: the device's file is the host's, and zlib reads the records back"""
    from bwamem_hip.lib import bam_header, bam_sorted_file
    c = next(c for c in D.cases() if c.name.startswith("one call of"))
    contigs = [("chr1", 1000)]
    hdr = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:1000\n"
    recs = _records(c.data)
    h = bam_sorted_file(hdr, contigs, recs, level=1, host=True)
    d = bam_sorted_file(hdr, contigs, recs, level=1)
    assert d[0] == h[0] and d[1] == h[1]
    ms = D.split_members(d[0])
    text = b"".join(zlib.decompress(m, 31) for m in ms)
    assert text == bam_header(hdr, contigs) + recs
    forms = {D.read_member(m).form for m in ms[:-1]}
    assert forms == {"stored", "dynamic"} and len(ms) >= 40


@pytest.mark.gpu
def test_every_member_through_the_inflate_kernel(hip):
    """all members of the table as one member table: status 0 and the text, at every launch size"""
    from bwamem_hip.lib import INFLATE_MEMBER, bgzf_compress, inflate_members
    ms, want = [], []
    for c in D.cases():
        for m in D.split_members(bgzf_compress(c.data, 1, host=True)):
            ms.append(m)
    tab = np.zeros(len(ms), INFLATE_MEMBER)
    blob, text = bytearray(), 0
    for i, m in enumerate(ms):
        crc, isize = struct.unpack("<II", m[-8:])
        blob += b"\xff" * (1 + i % 3)
        tab[i] = (len(blob) + 18, text, len(m) - 26, isize, crc, 0)
        blob += m
        text += isize
    want = b"".join(c.data for c in D.cases())
    assert text == len(want)
    for per_launch in (0, 65, 2, 1):
        out, st = inflate_members(bytes(blob), tab, text, per_launch=per_launch)
        assert not st.any(), (per_launch, np.nonzero(st)[0][:10], st[st != 0][:10])
        assert out.tobytes() == want, per_launch
