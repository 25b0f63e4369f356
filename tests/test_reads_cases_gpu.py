"""The case table of tests/reads_cases.py on the device record parser (csrc/reads_parse.hip): every case against what the reference's kseq_read returned
(tests/golden/reads_input/cases_expected.npz) with the window cut at every byte, the route every case takes at the default window, BGZF inflated on
the device, two files, the refusals through the flag, the seeded corpus against the plain model, and the batch cut of Aligner.align_files."""
import io
import os

import numpy as np
import pytest

import reads_cases
from reads_cases import LONG, SHORT_PAIRS
from test_inflate_gpu import _tune
from test_reads_cases import BLOCK, CASES, PAIRS, REFUSALS, case_forms, check_records, write
from test_reads_input import FIX, bgzf
from test_reads_input_gpu import _set_chunk

WINDOWS = (None, 64, 257, 1000)
LONG_WINDOWS = (None, 65535, 65536, 65537, 4093)
NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = NT4[_c + 32] = _i


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.fixture(scope="module")
def expected():
    """the archive, read once: name -> its arrays as bytes and lists (shared, never changed)"""
    E = np.load(os.path.join(FIX, "cases_expected.npz"))
    out = {}
    for name in list(CASES) + list(PAIRS):
        seq = E[name + "__seq"]
        out[name] = dict(lens=E[name + "__lens"], seq=bytes(seq), codes=bytes(NT4[seq]), names=bytes(E[name + "__names"]), comments=bytes(E[name + "__comments"]),
                         qual=bytes(E[name + "__qual"]))
    return out


def first_difference(W, rs):
    """None, or (field, read) of the first field of rs (comments=True) that is not the archive's, and the first read it differs in"""
    def blob_read(a: bytes, b: bytes):
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        return a[:k].count(0)
    lens, nb = rs.lens, len(W["seq"])
    if not np.array_equal(lens, W["lens"]):
        m = min(len(lens), len(W["lens"]))
        d = np.nonzero(lens[:m] != W["lens"][:m])[0]
        return "lens", int(d[0]) if len(d) else m
    if not np.array_equal(rs.offs, np.concatenate([[0], np.cumsum(W["lens"])[:-1]]).astype(np.uint64)):
        return "offs", 0
    ends = np.cumsum(W["lens"])
    for field, got, want in (("seq", rs.ascii, W["seq"]), ("codes", rs.codes, W["codes"]), ("qual", rs.qual, W["qual"])):
        if field == "qual" and not want:
            if got is not None:
                return "qual", 0
            continue
        if got is None:
            return field, 0
        g = bytes(got[:nb])
        if g != want:
            k = next(i for i, (x, y) in enumerate(zip(g, want)) if x != y)
            return field, int(np.searchsorted(ends, k, side="right"))
    if bytes(rs.name_blob) != W["names"]:
        return "names", blob_read(bytes(rs.name_blob), W["names"])
    if bytes(rs.comments[0]) != W["comments"]:
        return "comments", blob_read(bytes(rs.comments[0]), W["comments"])
    return None


def load(p, q=None):
    from bwamem_hip.aligner import read_reads_files
    from bwamem_hip.lib import reads_last_counts
    rs = read_reads_files(p, q, comments=True)
    return rs, reads_last_counts()


# ---------------------------------------------------------------------------------------------------------------- every window cut, and the routes

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_parser_at_every_window_cut(hip, tmp_path, expected, name):
    """a window begins at a record and is `chunk` bytes long: every chunk from 1 to the text's length + 1 puts the cut at every byte of every record and
    walks the doubling growth.  At the default window the case takes its declared route."""
    text, kind, route = CASES[name]
    W = expected[name]
    p = write(tmp_path, name, text)
    rs, cnt = load(p)
    assert first_difference(W, rs) is None, (name, "default window") + first_difference(W, rs)
    assert cnt["records"] == len(W["lens"]) and cnt["text_bytes"] == len(text), (name, cnt)
    if route == "device":
        assert cnt["host_windows"] == 0 and cnt["device_windows"] > 0, (name, "a regular file went to the host walker", cnt)
    else:
        assert cnt["host_windows"] > 0, (name, "the kernels took a window that is the walker's", cnt)
    try:
        for chunk in (LONG_WINDOWS[1:] if name in LONG else range(1, len(text) + 2)):
            _set_chunk(chunk)
            rs, cnt = load(p)
            d = first_difference(W, rs)
            assert d is None, (name, "chunk", chunk, "field", d[0], "read", d[1])
            assert cnt["records"] == len(W["lens"]), (name, chunk, cnt)
    finally:
        _set_chunk(0)


# ---------------------------------------------------------------------------------------------------------------- BGZF inflated on the device

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_inflate(hip, tmp_path, expected, name):
    """the text never was on the host: the 64-byte peek decides FASTA or FASTQ, the rest of a window moves between two buffers, and a flagged window is
    mirrored for the walker"""
    text, kind, route = CASES[name]
    W = expected[name]
    p = write(tmp_path, name + ".bgzf", bgzf(text, 0xff00 if name in LONG else BLOCK))
    _tune(b"INFLATE_DEVICE", 1)
    try:
        for chunk in WINDOWS:
            _set_chunk(chunk)
            rs, cnt = load(p)
            d = first_difference(W, rs)
            assert d is None, (name, "chunk", chunk, "field", d[0], "read", d[1])
            assert cnt["device_inflate_members"] > 0 and cnt["host_inflate_members"] == 0 and cnt["records"] == len(W["lens"]), (name, chunk, cnt)
            if chunk is None and route == "host":
                assert cnt["host_windows"] > 0, (name, cnt)
            if chunk is None and "_lead_nl" in name:         # both sides of the peek: beyond 63 blank bytes the host looks
                assert (cnt["host_windows"] > 0) == (int(name.split("_lead_nl")[1]) >= 64), (name, cnt)
    finally:
        _set_chunk(0)
        _tune(b"INFLATE_DEVICE", None)


# ---------------------------------------------------------------------------------------------------------------- two files

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_device_parser_two_files(hip, tmp_path, expected, name):
    t1, t2 = PAIRS[name]
    W = expected[name]
    f1, f2 = case_forms(tmp_path, name + ".1", t1), case_forms(tmp_path, name + ".2", t2)
    try:
        for chunk in WINDOWS:
            _set_chunk(chunk)
            for a, b in (("plain", "plain"), ("gz", "bgzf"), ("bgzf", "bgzf")):
                if name in SHORT_PAIRS:
                    short, n_pairs = SHORT_PAIRS[name]
                    first, other = (f1[a], f2[b]) if short == 0 else (f2[b], f1[a])
                    with pytest.raises(ValueError) as ei:
                        load(f1[a], f2[b])
                    assert f"{first} ends before {other} (after {n_pairs} pairs)" in str(ei.value), (name, chunk, a, b)
                    rs = ei.value.partial
                    assert len(rs) == 2 * n_pairs, (name, chunk, a, b)
                else:
                    rs, cnt = load(f1[a], f2[b])
                d = first_difference(W, rs)
                assert d is None, (name, "chunk", chunk, a, b, "field", d[0], "read", d[1])
    finally:
        _set_chunk(0)


# ---------------------------------------------------------------------------------------------------------------- refusals

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_device_refusals_are_the_walkers(hip, tmp_path, name):
    from bwamem_hip.aligner import read_reads_files
    text, piece = REFUSALS[name]
    p = write(tmp_path, name, text)
    with pytest.raises(ValueError) as eh:
        read_reads_files(p, comments=True, host=True)
    assert piece in str(eh.value)
    try:
        for chunk in (None, 64):
            _set_chunk(chunk)
            with pytest.raises(ValueError) as e:
                read_reads_files(p, comments=True)
            assert str(e.value) == str(eh.value), (name, chunk)
    finally:
        _set_chunk(0)


# ---------------------------------------------------------------------------------------------------------------- the corpus

CORPUS = reads_cases.random_texts()


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, len(CORPUS), 25))
def test_device_parser_equals_the_model_on_the_corpus(hip, tmp_path, first):
    from bwamem_hip.aligner import read_reads_files
    from bwamem_hip.lib import reads_last_counts
    try:
        for i in range(first, min(first + 25, len(CORPUS))):
            text = CORPUS[i]
            status, want = reads_cases.model_outcome(text)
            p = write(tmp_path, "t", text)
            for chunk in (None, 64, 17):
                _set_chunk(chunk)
                if status == "refused":
                    with pytest.raises(ValueError) as ei:
                        read_reads_files(p, comments=True)
                    assert want in str(ei.value), (i, chunk, text)
                    continue
                rs = read_reads_files(p, comments=True)
                cnt = reads_last_counts()
                check_records(want, rs, (i, chunk, text))
                assert bytes(rs.codes[:int(rs.lens.sum())]) == bytes(NT4[np.frombuffer(reads_cases.packed(want)["seq"], np.uint8)]), (i, chunk, text)
                if chunk is None:
                    route = reads_cases.device_route(text)
                    assert (cnt["host_windows"] == 0 and cnt["device_windows"] > 0) if route == "device" else cnt["host_windows"] > 0, (i, route, cnt, text)
    finally:
        _set_chunk(0)


# ---------------------------------------------------------------------------------------------------------------- the batch cut

def _concatenated(kind: str, expected):
    """the "device" cases of one kind in one file (the two long-line cases stay out: their reads are beyond what the aligner takes; a text without its last
    '\\n' can only stand last) and their recorded reads: (text, [(name, seq, qual)])"""
    names = [n for n in sorted(CASES) if CASES[n][1] == kind and CASES[n][2] == "device" and n not in LONG]
    names = [n for n in names if CASES[n][0].endswith(b"\n")] + [n for n in names if not CASES[n][0].endswith(b"\n")][:1]
    reads = []
    for n in names:
        W = expected[n]
        ends = np.cumsum(W["lens"]).tolist()
        qn = W["names"].split(b"\0")[:-1]
        for k, (e, ln) in enumerate(zip(ends, W["lens"].tolist())):
            reads.append((qn[k], W["seq"][e - ln:e], W["qual"][e - ln:e]))
    return b"".join(CASES[n][0] for n in names), reads


_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _check_sam(sam: bytes, reads, what):
    """the primary record of every read, in the order of the reads: QNAME, SEQ and QUAL as recorded, turned on the reverse strand"""
    rows = [ln.split(b"\t") for ln in sam.split(b"\n") if ln and not ln.startswith(b"@")]
    rows = [r for r in rows if not int(r[1]) & 0x900]
    assert [r[0] for r in rows] == [r[0] for r in reads], what
    for row, (qn, seq, qual) in zip(rows, reads):
        want = bytes(b"ACGTN"[c] for c in NT4[np.frombuffer(seq, np.uint8)])
        rev = bool(int(row[1]) & 16)
        assert row[9] == (want.translate(_COMP)[::-1] if rev else want), (what, qn)
        assert row[10] == ((qual[::-1] if rev else qual) if qual else b"*"), (what, qn)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fa", "fq"])
def test_batches_are_cut_from_one_parse(hip, tmp_path, expected, kind):
    """align_files with batch_reads 1, 2, 3 and 7 over 64-byte windows: the pump parses a window again until it holds the batch, and every read comes out once,
    in order, with its own bases and qualities"""
    from test_bam_gpu import PREFIX
    from bwamem_hip.aligner import Aligner
    text, reads = _concatenated(kind, expected)
    p = write(tmp_path, "all." + kind, text)
    al = Aligner(PREFIX, n_threads=4)
    try:
        _set_chunk(64)
        for batch_reads in (1, 2, 3, 7):
            buf = io.BytesIO()
            n = al.align_files(p, out=buf, batch_reads=batch_reads)
            assert n == len(reads) and al.last_stats.n_batches == -(-len(reads) // batch_reads), (kind, batch_reads, n, al.last_stats.n_batches)
            _check_sam(buf.getvalue(), reads, (kind, batch_reads))
    finally:
        _set_chunk(0)
        al.close()


@pytest.mark.gpu
def test_a_pair_is_never_split_across_batches(hip, tmp_path, expected):
    """paired=True on an interleaved file of ten reads over 64-byte windows.  batch_reads 3: a paired run takes an even number of reads, the odd count
    rounded down, so five batches of one pair.  chunk_bases 5: a batch is complete when it holds 5 bases and an even count (bseq_read's rule), which the
    read lengths make differ from the cut without it: 2 + 4 + 2 + 2 reads, not 3 + 2 + 1 + 2 + 2"""
    from test_bam_gpu import PREFIX
    from bwamem_hip.aligner import Aligner
    t1, t2 = PAIRS["pair_fq_lf_crlf"]
    W = expected["pair_fq_lf_crlf"]

    def records(t, eol):
        lines = t.split(eol)[:-1]
        return [eol.join(lines[k:k + 4]) + eol for k in range(0, len(lines), 4)]
    text = b"".join(a + b for a, b in zip(records(t1, b"\n"), records(t2, b"\r\n")))
    ends = np.cumsum(W["lens"]).tolist()
    reads = [(qn, W["seq"][e - ln:e], W["qual"][e - ln:e]) for qn, e, ln in zip(W["names"].split(b"\0")[:-1], ends, W["lens"].tolist())]
    assert len(reads) == 10

    def batches(lens, chunk, even):
        n, size, cnt = 0, 0, 0
        for ln in lens:
            size += ln; cnt += 1
            if size >= chunk and (not even or cnt % 2 == 0):
                n, size, cnt = n + 1, 0, 0
        return n + (cnt > 0)
    lens = W["lens"].tolist()
    assert batches(lens, 5, True) == 4 and batches(lens, 5, False) == 5
    p = write(tmp_path, "interleaved.fq", text)
    al = Aligner(PREFIX, n_threads=4)
    try:
        _set_chunk(64)
        for kw, want in ((dict(batch_reads=3), 5), (dict(chunk_bases=5), 4)):
            buf = io.BytesIO()
            n = al.align_files(p, out=buf, paired=True, **kw)
            assert n == 10 and al.last_stats.n_batches == want, (kw, n, al.last_stats.n_batches)
            _check_sam(buf.getvalue(), reads, ("paired", kw))
    finally:
        _set_chunk(0)
        al.close()
