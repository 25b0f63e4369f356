"""Mates collated by name (collate=True): a paired BAM in any record order as read input -- the host form, which is the definition the device form must equal
(tests/test_bam_collate_gpu.py runs the same tables on the device).

The expected reads come from `model` below, a restatement of the definition (include/bwamem_hip.h): kept records in file order; a record whose name is open
closes that record, the pair completes there and pairs come in the order of completion; any other record opens its name; an open record at the end is refused.
The core (csrc/bam_collate_core.h) also runs as a stand-alone program under AddressSanitizer and UBSan (tests/bam_collate_host.cpp)."""
import collections
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from bwamem_hip.aligner import bam_to_reads, read_reads_files
from bwamem_hip.lib import reads_last_bam_counts, reads_last_collate_counts
from test_bam_input import bam_file, bam_header, reads_of, stored, tag
from test_reads_input import bgzf
from test_reads_input_gpu import _set_chunk

HERE = os.path.dirname(os.path.abspath(__file__))

# a record as the tests write it: the read in sequencing orientation, stored reverse-complemented under 0x10 when rev; comment: what -C makes of its tags
Rec = collections.namedtuple("Rec", "name seq qual flag tags rev comment rg")


def rec(name, seq, qual, flag, tags=b"", rev=False, comment=b"", rg=None):
    return Rec(name, seq, qual, flag, tags + (tag(b"RG", b"Z", rg) if rg is not None else b""), rev, comment, rg)


def encode(r: Rec) -> bytes:
    return stored(r.name, r.seq, r.qual, r.flag, r.tags, r.rev)


def blob(recs) -> bytes:
    return b"".join(encode(r) for r in recs)


Model = collections.namedtuple("Model", "reads pairs adjacent peak_records peak_bytes refusal over_cap")


def model(recs, cap=8 << 30) -> Model:
    """the definition.  reads: the records of the pairs in the order of completion (0x40 first); refusal: None, ("role", j, i), ("open", smallest index) or
    ("cap", index) -- reads then holds the pairs completed before it.  The open bytes are held against the cap at every completion (the record named is the first
    since the completion before it that went beyond), so the peaks are those up to the last completion."""
    open_, reads, adjacent, seq = {}, [], 0, 0
    n_open = b_open = peak_n = peak_b = at_n = at_b = 0
    over = None
    size = [len(encode(r)) for r in recs]
    for i, r in enumerate(recs):
        if r.flag & 0x900:
            continue
        if r.name in open_:
            j, jseq = open_[r.name]
            if over is not None:
                return Model(reads, len(reads) // 2, adjacent, at_n, at_b, ("cap", over), over)
            if (recs[j].flag & 0xc0) == (r.flag & 0xc0):
                return Model(reads, len(reads) // 2, adjacent, at_n, at_b, ("role", j, i), None)
            del open_[r.name]
            n_open -= 1; b_open -= size[j]
            reads += [recs[j], r] if recs[j].flag & 0x40 else [r, recs[j]]
            adjacent += jseq + 1 == seq
            at_n, at_b = peak_n, peak_b
        else:
            open_[r.name] = (i, seq)
            n_open += 1; b_open += size[i]
            peak_n, peak_b = max(peak_n, n_open), max(peak_b, b_open)
            if b_open > cap and over is None:
                over = i
        seq += 1
    refusal = ("open", min(j for j, _ in open_.values())) if open_ else None
    return Model(reads, len(reads) // 2, adjacent, at_n, at_b, refusal, None)


def as_reads(recs):
    return [(r.name, r.seq, r.qual, r.comment) for r in recs]


# ---------------------------------------------------------------------------------------------------------------- the cases

def _seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def _qual(rng, n):
    return bytes(rng.integers(35, 74, n, dtype=np.uint8))


def _pair(rng, name, n1=20, n2=17, qual=True, rev=(False, True), tags=(b"", b""), comments=(b"", b""), rg=None):
    s1, s2 = _seq(rng, n1), _seq(rng, n2)
    return (rec(name, s1, _qual(rng, n1) if qual else None, 0x41 | (0x20 if rev[1] else 0), tags[0], rev[0], comments[0], rg),
            rec(name, s2, _qual(rng, n2) if qual else None, 0x81 | (0x20 if rev[0] else 0), tags[1], rev[1], comments[1], rg))


def _skipped(rng, name, flag):
    return rec(name, _seq(rng, 9), _qual(rng, 9), flag)


def _random_case(n_pairs, seed, tags=False, groups=None, skipped=True):
    """n_pairs pairs in a random record order, secondary and supplementary records (some with a pair's own name) strewn between them"""
    rng = np.random.default_rng(seed)
    recs = []
    for k in range(n_pairs):
        name = b"r%05d:%d" % (k, seed)
        tg, cm = (b"", b""), (b"", b"")
        if tags and k % 3:
            bc = b"ACGT"[k % 4:k % 4 + 1] * 5
            tg, cm = (tag(b"BC", b"Z", bc) + tag(b"NM", b"C", 1), tag(b"XY", b"i", k)), (b"BC:Z:" + bc, b"XY:i:%d" % k)
        recs += _pair(rng, name, int(rng.integers(1, 40)), int(rng.integers(1, 40)), rev=(bool(k & 1), bool(k & 2)), tags=tg, comments=cm, rg=None if groups is None else groups[k % len(groups)])
    order = rng.permutation(len(recs))
    out = []
    for i in order:
        out.append(recs[i])
        if skipped and rng.random() < 0.1:
            out.append(_skipped(rng, recs[int(rng.integers(len(recs)))].name if rng.random() < 0.5 else b"other", (0x100, 0x800)[int(rng.integers(2))] | (0x41, 0x81)[int(rng.integers(2))]))
    return out


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    rng = np.random.default_rng(11)
    A, B, C, D = (_pair(rng, n) for n in (b"A", b"B", b"C", b"D"))
    out = {}
    out["grouped"] = [r for k in range(6) for r in (_pair(rng, b"g%d" % k) if k & 1 else _pair(rng, b"g%d" % k)[::-1])]
    out["A1 B1 A2 B2"] = [A[0], B[0], A[1], B[1]]
    out["A1 B1 B2 A2"] = [A[0], B[0], B[1], A[1]]
    out["0x80 first"] = [A[1], B[1], C[0], A[0], C[1], B[0]]
    rv = [_pair(rng, b"rv%d" % k, 21, 8, rev=((k & 1) == 1, (k & 2) == 2)) for k in range(4)]
    out["reverse strand"] = [rv[0][0], rv[1][1], rv[2][0], rv[3][0], rv[1][0], rv[0][1], rv[3][1], rv[2][1]]
    nq = [_pair(rng, b"nq%d" % k, 21, 8, qual=False, rev=((k & 1) == 1, (k & 2) == 2)) for k in range(4)]
    out["reverse strand, no qualities"] = [nq[0][0], nq[1][1], nq[2][0], nq[3][0], nq[1][0], nq[0][1], nq[3][1], nq[2][1]]
    out["skipped between mates"] = [A[0], _skipped(rng, b"x", 0x141), B[0], _skipped(rng, b"y", 0x881), A[1], _skipped(rng, b"z", 0x900 | 0x41), B[1]]
    out["skipped with the pair's name"] = [A[0], _skipped(rng, b"A", 0x181), _skipped(rng, b"A", 0x841), B[0], _skipped(rng, b"B", 0x141), A[1], _skipped(rng, b"A", 0x881), B[1], _skipped(rng, b"B", 0x981)]
    P1, P2, P3 = _pair(rng, b"ab"), _pair(rng, b"abc"), _pair(rng, b"a")
    out["a name is a prefix of another"] = [P2[0], P1[0], P3[1], P1[1], P3[0], P2[1]]
    L1, L2 = _pair(rng, b"read:1:x"), _pair(rng, b"read:1:y")
    out["names differ in the last byte"] = [L1[0], L2[0], L2[1], L1[1]]
    N1, N2, N3 = _pair(rng, b"q"), _pair(rng, b"n" * 254), _pair(rng, b"n" * 253 + b"m")
    out["names of 1 and 254 bytes"] = [N2[0], N1[1], N3[1], N2[1], N1[0], N3[0]]
    firsts = [_pair(rng, b"f%04d" % k, 12, 9) for k in range(1000)]
    out["1000 first mates, then the second mates reversed"] = [p[0] for p in firsts] + [p[1] for p in firsts[::-1]]
    out["2000 pairs, random order"] = _random_case(2000, 3)
    out["2000 pairs, random order, tags"] = _random_case(2000, 4, tags=True)
    # waves: ten first mates, then their partners, again and again with pairs in between -- the pool fills and empties, and its slots are taken again
    waves = []
    for wv in range(6):
        ps = [_pair(rng, b"w%d_%d" % (wv, k), 15, 15) for k in range(10 + wv)]
        waves += [p[0] for p in ps] + [r for r in _pair(rng, b"mid%d" % wv)] + [p[1] for p in ps[::2]] + [p[1] for p in ps[1::2]]
    out["slots free up and refill"] = waves
    return out


GROUPS = ["lane1", "lane2", "l"]
RG_HEADER = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@RG\tID:%s\tSM:s\n" % g.encode() for g in GROUPS)      # the header of a file read under its own groups


@functools.lru_cache(maxsize=None)
def group_case():
    return _random_case(2000, 5, tags=True, groups=[g.encode() for g in GROUPS])


CASES = list(cases())
# explicit expectations beside the model's, for the cases the definition is explained with
ORDER = {"A1 B1 A2 B2": [b"A", b"B"], "A1 B1 B2 A2": [b"B", b"A"], "0x80 first": [b"A", b"C", b"B"]}


def cap_case():
    """complete pairs between first mates whose partners never come: every prefix is consumed, and the pool grows by a record per round"""
    rng = np.random.default_rng(17)
    out = []
    for k in range(40):
        out += list(_pair(rng, b"p%02d" % k)) + [_pair(rng, b"u%02d" % k)[0]]
    return out


@functools.lru_cache(maxsize=None)
def refusals() -> dict:
    """name -> (records, what the message must hold, keyword arguments, the pairs delivered in `partial` or None)"""
    rng = np.random.default_rng(23)
    A, B, C, D, X = (_pair(rng, n) for n in (b"A", b"B", b"C", b"D", b"X"))
    A2 = _pair(rng, b"A")
    out = {}
    out["a repeated role while open"] = ([A[0], X[0], X[1], A2[0], B[0], B[1]], ["BAM records 0 and 3 (A) both carry flag 0x40"], {}, None)
    out["an open record at the end"] = ([A[0], B[0], B[1], C[1], D[0], C[0]], ["BAM record 0 (A): flag 0x1 and no partner"], {}, [b"B", b"C"])
    g1, g2 = _pair(rng, b"G", rg=b"lane1"), _pair(rng, b"G", rg=b"lane2")
    h = _pair(rng, b"H", rg=b"lane2")
    out["a pair of two read groups"] = ([g1[0], h[0], h[1], g2[1]], ["BAM records 0 and 3 (G) name different read groups (lane1 and lane2)"], dict(read_groups=GROUPS), None)
    cc = cap_case()
    m = model(cc, 1024)
    assert m.refusal[0] == "cap" and m.pairs >= 5                       # (by construction: several prefixes are consumed before the cap is reached)
    out["the pool beyond collate_mem"] = (cc, ["BAM record %d:" % m.over_cap, "--collate-mem 1024 bytes"], dict(collate_mem=1024), None)
    return out


REFUSALS = list(refusals())


def check_counts(m: Model, what):
    c = reads_last_collate_counts()
    assert (c["pairs"], c["pairs_adjacent"], c["open_records_peak"], c["open_bytes_peak"]) == (m.pairs, m.adjacent, m.peak_records, m.peak_bytes), (what, c, m[1:])
    return c


def _file(tmp_path, name, recs, block=777, header_text=None):
    p = str(tmp_path / (name.replace(" ", "_").replace(",", "") + ".bam"))
    with open(p, "wb") as f:
        f.write(bam_file(blob(recs), block) if header_text is None else bgzf(bam_header(header_text, ()) + blob(recs), block))
    return p


# ---------------------------------------------------------------------------------------------------------------- the host form

@pytest.mark.parametrize("name", CASES)
def test_host_form_follows_the_definition(tmp_path, name):
    recs = cases()[name]
    m = model(recs)
    assert m.refusal is None and m.pairs == sum(1 for r in recs if not r.flag & 0x900) // 2
    if name in ORDER:
        assert [r.name for r in m.reads[::2]] == ORDER[name]
    want = as_reads(m.reads)
    got = bam_to_reads(blob(recs), comments=True, host=True, collate=True)
    assert reads_of(got) == want, name
    check_counts(m, name)
    assert reads_last_bam_counts()["records_skipped"] == sum(1 for r in recs if r.flag & 0x900)
    if name == "1000 first mates, then the second mates reversed":
        assert reads_last_collate_counts()["open_records_peak"] == 1000
    if name == "grouped":
        assert reads_of(bam_to_reads(blob(recs), comments=True, host=True)) == want
        assert m.adjacent == m.pairs
    path = _file(tmp_path, name, recs)
    try:
        for chunk in (None, 257, 64):
            _set_chunk(chunk)
            assert reads_of(read_reads_files(path, comments=True, host=True, collate=True)) == want, (name, chunk)
            check_counts(m, (name, chunk))
            assert reads_last_bam_counts()["records_skipped"] == sum(1 for r in recs if r.flag & 0x900), (name, chunk)
    finally:
        _set_chunk(0)
    assert reads_of(bam_to_reads(blob(recs), host=True, collate=True, comments=True)) == want          # (the call leaves no state behind)


def test_collate_off_is_todays_refusal(tmp_path):
    recs = cases()["A1 B1 A2 B2"]
    with pytest.raises(ValueError, match=r"BAM records 0 and 1 carry different names \(A and B\): is the file grouped by read name\?"):
        bam_to_reads(blob(recs), host=True)
    with pytest.raises(ValueError, match=r"BAM records 0 and 1 carry different names \(A and B\): is the file grouped by read name\?"):
        read_reads_files(_file(tmp_path, "off", recs), host=True)


def test_read_groups(tmp_path):
    recs = group_case()
    m = model(recs)
    got = bam_to_reads(blob(recs), comments=True, host=True, collate=True, read_groups=GROUPS)
    assert reads_of(got) == as_reads(m.reads)
    assert [GROUPS[g].encode() for g in got.groups] == [r.rg for r in m.reads]
    check_counts(m, "read groups")
    groups_through_the_file_reader(tmp_path, True)


def groups_through_the_file_reader(tmp_path, host, chunks=(None, 257, 64)):
    """the file under its own header's read groups: at small windows a pair's first record waits in the pool, and its group is compared when its partner comes"""
    recs = group_case()
    m = model(recs)
    path = _file(tmp_path, "groups", recs, header_text=RG_HEADER)
    try:
        for chunk in chunks:
            _set_chunk(chunk)
            got = read_reads_files(path, comments=True, host=host, collate=True, keep_rg=True)
            assert reads_of(got) == as_reads(m.reads), chunk
            assert [GROUPS[g].encode() for g in got.groups] == [r.rg for r in m.reads], chunk
            check_counts(m, ("read groups", chunk))
    finally:
        _set_chunk(0)


def test_single_end(tmp_path):
    rng = np.random.default_rng(2)
    recs = [rec(b"s%d" % (k // 2), _seq(rng, 11), _qual(rng, 11), (0, 16)[k & 1], rev=bool(k & 1)) for k in range(9)]         # (names repeat: nothing is collated)
    want = reads_of(bam_to_reads(blob(recs), comments=True, host=True))
    assert want == as_reads(recs)
    assert reads_of(bam_to_reads(blob(recs), comments=True, host=True, collate=True)) == want
    assert reads_of(read_reads_files(_file(tmp_path, "single", recs), comments=True, host=True, collate=True)) == want
    assert reads_last_collate_counts()["pairs"] == 0


def run_refusal(name, host, tmp_path, chunk=None, file_only=False):
    """the messages of the one-window reader and of the file reader for a case of REFUSALS"""
    recs, frags, kw, partial = refusals()[name]
    m = model(recs, kw.get("collate_mem", 8 << 30))
    msgs = []
    calls = [] if file_only else [lambda: bam_to_reads(blob(recs), comments=True, host=host, collate=True, **kw)]
    if "read_groups" in kw:                                # (the file reader takes the groups from the file's own header)
        path = _file(tmp_path, name, recs, header_text=RG_HEADER)
        calls.append(lambda: read_reads_files(path, comments=True, host=host, collate=True, keep_rg=True))
    else:
        path = _file(tmp_path, name, recs)
        calls.append(lambda: read_reads_files(path, comments=True, host=host, collate=True, **kw))
    try:
        _set_chunk(chunk)
        for call in calls:
            with pytest.raises(ValueError) as ei:
                call()
            msg = str(ei.value)
            for f in frags:
                assert f in msg, (name, msg)
            if partial is not None:
                assert [r[0] for r in reads_of(ei.value.partial)[::2]] == partial and reads_of(ei.value.partial) == as_reads(m.reads), name
            else:
                assert getattr(ei.value, "partial", None) is None
            msgs.append(msg)
    finally:
        _set_chunk(0)
    return msgs


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals(tmp_path, name):
    for chunk in (None, 257, 64):
        run_refusal(name, True, tmp_path, chunk, file_only=chunk is not None)


def test_counts_are_zero_after_a_call_that_did_not_collate(tmp_path):
    recs = cases()["grouped"]
    bam_to_reads(blob(recs), host=True, collate=True)
    assert reads_last_collate_counts()["pairs"] == 6
    bam_to_reads(blob(recs), host=True)
    assert not any(reads_last_collate_counts().values())
    read_reads_files(_file(tmp_path, "g", recs), host=True, collate=True)
    assert reads_last_collate_counts()["pairs"] == 6
    read_reads_files(_file(tmp_path, "g", recs), host=True)
    assert not any(reads_last_collate_counts().values())


def test_other_refusals(tmp_path):
    fq = str(tmp_path / "t.fq")
    with open(fq, "wb") as f:
        f.write(b"@a/1\nACGT\n+\nIIII\n@a/2\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError, match="collated by name .* in BAM input only"):
        read_reads_files(fq, host=True, collate=True)
    recs = cases()["A1 B1 A2 B2"]
    with pytest.raises(ValueError, match="collate_mem without collate"):
        bam_to_reads(blob(recs), host=True, collate_mem=1024)
    with pytest.raises(ValueError, match="collate_mem without collate"):
        read_reads_files(_file(tmp_path, "x", recs), host=True, collate_mem=1024)
    from bwamem_hip.aligner import Aligner
    for fn in (Aligner.align_files, Aligner.align_groups):                      # (refused before the aligner is looked at)
        with pytest.raises(ValueError, match="collate_mem without collate"):
            fn(None, "x.bam", out=object(), collate_mem=1 << 20)


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

@pytest.fixture(scope="module")
def core_exe():
    out = os.path.join(HERE, "_build")
    exe = os.path.join(out, "bam_collate_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_collate_host.cpp")] + [os.path.join(csrc, h) for h in ("bam_collate_core.h", "bam_in_core.h", "bam_dup_core.h", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        os.makedirs(out, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def _core(core_exe, tmp_path, recs, per, cap=8 << 30):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.txt")
    with open(src, "wb") as f:
        f.write(struct.pack("<QII", cap, per, len(recs)))
        for r in recs:
            e = encode(r)
            f.write(struct.pack("<I", len(e)) + e)
    subprocess.check_call([core_exe, src, dst])
    with open(dst) as f:
        return [ln.split() for ln in f.read().splitlines()]


def _core_expect(recs, m: Model):
    idx = {id(r): i for i, r in enumerate(recs)}
    want = [["pair", str(idx[id(a)]), str(idx[id(b)])] for a, b in zip(m.reads[::2], m.reads[1::2])]
    if m.refusal is not None:
        want.append([{"role": "same_role", "open": "open", "cap": "over_cap"}[m.refusal[0]]] + [str(v) for v in m.refusal[1:]])
    return want


def test_core_under_sanitizers(core_exe, tmp_path):
    todo = [(cases()["2000 pairs, random order"], 8 << 30), (cases()["slots free up and refill"], 8 << 30), (cases()["1000 first mates, then the second mates reversed"], 8 << 30)]
    todo += [(refusals()[n][0], refusals()[n][2].get("collate_mem", 8 << 30)) for n in REFUSALS if n != "a pair of two read groups"]
    for recs, cap in todo:
        m = model(recs, cap)
        for per in (1, 3, 64, 1 << 20):
            got = _core(core_exe, tmp_path, recs, per, cap)
            assert got[:-1] == _core_expect(recs, m), (per, cap)
            if m.refusal is None:
                assert got[-1] == ["counts", str(m.pairs), str(m.adjacent), str(m.peak_records), str(m.peak_bytes)], per
