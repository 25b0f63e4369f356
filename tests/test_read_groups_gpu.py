"""Runs over several read groups on the device: the library rule of the duplicate-marking kernels against the host forms on test_read_groups.py's corpus, and
Aligner.align_groups end to end -- the SAM of a run over groups is the groups' lone runs one after the other, whatever the lanes; sorted, marked output calls
duplicates per library and does not depend on batch cuts, lanes, the window or a spilled run store; a BAM as a group's input; the refusals; the command."""
import gzip
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import common
from test_bam_core import encode_text
from test_bam_dup import DUP, flag_of, mask_dup, name_of, templates_of
from test_bam_dup_gpu import _dup_reads
from test_bam_gpu import PREFIX, _reads_files
from test_bam_sort import CONTIGS, BamFile, check_file, split_records
from test_read_groups import COUNT_KEYS, HDR, corpus, expected, library_model, rg_of

HD = "@HD\tVN:1.6\tSO:coordinate\n"
RG_A, RG_B = "@RG\\tID:a\\tLB:libX\\tSM:s", "@RG\\tID:b\\tLB:libX\\tSM:s"
RG_B_OTHER = "@RG\\tID:b\\tLB:libY\\tSM:s"


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.fixture(scope="module")
def al(hip):
    from bwamem_hip.aligner import Aligner
    a = Aligner(PREFIX, n_threads=4)
    yield a
    a.close()


# ---------------------------------------------------------------------------------------------------------------- the kernels

@pytest.mark.gpu
def test_device_equals_host(hip):
    """63 / 64 / 65 templates (wave edge), 257 (workgroup edge), 1000, and the 300 pairs at one key, whose runs of equal lanes cross a workgroup boundary inside
    each library"""
    from bwamem_hip.lib import bam_markdup
    for what, groups, stream, _must in corpus():
        want, total, per, _h = expected(what, groups, stream)
        got, c = bam_markdup(stream, read_groups=groups)
        assert (got, c) == bam_markdup(stream, host=True, read_groups=groups), what
        assert got == want and c["libraries"] == per and {k: c[k] for k in COUNT_KEYS} == total, what
    # the refusals name the same record on the device as on the host
    what, groups, stream, _must = corpus()[4]
    recs = split_records(stream)
    first = templates_of(recs)[40][0]                                       # (the template's first record: the one whose tag is read)
    no_tag = b"".join(recs[:first]) + _untagged(recs[first]) + b"".join(recs[first + 1:])
    for bad, g, msg in ((stream, [x for x in groups if x[0] != "lane1"], "record 0 .*not among those given"), (no_tag, groups, "record %d .*no RG:Z tag" % first)):
        for host in (True, False):
            with pytest.raises(ValueError, match=msg):
                bam_markdup(bad, host=host, read_groups=g)


def _untagged(r: bytes) -> bytes:
    """the record without its trailing RG:Z tag (the one test_read_groups.tag appended)"""
    import struct
    cut = r[:r.rindex(b"RGZ")]
    return struct.pack("<I", len(cut) - 4) + cut[4:]


@pytest.mark.gpu
@pytest.mark.parametrize("window", [0, 1, 7, 100])
def test_sorted_file_device_equals_host(hip, window):
    from bwamem_hip.lib import bam_sorted_file
    for what, groups, stream, _must in corpus():
        dev = bam_sorted_file(HDR, CONTIGS, stream, 1, window, markdup=True, read_groups=groups)
        assert dev == bam_sorted_file(HDR, CONTIGS, stream, 1, window, host=True, markdup=True, read_groups=groups), (what, window)
        assert dev[2]["libraries"] == expected(what, groups, stream)[2], what


# ---------------------------------------------------------------------------------------------------------------- inputs

def _fasta_records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 2) if lines[i]]


def _group_inputs(tmp_path, paired):
    """group A and group B of the concatenation test -> ((reads, mates) of A, (reads, mates) of B)"""
    da = tmp_path / "ga"; da.mkdir()
    src = _reads_files(da, paired)
    if not paired:
        # B: the same reads under other names with another seed's substitutions, gzip-compressed
        rng = np.random.default_rng(11)
        out = []
        for i, (_n, seq) in enumerate(_fasta_records(src)):
            s = bytearray(seq)
            for k in np.flatnonzero(rng.random(len(s)) < 0.02):
                s[int(k)] = b"ACGT"[(b"ACGT".index(s[int(k)]) + int(rng.integers(1, 4))) % 4] if s[int(k)] in b"ACGT" else s[int(k)]
            out.append(b">s%d\n%s\n" % (i, bytes(s)))
        b = str(tmp_path / "b.fa.gz")
        with gzip.open(b, "wb") as f:
            f.write(b"".join(out))
        return (src, None), (b, None)
    # A: the interleaved FASTQ as R1 + R2 files; B: the same pairs interleaved, under other names
    recs = open(src, "rb").read().split(b"\n")
    four = [recs[i:i + 4] for i in range(0, len(recs) - 1, 4)]
    r1, r2, b = str(tmp_path / "a_1.fq"), str(tmp_path / "a_2.fq"), str(tmp_path / "b.fq")
    with open(r1, "wb") as f1, open(r2, "wb") as f2, open(b, "wb") as fb:
        for i, q in enumerate(four):
            (f2 if i & 1 else f1).write(b"\n".join(q) + b"\n")
            fb.write(b"\n".join([b"@q" + q[0][2:]] + q[1:]) + b"\n")
    return (r1, r2), (b, None)


def _body(text: bytes) -> bytes:
    return b"".join(l + b"\n" for l in text.split(b"\n") if l and not l.startswith(b"@"))


def _lone(rg, reads, mates, **kw):
    """(SAM body, batches) of align_files on one group's input alone under -R rg"""
    from bwamem_hip.aligner import Aligner
    a = Aligner(PREFIX, n_threads=4)
    a.set_options(["-R", rg])
    buf = io.BytesIO()
    a.align_files(reads, mates, out=buf, **kw)
    n = a.last_stats.n_batches
    assert buf.getvalue().startswith(a.header().encode())
    a.close()
    return _body(buf.getvalue()), n


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_sam_is_the_concatenation(al, tmp_path, monkeypatch, paired):
    ga, gb = _group_inputs(tmp_path, paired)
    kw = dict(batch_reads=256, paired=paired)                               # three batches per group, the last one short
    body_a, na = _lone(RG_A, *ga, **kw)
    body_b, nb = _lone(RG_B_OTHER, *gb, **kw)
    assert na == 3 and nb == 3 and body_a.count(b"\tRG:Z:a") == body_a.count(b"\n") >= 600 and body_b.count(b"\tRG:Z:b") == body_b.count(b"\n") >= 600
    groups = [(RG_A, *ga), (RG_B_OTHER, *gb)]
    for lanes in ("1", "3"):
        monkeypatch.setenv("BMH_ALIGNER_LANES", lanes)
        buf = io.BytesIO()
        assert al.align_groups(groups, out=buf, **kw) == 1200
        text = buf.getvalue()
        assert text.startswith(("".join("@SQ\tSN:%s\tLN:%d\n" % c for c in al.contigs) + "@RG\tID:a\tLB:libX\tSM:s\n@RG\tID:b\tLB:libY\tSM:s\n").encode())
        assert _body(text) == body_a + body_b, lanes
        assert al.last_stats.n_batches == na + nb and al.last_stats.n_lanes == int(lanes)
    assert al.header() == "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in al.contigs)      # the groups are the run's, not the aligner's
    # unsorted BAM: the records of that same text
    want, st = encode_text(body_a + body_b, al.contigs)
    assert not st.any()
    buf = io.BytesIO()
    al.align_groups(groups, out=buf, fmt="bam", **kw)
    f = BamFile(buf.getvalue())
    assert f.stream == want and f.header_text == text[:len(text) - len(_body(text))] and len(f.text) >= 1 + 6 + 1      # header, a member per batch at least, end of file
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")                      # the host formatter takes the batch's read group too
    buf = io.BytesIO()
    al.align_groups(groups, out=buf, **kw)
    assert _body(buf.getvalue()) == body_a + body_b


# ---------------------------------------------------------------------------------------------------------------- sorted, marked

def _sorted_run(al, groups, **kw):
    out, idx = io.BytesIO(), io.BytesIO()
    kw.setdefault("markdup", True)
    al.align_groups(groups, out=out, fmt="bam", sort=True, index=idx, **kw)
    return out.getvalue(), idx.getvalue()


def _writer_order(stream: bytes, ids, names) -> bytes:
    """the records of a sorted file back in the writer's order: group after group, inside a group by read name in input order, read 1 before read 2, the primary
    line first"""
    by = {}
    for i, r in enumerate(split_records(stream)):
        by.setdefault((rg_of(r), name_of(r)), []).append((bool(flag_of(r) & 0x80), bool(flag_of(r) & 0x900), i, r))
    assert set(by) == {(g, n) for g in ids for n in names}
    return b"".join(r for g in ids for n in names for _a, _b, _i, r in sorted(by[(g, n)]))


def _flagged(stream: bytes, rid=None) -> set:
    return {(name_of(r), flag_of(r)) for r in split_records(stream) if flag_of(r) & DUP and (rid is None or rg_of(r) == rid)}


def _mapped_templates(stream: bytes, rid) -> set:
    return {name_of(r) for r in split_records(stream) if rg_of(r) == rid and not flag_of(r) & 0x904}


def _lone_sorted(rg, path, paired):
    from bwamem_hip.aligner import Aligner
    a = Aligner(PREFIX, n_threads=4)
    a.set_options(["-R", rg])
    out = io.BytesIO()
    a.align_files(path, out=out, paired=paired, batch_reads=256, fmt="bam", sort=True, markdup=True)
    c = dict(a.markdup_counts)
    a.close()
    return BamFile(out.getvalue()).stream, c


def _invariance(al, groups, ids, names, base, monkeypatch, tmp_path, paired):
    """the file and its index (windows of 100 records; base: one lane, batches of 256 reads) across batch cuts, lanes and a spilling run store: the same bytes.
    Pairs under other cuts are the exception the aligner has always had -- the insert-size statistics are a batch's, so a pair's records (flags, MAPQ, a rescued
    mate) may change with the cuts before any duplicate is looked for; there the flagged templates are compared, as test_bam_dup_gpu.py does"""
    bam, bai = base
    spill = tmp_path / "spill"; spill.mkdir()
    want = _writer_order(BamFile(bam).stream, ids, names)
    flagged = {(rg_of(r), name_of(r)) for r in split_records(want) if flag_of(r) & DUP}
    hdr = HD + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in al.contigs) + "".join(g[0].replace("\\t", "\t") + "\n" for g in groups)
    check_file(bam, bai, hdr, al.contigs, want, "base", n_regions=10)
    for lanes, knobs in (("3", dict(batch_reads=256)), ("1", dict(batch_reads=0)), ("3", dict(batch_reads=0)), ("1", dict(batch_reads=256, sort_mem=1, sort_tmp=str(spill)))):
        monkeypatch.setenv("BMH_ALIGNER_LANES", lanes)
        b2, i2 = _sorted_run(al, groups, paired=paired, sort_window=100, **knobs)
        if paired and knobs["batch_reads"] != 256:
            f2 = BamFile(b2)
            assert {(rg_of(r), name_of(r)) for r in f2.recs if flag_of(r) & DUP} == flagged, (lanes, knobs)
            check_file(b2, i2, hdr, al.contigs, _writer_order(f2.stream, ids, names), knobs, n_regions=10)
            continue
        assert (b2, i2) == (bam, bai), (lanes, knobs)
        check_file(b2, i2, hdr, al.contigs, want, knobs, n_regions=10)
    assert os.listdir(spill) == []


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_one_file_as_two_lanes_of_one_library(al, tmp_path, monkeypatch, paired):
    """the same file as groups a and b of one library: b's copy of every mapped template is a duplicate (equal scores: the earlier ordinal stays); with higher
    qualities in b's file the roles swap"""
    path, names = _dup_reads(tmp_path, paired)
    groups = [(RG_A, path, None), (RG_B, path, None)]
    monkeypatch.setenv("BMH_ALIGNER_LANES", "1")
    base = _sorted_run(al, groups, paired=paired, batch_reads=256, sort_window=100)
    assert al.last_stats.n_batches >= 6
    f = BamFile(base[0])
    lone_a, _counts_a = _lone_sorted(RG_A, path, paired)
    assert {rg_of(r) for r in f.recs} == {"a", "b"} and sum(rg_of(r) == "a" for r in f.recs) == sum(rg_of(r) == "b" for r in f.recs) == len(split_records(lone_a))
    mapped = _mapped_templates(f.stream, "b")
    assert len(mapped) >= 200 and {n for n, _fl in _flagged(f.stream, "b")} == mapped                       # every mapped template of b, and no other
    assert all(flag_of(r) & DUP for r in f.recs if rg_of(r) == "b" and name_of(r) in mapped)               # ... on every record
    assert _flagged(f.stream, "a") == _flagged(lone_a) and len(_flagged(lone_a)) >= 10                     # a: as alone
    # the whole file against the model applied per library
    plain = BamFile(_sorted_run(al, groups, paired=paired, batch_reads=256, markdup=False)[0])
    assert mask_dup(f.stream) == plain.stream and not _flagged(plain.stream)
    table = [("a", "libX"), ("b", "libX")]
    want, total, per, _h = library_model(_writer_order(plain.stream, "ab", names), table)
    assert _writer_order(f.stream, "ab", names) == want and al.markdup_counts == total and al.markdup_library_counts == per
    _invariance(al, groups, "ab", names, base, monkeypatch, tmp_path, paired)
    # higher qualities in b's file: now a's copies are the duplicates, and b is flagged as b alone
    lines = open(path, "rb").read().split(b"\n")
    for i in range(3, len(lines), 4):
        lines[i] = bytes(min(q + 1, 74) for q in lines[i])
    better = str(tmp_path / "better.fq")
    with open(better, "wb") as fh:
        fh.write(b"\n".join(lines))
    g = BamFile(_sorted_run(al, [(RG_A, path, None), (RG_B, better, None)], paired=paired, batch_reads=256)[0])
    lone_b, _c = _lone_sorted(RG_B, better, paired)
    assert {n for n, _fl in _flagged(g.stream, "a")} == _mapped_templates(g.stream, "a") and _flagged(g.stream, "b") == _flagged(lone_b)


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_one_file_as_two_libraries(al, tmp_path, monkeypatch, paired):
    path, names = _dup_reads(tmp_path, paired)
    groups = [(RG_A, path, None), (RG_B_OTHER, path, None)]
    monkeypatch.setenv("BMH_ALIGNER_LANES", "1")
    met = io.StringIO()
    base = _sorted_run(al, groups, paired=paired, batch_reads=256, sort_window=100, markdup_metrics=met)
    f = BamFile(base[0])
    lone_a, counts_a = _lone_sorted(RG_A, path, paired)
    lone_b, counts_b = _lone_sorted(RG_B_OTHER, path, paired)
    assert _flagged(f.stream, "a") == _flagged(lone_a) and _flagged(f.stream, "b") == _flagged(lone_b) and len(_flagged(lone_a)) >= 10
    assert _flagged(f.stream) == _flagged(lone_a) | _flagged(lone_b)
    assert sorted(r for r in f.recs if rg_of(r) == "a") == sorted(split_records(lone_a)) and sorted(r for r in f.recs if rg_of(r) == "b") == sorted(split_records(lone_b))
    assert al.markdup_library_counts == {"libX": counts_a, "libY": counts_b}
    assert al.markdup_counts == {k: counts_a[k] + counts_b[k] for k in COUNT_KEYS}
    rows = met.getvalue().split("\n")
    assert len(rows) == 5 and [r.split("\t")[0] for r in rows[2:4]] == ["libX", "libY"]
    assert [int(v) for v in rows[2].split("\t")[5:7]] == [counts_a["duplicate_fragments"], counts_a["duplicate_pairs"]] and counts_a["duplicate_pairs" if paired else "duplicate_fragments"] >= 1
    _invariance(al, groups, "ab", names, base, monkeypatch, tmp_path, paired)


# ---------------------------------------------------------------------------------------------------------------- a BAM as a group's input, refusals, the command

def _single_end_fastq(tmp_path):
    """group B of the BAM test: test_bam_gpu's single-end reads as FASTQ under other names"""
    d = tmp_path / "gb"; d.mkdir()
    rng = np.random.default_rng(2)
    b = str(tmp_path / "b.fq")
    with open(b, "wb") as f:
        for i, (_n, seq) in enumerate(_fasta_records(_reads_files(d, False))):
            f.write(b"@s%d\n%s\n+\n%s\n" % (i, seq, bytes((rng.integers(2, 41, len(seq)) + 33).astype(np.uint8))))
    return b


@pytest.mark.gpu
def test_bam_input_as_a_group(al, tmp_path, monkeypatch):
    from bwamem_hip.aligner import Aligner
    da = tmp_path / "ga"; da.mkdir()
    a_fa, b_fq = _reads_files(da, False), _single_end_fastq(tmp_path)
    other = Aligner(PREFIX, n_threads=4)
    other.set_options(["-R", "@RG\\tID:elsewhere"])                         # the BAM's own @RG line and RG tags stay ignored
    a_bam = str(tmp_path / "a.bam")
    with open(a_bam, "wb") as f:
        other.align_files(a_fa, out=f, fmt="bam")
    other.close()
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")
    text, from_bam = io.BytesIO(), io.BytesIO()
    al.align_groups([(RG_A, a_fa, None), (RG_B, b_fq, None)], out=text, batch_reads=256)
    al.align_groups([(RG_A, a_bam, None), (RG_B, b_fq, None)], out=from_bam, batch_reads=256)
    assert from_bam.getvalue() == text.getvalue() and text.getvalue().count(b"\tRG:Z:a") >= 600 and b"elsewhere" not in from_bam.getvalue()


@pytest.mark.gpu
def test_run_time_refusals(al, tmp_path):
    from bwamem_hip.aligner import Aligner
    (r1, r2), (b_fq, _n) = _group_inputs(tmp_path, True)
    da = tmp_path / "se"; da.mkdir()
    se_fa = _reads_files(da, False)
    out = io.BytesIO()
    with pytest.raises(ValueError, match=r"read group 'b'.*missing\.fq"):
        al.align_groups([(RG_A, r1, r2), (RG_B, str(tmp_path / "missing.fq"), None)], out=out)
    assert out.getvalue() == b""                                             # nothing written
    with pytest.raises(ValueError, match=r"read group 'b'.*single-end reads"):
        al.align_groups([(RG_A, r1, r2), (RG_B, se_fa, None)], out=io.BytesIO())
    se_bam = str(tmp_path / "se.bam")
    other = Aligner(PREFIX, n_threads=4)
    with open(se_bam, "wb") as f:
        other.align_files(se_fa, out=f, fmt="bam")
    other.close()
    with pytest.raises(ValueError, match=r"read group 'b'.*flag 0x1"):
        al.align_groups([(RG_A, r1, r2), (RG_B, se_bam, None)], out=io.BytesIO(), paired=True)
    with pytest.raises(ValueError, match=r"read group 'b'.*single-end reads"):
        al.align_groups([(RG_A, r1, r2), (RG_B, se_bam, None)], out=io.BytesIO())
    al.set_options(["-R", "@RG\\tID:z"])
    try:
        with pytest.raises(ValueError, match="-R is set"):
            al.align_groups([(RG_A, r1, r2)], out=io.BytesIO())
        nat = al._native_aligner()                                           # the library refuses it too
        with pytest.raises(ValueError, match="read group of its own"):
            nat.run_groups([("a", 0, r1, r2)], True, lambda mv: None, batch_reads=256)
    finally:
        al.rg_line = ""; al.po.rg_id = None
    nat = al._native_aligner()
    for bad, msg in (([], "no read groups"), ([("a", 0, r1, r2), ("a", 0, b_fq, None)], "share the ID"), ([("a", 255, r1, r2)], "at most 255 libraries")):
        with pytest.raises(ValueError, match=msg):
            nat.run_groups(bad, True, lambda mv: None, batch_reads=256)
    out = io.BytesIO()                                                       # the aligner still runs
    assert al.align_groups([(RG_A, r1, r2), (RG_B, b_fq, None)], out=out, paired=True, batch_reads=256) == 1200


@pytest.mark.gpu
def test_mem_command_read_groups(al, tmp_path):
    (a_fa, _n), (b_gz, _m) = _group_inputs(tmp_path, False)
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(common.GOLDEN), "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    bam, met = str(tmp_path / "x.bam"), str(tmp_path / "m.txt")
    r = subprocess.run([sys.executable, "-m", "bwamem_hip.mem", PREFIX, "--sort", "--markdup", "--markdup-metrics", met, "-o", bam, "--rg", RG_A, a_fa, "--rg", RG_B_OTHER, b_gz],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    out, idx, m2 = io.BytesIO(), io.BytesIO(), io.StringIO()
    al.align_groups([(RG_A, a_fa, None), (RG_B_OTHER, b_gz, None)], out=out, fmt="bam", sort=True, index=idx, markdup=True, markdup_metrics=m2)
    with open(bam, "rb") as f, open(bam + ".bai", "rb") as g:
        assert f.read() == out.getvalue() and g.read() == idx.getvalue()
    rows = open(met).read().split("\n")
    assert open(met).read() == m2.getvalue() and len(rows) == 5 and [r.split("\t")[0] for r in rows[2:4]] == ["libX", "libY"]
