"""A BAM realigned under its own read groups, on the device: the decoder kernels' group per read against the host form (test_keep_rg.py's cases and refusals, the
wave and workgroup edges, tables of 1 .. 257 groups), the device writer with a read group per read against the host formatter, and Aligner.align_files(keep_rg=True)
end to end -- the records of every read are those of a plain run of the same BAM under -R of the read's own @RG line, whatever the batch cuts, the lanes and the
form that decodes the input; a round trip through align_groups' BAM; sorted, marked output per library against the stand-alone host form; the refusals; the command."""
import io
import os
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

import common
import sam_table
from test_bam_dup import DUP, flag_of, name_of
from test_bam_dup_gpu import _dup_reads
from test_bam_gpu import PREFIX, _reads_files
from test_bam_input import bam_header, stored, tag
from test_bam_sort import BamFile, split_records
from test_keep_rg import IDS3, OTHER_TAGS, group_cases, host_text, mixed_tables, picked, refusals, rg
from test_read_groups import rg_of
from test_reads_input import bgzf

pytestmark = pytest.mark.gpu

LINES3 = ["@RG\tID:a\tLB:libX\tSM:s", "@RG\tID:ab\tSM:s\tLB:libX\tPU:unit.2", "@RG\tID:lane.3-of_three\tLB:libY\tSM:s"]
HD_IN = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:old\tLN:5\n@PG\tID:before\n"


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


# ---------------------------------------------------------------------------------------------------------------- the decoder kernels

def same_reads(a, b, what):
    for k in ("ascii", "codes", "offs", "lens", "name_blob", "name_off", "qual", "groups"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or (x.dtype == y.dtype and np.array_equal(x, y))), (what, k)
    assert (a.comments is None) == (b.comments is None), what
    if a.comments is not None:
        assert np.array_equal(a.comments[0], b.comments[0]) and np.array_equal(a.comments[1], b.comments[1]), (what, "comments")


def _edge_case(n_kept, paired, n_groups):
    """n_kept kept records (pairs: n_kept // 2 templates, their two records in either order) over a table of n_groups IDs, every group of the table's end used,
    skipped records interleaved so that kept and file indices differ, reverse-strand records among them; -> (records, ids, the group of every read)"""
    ids = ["g%d" % k for k in range(n_groups)]
    grp = lambda t: n_groups - 1 - (t * 7) % min(n_groups, 300) if t % 2 else (t * 5) % n_groups
    recs, want = [], []
    n_tpl = n_kept // 2 if paired else n_kept
    for t in range(n_tpl):
        g = n_groups - 1 if t == n_tpl - 1 else grp(t)
        L = 3 + t % 9
        seq = bytes(b"ACGT"[(t + i) & 3] for i in range(L))
        q = bytes(40 + (i + t) % 30 for i in range(L))
        before, after = OTHER_TAGS[t % len(OTHER_TAGS)], OTHER_TAGS[(t * 3 + 1) % len(OTHER_TAGS)] if t % 3 else b""
        if not paired:
            recs.append(stored(b"r%d" % t, seq, q, 4, before + rg(ids[g]) + after, rev=t % 4 == 1)); want.append(g)
        else:
            a = stored(b"p%d" % t, seq, q, 0x4d, before + rg(ids[g]), rev=t % 4 == 1)
            b = stored(b"p%d" % t, seq[::-1], q, 0x8d, rg(ids[g]) + after, rev=t % 4 == 2)
            recs += [b, a] if t % 5 == 3 else [a, b]
            want += [g, g]
        if t % 3 == 0:                                             # a skipped record without a tag, one with an unknown ID
            recs.append(stored(b"x%d" % t, b"ACG", b"III", (0x100 if t % 2 else 0x800) | (0x41 if paired else 0), b"" if t % 6 else rg("nowhere")))
    return b"".join(recs), ids, want


@pytest.mark.parametrize("n_groups", [1, 2, 257])
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n_kept", [63, 64, 65, 257])
def test_decoder_device_equals_host(hip, n_kept, paired, n_groups):
    from bwamem_hip.aligner import bam_to_reads
    if paired:
        n_kept += n_kept & 1                                       # (an even number of kept records: 64, 64, 66 and 258)
    records, ids, want = _edge_case(n_kept, paired, n_groups)
    host = bam_to_reads(records, comments=True, host=True, read_groups=ids)
    assert len(host) == n_kept and host.groups.tolist() == want and max(want) == n_groups - 1
    same_reads(bam_to_reads(records, comments=True, read_groups=ids), host, (n_kept, paired, n_groups))
    same_reads(bam_to_reads(records, read_groups=ids), bam_to_reads(records, host=True, read_groups=ids), (n_kept, paired, n_groups, "no comments"))


@pytest.mark.parametrize("n_groups", [255, 256])
def test_decoder_first_index_that_leaves_a_byte(hip, n_groups):
    from bwamem_hip.aligner import bam_to_reads
    records, ids, want = _edge_case(257, False, n_groups)
    dev = bam_to_reads(records, read_groups=ids)
    assert dev.groups.tolist() == want and max(want) == n_groups - 1
    same_reads(dev, bam_to_reads(records, host=True, read_groups=ids), n_groups)


@pytest.mark.parametrize("case", list(group_cases()))
def test_decoder_cases(hip, case):
    from bwamem_hip.aligner import bam_to_reads
    records, ids, want = group_cases()[case]
    dev = bam_to_reads(records, comments=True, read_groups=ids)
    assert dev.groups.tolist() == want
    same_reads(dev, bam_to_reads(records, comments=True, host=True, read_groups=ids), case)
    same_reads(bam_to_reads(records, comments=True), bam_to_reads(records, comments=True, host=True), (case, "without a table"))


@pytest.mark.parametrize("case", list(refusals()))
def test_decoder_refusals_are_the_hosts(hip, case):
    from bwamem_hip.aligner import bam_to_reads
    records, ids, piece, index = refusals()[case]
    with pytest.raises(ValueError) as eh:
        bam_to_reads(records, host=True, read_groups=ids)
    with pytest.raises(ValueError) as ed:
        bam_to_reads(records, read_groups=ids)
    assert str(ed.value) == str(eh.value).replace("bmh_bam_reads_groups_host", "bmh_bam_reads_groups_device") and piece in str(ed.value)
    assert f"record {index} " in str(ed.value) or f"records {index} and {index + 1} " in str(ed.value)


# ---------------------------------------------------------------------------------------------------------------- the writer

def device_text(T, po, tags, read_groups) -> bytes:
    import torch
    from bwamem_hip.lib import cigar_pack, sam_select_device, sam_text_device
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).cuda()
    fin, fpr = t(T.fin.reshape(-1, 16), np.int32), t(T.fpr, np.int32)
    h = t(T.h_rec, np.int32) if T.paired else None
    _sel, slot = sam_select_device(po, fin, fpr, h)
    aln = t(T.aln.reshape(-1, 8), np.int32)
    off, packed = cigar_pack(aln, t(T.cigar.view(np.int32), np.int32), t(T.md, np.uint8))
    return sam_text_device(po, T.names, t(T.ascii, np.uint8), t(T.offs, np.int32), t(T.lens, np.int32), T.contigs, fin, fpr, slot, aln, off, packed, h_rec_t=h,
                           unflag_t=t(T.unflag, np.int32) if T.paired else None, quals_t=t(T.quals, np.uint8) if tags else None, comments=T.comments if tags else None,
                           read_groups=read_groups)


def test_writer_device_equals_host(hip):
    for T, opts, tags, groups in mixed_tables():
        po = sam_table.post_opt(opts)
        want = host_text(T, po, tags, read_groups=(IDS3, groups))
        assert device_text(T, po, tags, (IDS3, groups)) == want == picked(T, opts, tags, groups)
        assert device_text(T, po, tags, None) == host_text(T, po, tags)                                  # without the arrays: as before, no tag
        with pytest.raises(RuntimeError, match="outside the table"):
            device_text(T, po, tags, (IDS3, groups[:-1] + [3]))
        with pytest.raises(RuntimeError, match="beside the options' one read group"):
            device_text(T, sam_table.post_opt(dict(opts, rg_id=b"x")), tags, (IDS3, groups))
    # a wave of 64 reads whose records exceed its LDS share, every read of another group than its neighbours: the counted and the written sizes agree per read
    ids = ["g", "a_longer_read_group_id" * 8, "mid-sized.id"]
    reads = [sam_table.read("n%02d_" % k + "x" * (150 + k % 9), "ACGT" * 30, [sam_table.rec(100, ("c2", 11 + 3 * k, k & 1, "120M", 0, "120"), mapq=60 - k % 7)]) for k in range(70)]
    T = sam_table.Table(reads)
    g = [(k * 2) % 3 for k in range(70)]
    got = device_text(T, sam_table.post_opt({}), True, (ids, g))
    assert got == host_text(T, sam_table.post_opt({}), True, read_groups=(ids, g)) and len(got) > 16384 + 3


# ---------------------------------------------------------------------------------------------------------------- end to end

def _fastx(path):
    """(name, sequence, qualities or None, comment) of every record of _reads_files' FASTA or interleaved FASTQ"""
    lines = open(path, "rb").read().split(b"\n")
    if lines[0].startswith(b">"):
        return [(lines[i][1:], lines[i + 1], None, b"") for i in range(0, len(lines) - 1, 2) if lines[i]]
    out = []
    for i in range(0, len(lines) - 1, 4):
        head = lines[i][1:].split(b" ")
        out.append((head[0].partition(b"/")[0], lines[i + 1], lines[i + 3], head[1] if len(head) > 1 else b""))
    return out


def _input_bam(tmp_path, name, reads, paired, group_of, header_lines, block=60000):
    """an unaligned BAM of the reads: template t's records carry RG:Z of group_of(t) (an ID), every fourth record stored reverse-complemented, a skipped record
    without a tag now and then; the header's text holds header_lines among other lines"""
    recs = []
    per = 2 if paired else 1
    for i, (nm, seq, q, c) in enumerate(reads):
        t = i // per
        fl = 4 if not paired else (0x4d if i % 2 == 0 else 0x8d)
        g = group_of(t)
        tags = (tag(b"BC", b"Z", c[5:]) if c else b"") + (rg(g) if g is not None else b"") + tag(b"XQ", b"i", i)
        recs.append(stored(nm, seq, q, fl, tags, rev=i % 4 == 3))
        if i % 50 == 7:
            recs.append(stored(nm, seq[:9], None if q is None else q[:9], 0x800 | (fl & 0xc1)))
    text = (HD_IN + "".join(l + "\n" for l in header_lines) + "@CO\tafter\n").encode()
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(bgzf(bam_header(text) + b"".join(recs), block))
    return path


def _by_name(text: bytes) -> dict:
    by = {}
    for l in text.split(b"\n"):
        if l and not l.startswith(b"@"):
            by.setdefault(l.split(b"\t")[0], []).append(l)
    return by


def _plain_run(rg_line, bam, **kw) -> bytes:
    from bwamem_hip.aligner import Aligner
    a = Aligner(PREFIX, n_threads=4)
    a.set_options(["-R", rg_line.replace("\t", "\\t")])
    buf = io.BytesIO()
    a.align_files(bam, out=buf, **kw)
    a.close()
    return buf.getvalue()


def _sq(al) -> str:
    return "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in al.contigs)


@pytest.mark.parametrize("paired", [False, True])
def test_sam_end_to_end(al, tmp_path, monkeypatch, paired):
    reads = _fastx(_reads_files(tmp_path, paired, n=300))
    group_of = lambda t: IDS3[t % 3]
    bam = _input_bam(tmp_path, "in.bam", reads, paired, group_of, LINES3)
    kw = dict(batch_reads=64)                                               # five batches, each of every group; every group in every batch
    buf = io.BytesIO()
    assert al.align_files(bam, out=buf, keep_rg=True, **kw) == 300 and al.last_stats.n_batches == 5
    text = buf.getvalue()
    header = (_sq(al) + "".join(l + "\n" for l in LINES3)).encode()
    assert text.startswith(header) and not text[len(header):].startswith(b"@")
    assert al.header() == _sq(al)                                           # the groups were the run's, not the aligner's
    # every read's records are those of the plain run of the same BAM under -R of its own line: three plain runs, picked per read
    plain = [_by_name(_plain_run(l, bam, **kw)) for l in LINES3]
    names = list(dict.fromkeys(r[0] for r in reads))
    want = b"".join(l + b"\n" for t, nm in enumerate(names) for l in plain[t % 3][nm])
    assert text[len(header):] == want and want.count(b"\n") >= 300 and all(want.count(b"\tRG:Z:" + i.encode() + b"\t") + want.count(b"\tRG:Z:" + i.encode() + b"\n") >= 100 for i in IDS3)
    # lanes, a pipe, the host's decoder, the host formatter: the same bytes
    for lanes in ("2", "4"):
        monkeypatch.setenv("BMH_ALIGNER_LANES", lanes)
        b2 = io.BytesIO(); al.align_files(bam, out=b2, keep_rg=True, **kw)
        assert b2.getvalue() == text and al.last_stats.n_lanes == int(lanes), lanes
    monkeypatch.delenv("BMH_ALIGNER_LANES")
    fifo = str(tmp_path / "in.fifo"); os.mkfifo(fifo)
    feeder = threading.Thread(target=lambda: open(fifo, "wb").write(open(bam, "rb").read())); feeder.start()
    b3 = io.BytesIO(); al.align_files(fifo, out=b3, keep_rg=True, **kw); feeder.join()
    assert b3.getvalue() == text
    from bwamem_hip.lib import reads_last_counts
    assert reads_last_counts()["host_windows"] == 0
    monkeypatch.setenv("BMH_READS_HOST", "1")
    b4 = io.BytesIO(); al.align_files(bam, out=b4, keep_rg=True, **kw)
    assert b4.getvalue() == text and reads_last_counts()["device_windows"] == 0
    monkeypatch.delenv("BMH_READS_HOST")
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")
    b5 = io.BytesIO(); al.align_files(bam, out=b5, keep_rg=True, **kw)
    assert b5.getvalue() == text
    monkeypatch.delenv("BMH_ALIGNER_HOST_FORMAT")
    # a BAM of one group: byte for byte the plain run under -R of its line
    one = _input_bam(tmp_path, "one.bam", reads, paired, lambda t: "ab", LINES3[1:2])
    b6 = io.BytesIO(); al.align_files(one, out=b6, keep_rg=True, **kw)
    assert b6.getvalue() == _plain_run(LINES3[1], one, **kw)
    # and without the option the aligner is what it was: no tag, no @RG line
    b7 = io.BytesIO(); al.align_files(bam, out=b7, **kw)
    assert b"RG:Z" not in b7.getvalue() and b"@RG" not in b7.getvalue()


def test_round_trip_of_a_run_over_groups(al, tmp_path):
    """the unsorted BAM of an align_groups run, given back with keep_rg: every read keeps the group it had, the header's @RG lines are the first run's"""
    da, db = tmp_path / "a", tmp_path / "b"; da.mkdir(); db.mkdir()
    src = _fastx(_reads_files(da, False, n=200))
    fa, fq = str(da / "a.fq"), str(db / "b.fq")                               # (both with qualities: a BAM's records all have them or none does)
    with open(fa, "wb") as f:
        for nm, seq, _q, _c in src:
            f.write(b"@%s\n%s\n+\n%s\n" % (nm, seq, b"A" * len(seq)))
    with open(fq, "wb") as f:
        for i, (_n, seq, _q, _c) in enumerate(src[:150]):
            f.write(b"@s%d\n%s\n+\n%s\n" % (i, seq[::-1], b"F" * len(seq)))
    lines = ["@RG\\tID:one\\tLB:l1", "@RG\\tID:two\\tLB:l2\\tSM:x"]
    first = io.BytesIO()
    al.align_groups([(lines[0], fa, None), (lines[1], fq, None)], out=first, fmt="bam", batch_reads=64)
    f1 = BamFile(first.getvalue())
    had = {name_of(r): rg_of(r) for r in f1.recs}
    assert set(had.values()) == {"one", "two"} and len(had) == 350
    path = str(tmp_path / "first.bam")
    with open(path, "wb") as f:
        f.write(first.getvalue())
    second = io.BytesIO()
    assert al.align_files(path, out=second, fmt="bam", keep_rg=True, batch_reads=64) == 350
    f2 = BamFile(second.getvalue())
    assert {name_of(r): rg_of(r) for r in f2.recs} == had
    rg_lines = lambda f: [l for l in f.header_text.split(b"\n") if l.startswith(b"@RG")]
    assert rg_lines(f2) == rg_lines(f1) == [l.replace("\\t", "\t").encode() for l in lines]


# ---------------------------------------------------------------------------------------------------------------- sorted, marked

LIB_OF = {"a": "libX", "ab": "libX", "lane.3-of_three": "libY"}


def _dup_input(tmp_path, paired):
    """_dup_reads' templates as a BAM in three groups of two libraries: an original t is of group a (every fifth: it has copies) or t % 3; its first copy is of
    group ab (library X, as a) or of the third group (library Y), alternating, its second copy of the other -- identical templates within and across libraries"""
    path, names = _dup_reads(tmp_path, paired)
    reads = _fastx(path)
    n_orig = sum(1 for n in names if b"c" not in n)

    def group_of(t):
        nm = names[t]
        if b"c" not in nm:
            return "a" if t % 5 == 0 else IDS3[t % 3]
        base, copy = int(nm[1:nm.index(b"c")]), int(nm[-1:])
        return ("ab", "lane.3-of_three")[((base // 5) + copy) & 1]
    assert n_orig in (300, 600)
    return _input_bam(tmp_path, "dups.bam", reads, paired, group_of, LINES3), names, group_of


@pytest.mark.parametrize("paired", [False, True])
def test_sorted_markdup_per_library(al, tmp_path, monkeypatch, paired):
    from bwamem_hip.lib import bam_sorted_file
    bam, names, group_of = _dup_input(tmp_path, paired)
    monkeypatch.setenv("BMH_ALIGNER_LANES", "1")
    unsorted = io.BytesIO()
    al.align_files(bam, out=unsorted, fmt="bam", keep_rg=True, batch_reads=256)
    fu = BamFile(unsorted.getvalue())
    assert {name_of(r): rg_of(r) for r in fu.recs} == {nm: group_of(t) for t, nm in enumerate(names)}
    hdr = "@HD\tVN:1.6\tSO:coordinate\n" + _sq(al) + "".join(l + "\n" for l in LINES3)
    table = [(i, LIB_OF[i]) for i in IDS3]
    want = bam_sorted_file(hdr, al.contigs, fu.stream, 1, 100, host=True, markdup=True, read_groups=table)

    def run(**kw):
        out, idx, met = io.BytesIO(), io.BytesIO(), io.StringIO()
        al.align_files(bam, out=out, fmt="bam", sort=True, index=idx, markdup=True, markdup_metrics=met, keep_rg=True, sort_window=100, **kw)
        return out.getvalue(), idx.getvalue(), met.getvalue()
    got = run(batch_reads=256)
    assert al.last_stats.n_batches >= 3
    assert (got[0], got[1]) == (want[0], want[1])
    assert al.markdup_library_counts == want[2]["libraries"] and list(al.markdup_library_counts) == ["libX", "libY"]
    assert al.markdup_counts == {k: v for k, v in want[2].items() if k != "libraries"}
    rows = got[2].split("\n")
    assert len(rows) == 5 and [r.split("\t")[0] for r in rows[2:4]] == ["libX", "libY"]
    # the same bytes whatever the batches, the lanes, the window and a spilling run store (pairs under other cuts: the insert-size statistics are a batch's, so
    # there only the runs that keep the cuts are compared byte for byte, as the tests of runs over groups do)
    spill = tmp_path / "spill"; spill.mkdir()
    for lanes, knobs in (("3", dict(batch_reads=256)), ("1", dict(batch_reads=256, sort_mem=1, sort_tmp=str(spill))), ("2", dict(batch_reads=100))):
        if paired and knobs["batch_reads"] != 256:
            continue
        monkeypatch.setenv("BMH_ALIGNER_LANES", lanes)
        assert run(**knobs) == got, (lanes, knobs)
    assert os.listdir(spill) == []
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")
    out1 = io.BytesIO()
    al.align_files(bam, out=out1, fmt="bam", sort=True, markdup=True, keep_rg=True, sort_window=1, batch_reads=256)
    assert BamFile(out1.getvalue()).stream == BamFile(got[0]).stream
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")                      # the host forms of the batch's entries and per-library counts
    assert run(batch_reads=256) == got
    monkeypatch.delenv("BMH_ALIGNER_HOST_FORMAT")
    # the model of test_read_groups.py applied per library to the unsorted run's records: the same flags, the same counts
    from test_bam_sort import py_sort
    from test_read_groups import library_model
    f = BamFile(got[0])
    model_stream, total, per, _h = library_model(fu.stream, table)
    assert f.stream == py_sort(model_stream) and al.markdup_library_counts == per and al.markdup_counts == total
    # a duplicate pair split across two libraries is not flagged; the same pair within one library is.  Every fifth template t has two copies: t is of group a
    # (library X), one copy of group ab (library X), the other of the third group (library Y).  (Not every triple qualifies: a read that maps to several places is
    # placed by a hash of its index, so identical reads may part.)  With all three groups in one library the third copy is flagged too.
    triples = _triples(names, group_of, f)
    good = [t for t in triples if len({t[0], t[1]} & t[3]) == 1 and t[2] not in t[3]]
    assert len(good) >= 20 and len(good) >= 0.8 * len(triples)
    one_lib = [l.replace("LB:libY", "LB:libX") for l in LINES3]
    bam1 = _input_bam(tmp_path, "one_library.bam", _fastx(str(tmp_path / "dups.fq")), paired, group_of, one_lib)
    out2 = io.BytesIO()
    al.align_files(bam1, out=out2, fmt="bam", sort=True, markdup=True, keep_rg=True, batch_reads=256)
    assert list(al.markdup_library_counts) == ["libX"]
    both = {t[0] for t in _triples(names, group_of, BamFile(out2.getvalue())) if len({t[0], t[1], t[2]} & t[3]) == 2}
    assert len(both & {t[0] for t in good}) >= 20


def _triples(names, group_of, f):
    """(original, its copy in library X, its copy in library Y, the flagged names) of every copied template whose three copies are all mapped"""
    flagged = {name_of(r) for r in f.recs if flag_of(r) & DUP}
    mapped = {name_of(r) for r in f.recs if not flag_of(r) & 0x904}
    idx_of = {nm: t for t, nm in enumerate(names)}
    out = []
    for nm in names:
        if b"c" in nm or nm + b"c1" not in idx_of:
            continue
        x_copy, y_copy = (nm + b"c1", nm + b"c2") if group_of(idx_of[nm + b"c1"]) == "ab" else (nm + b"c2", nm + b"c1")
        if {nm, x_copy, y_copy} <= mapped:
            out.append((nm, x_copy, y_copy, flagged))
    return out


# ---------------------------------------------------------------------------------------------------------------- refusals, the command

def test_refusals(al, tmp_path):
    reads = _fastx(_reads_files(tmp_path, False, n=300))
    bam = _input_bam(tmp_path, "in.bam", reads, False, lambda t: IDS3[t % 3], LINES3)
    fa = str(tmp_path / "r.fa")
    for kw, path, mates, msg in ((dict(), fa, None, "only when it is a BAM file"), (dict(fmt="bam", sort=True, markdup=True), fa, None, "only when it is a BAM file"),
                                 (dict(), bam, fa, "mates file")):
        out = io.BytesIO()
        with pytest.raises(ValueError, match=msg):
            al.align_files(path, mates, out=out, keep_rg=True, **kw)
        assert out.getvalue() == b""
    no_rg = _input_bam(tmp_path, "no_rg.bam", reads, False, lambda t: "a", [])
    twice = _input_bam(tmp_path, "twice.bam", reads, False, lambda t: "a", [LINES3[0], LINES3[2], "@RG\tID:a\tLB:other"])
    for path, msg in ((no_rg, "no @RG line"), (twice, r"@RG line 3 .*earlier @RG line")):
        for kw in (dict(), dict(fmt="bam")):
            out = io.BytesIO()
            with pytest.raises(ValueError, match=msg):
                al.align_files(path, out=out, keep_rg=True, **kw)
            assert out.getvalue() == b""
    al.set_options(["-R", "@RG\\tID:z"])
    try:
        out = io.BytesIO()
        with pytest.raises(ValueError, match="-R is set"):
            al.align_files(bam, out=out, keep_rg=True)
        assert out.getvalue() == b""
        nat = al._native_aligner()                                           # the library refuses it too
        nat.set_keep_rg(True)
        try:
            with pytest.raises(ValueError, match="read group of its own"):
                nat.run_files(bam, None, False, lambda mv: None, batch_reads=64)
        finally:
            nat.set_keep_rg(False)
    finally:
        al.rg_line = ""; al.po.rg_id = None
    nat = al._native_aligner()
    nat.set_keep_rg(True)
    try:
        with pytest.raises(ValueError, match="do not combine"):
            nat.run_groups([("a", 0, bam, None)], False, lambda mv: None, batch_reads=64)
    finally:
        nat.set_keep_rg(False)
    # a record without its tag halfway through the file: the run fails naming its index, after the batches before it were written
    bad_at = 150
    damaged = _input_bam(tmp_path, "damaged.bam", reads, False, lambda t: IDS3[t % 3] if t != bad_at else None, LINES3)
    n_before = bad_at + sum(1 for i in range(bad_at) if i % 50 == 7)          # (the skipped records count in the file's index)
    out = io.BytesIO()
    with pytest.raises(ValueError, match=r"BAM record %d \(r150\): no RG tag" % n_before):
        al.align_files(damaged, out=out, keep_rg=True, batch_reads=64)
    body = _by_name(out.getvalue())
    assert out.getvalue().startswith((_sq(al) + "".join(l + "\n" for l in LINES3)).encode()) and list(body) == [b"r%d" % k for k in range(128)]      # two whole batches
    unknown = _input_bam(tmp_path, "unknown.bam", reads, False, lambda t: IDS3[t % 3] if t != 5 else "abc", LINES3)
    with pytest.raises(ValueError, match=r"BAM record 5 \(r5\): its RG:Z names a read group the header"):
        al.align_files(unknown, out=io.BytesIO(), keep_rg=True, batch_reads=64)
    out = io.BytesIO()                                                       # the aligner still runs, with and without the option
    assert al.align_files(bam, out=out, keep_rg=True, batch_reads=64) == 300 and al.align_files(bam, out=io.BytesIO(), batch_reads=64) == 300


def test_mem_command_keep_rg(al, tmp_path):
    reads = _fastx(_reads_files(tmp_path, True, n=300))
    bam = _input_bam(tmp_path, "x.bam", reads, True, lambda t: IDS3[t % 3], LINES3)
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(common.GOLDEN), "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    sam = str(tmp_path / "out.sam")
    r = subprocess.run([sys.executable, "-m", "bwamem_hip.mem", "--keep-rg", PREFIX, bam, "-o", sam], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    out = io.BytesIO()
    al.align_files(bam, out=out, keep_rg=True)
    assert open(sam, "rb").read() == out.getvalue() and out.getvalue().count(b"\tRG:Z:") >= 300
    for extra, msg in ((["--rg", LINES3[0].replace("\t", "\\t")], "--keep-rg excludes --rg and -R"), (["-R", LINES3[0].replace("\t", "\\t")], "--keep-rg excludes --rg and -R")):
        r = subprocess.run([sys.executable, "-m", "bwamem_hip.mem", "--keep-rg", PREFIX] + (extra + [bam] if extra[0] == "--rg" else extra + [bam]) + ["-o", str(tmp_path / "no.sam")],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and msg in r.stderr.decode() and not os.path.exists(str(tmp_path / "no.sam"))
