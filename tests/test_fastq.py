"""FASTQ input: the loader (bmh_reads_load), its refusals, -C, and -- on the GPU -- QUAL and comments in the SAM text of every path,
byte for byte against the reference's own host code (oracle/_ref/dropin/bwa-gasal2) and against the same reads in FASTA."""
import io
import os
import subprocess

import numpy as np
import pytest

from bwamem_hip.aligner import _NT4, ReadSet, read_fasta_reads, read_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "oracle", "_ref", "dropin", "bwa-gasal2")


# ---------------------------------------------------------------------------------------------------------------- the file and its parse

def _records(rng, n, lo=1, hi=300):
    """n reads: (name, comment, seq, qual) with names "r<i>", "r<i>/1" / "/2", comments with spaces and tabs, qualities that begin with '@' / '+'"""
    alphabet = np.frombuffer(b"ACGTNacgtnRY", dtype=np.uint8)
    out = []
    for i in range(n):
        ln = int(rng.integers(lo, hi))
        s = rng.choice(alphabet, size=ln).tobytes()
        q = bytearray(rng.integers(33, 75, size=ln).astype(np.uint8).tobytes())
        if i % 3 == 0:
            q[0] = ord("@")
        elif i % 5 == 0:
            q[0] = ord("+")
        nm = b"r%d" % i + (b"/%d" % (1 + i % 2) if i % 4 == 1 else b"")
        cm = [b"", b"BC:Z:ACGT\tRX:Z:TTT", b"two words", b"x"][i % 4]
        out.append((nm, cm, s, bytes(q)))
    return out


def _write_fq(path, recs, crlf=False, blanks=False, tab=False, tail_nl=True):
    e = b"\r\n" if crlf else b"\n"
    with open(path, "wb") as f:
        for i, (nm, cm, s, q) in enumerate(recs):
            sep = b"\t" if (tab and i % 2) else b" "
            f.write(b"@" + nm + ((sep + cm) if cm else b"") + e + s + e + b"+" + e + q)
            if tail_nl or i < len(recs) - 1:
                f.write(e)
            if blanks and i % 5 == 0:
                f.write(e)


def _parse_fq_numpy(path):
    """the four-line layout with array operations: lines (CR dropped), blank lines removed, then headers / sequences / qualities by position"""
    buf = np.fromfile(path, dtype=np.uint8)
    if buf[-1] != 10:
        buf = np.concatenate([buf, np.array([10], np.uint8)])
    nl = np.flatnonzero(buf == 10)
    starts = np.concatenate([[0], nl[:-1] + 1]); ends = nl.copy()
    raw_ends = ends.copy()
    cr = (ends > starts) & (buf[np.maximum(ends - 1, 0)] == 13)
    ends = ends - cr
    keep = ends > starts
    starts, ends, raw_ends = starts[keep], ends[keep], raw_ends[keep]
    assert len(starts) % 4 == 0
    names, comments, seqs, quals = [], [], [], []
    for k in range(0, len(starts), 4):
        h = buf[starts[k] + 1:ends[k]].tobytes()
        j = min([x for x in (h.find(b" "), h.find(b"\t")) if x >= 0], default=-1)
        nm = h if j < 0 else h[:j]
        if len(nm) > 2 and nm[-2:-1] == b"/" and nm[-1:].isdigit():
            nm = nm[:-2]
        cm = b""
        if j >= 0:
            cm = buf[starts[k] + 2 + j:raw_ends[k]].tobytes()         # (kseq: the rest of the raw line, its CR dropped when longer than the CR)
            if len(cm) > 1 and cm[-1:] == b"\r":
                cm = cm[:-1]
        names.append(nm); comments.append(cm)
        seqs.append(buf[starts[k + 1]:ends[k + 1]].tobytes()); quals.append(buf[starts[k + 3]:ends[k + 3]].tobytes())
    return names, comments, seqs, quals


def _split(blob, offs, n):
    b = bytes(np.asarray(blob))
    return [b[int(offs[i]):b.index(b"\0", int(offs[i]))] for i in range(n)]


@pytest.mark.parametrize("kw", [dict(), dict(crlf=True), dict(blanks=True, tab=True), dict(tail_nl=False), dict(crlf=True, blanks=True, tab=True, tail_nl=False)])
def test_fastq_loader_equals_numpy_parse(tmp_path, kw):
    """letters, nt4 codes, qualities, names (trim_readno) and comments of FASTQ files with LF / CR LF, blank lines, comments behind a blank or a tab,
    quality lines that begin with '@' and '+'; 1, 7 and 20 000 reads (a file beyond 1 MB is cut across host threads)"""
    rng = np.random.default_rng(5)
    p = str(tmp_path / "r.fq")
    for n in (1, 7, 20000):
        _write_fq(p, _records(rng, n), **kw)
        if n == 20000:
            assert os.path.getsize(p) > (1 << 20)
        names, comments, seqs, quals = _parse_fq_numpy(p)
        a = read_reads(p, comments=True)
        assert len(a) == n
        assert list(a.lens) == [len(s) for s in seqs]
        assert bytes(a.ascii[:int(a.lens.sum())]) == b"".join(seqs)
        assert bytes(a.qual[:int(a.lens.sum())]) == b"".join(quals)
        assert np.array_equal(a.offs, np.concatenate([[0], np.cumsum(a.lens)[:-1]]).astype(np.uint64))
        assert np.array_equal(a.codes[:int(a.lens.sum())], _NT4[a.ascii[:int(a.lens.sum())]])
        assert _split(a.name_blob, a.name_off, n) == names
        assert _split(a.comments[0], a.comments[1], n) == comments
        b = read_reads(p)                                              # without comments: none kept
        assert b.comments is None and bytes(b.qual) == bytes(a.qual) and np.array_equal(b.name_blob, a.name_blob)
        s = a.slice(n // 2, n)
        assert bytes(s.qual) == b"".join(quals[n // 2:]) and _split(s.comments[0], s.comments[1], n - n // 2) == comments[n // 2:]


def test_fastq_comment_edge_cases(tmp_path):
    """kseq's comment: the raw rest of the header line behind the first blank; a trailing CR is dropped only when the comment is longer than it"""
    p = str(tmp_path / "e.fq")
    open(p, "wb").write(b"@a\r\nAC\r\n+\r\nII\r\n@b \r\nAC\r\n+\r\nII\r\n@c  x y\r\nAC\r\n+\r\nII\r\n@d\tt\tu\nAC\n+\nII\n@e\nAC\n+\nII\n")
    a = read_reads(p, comments=True)
    assert _split(a.name_blob, a.name_off, 5) == [b"a", b"b", b"c", b"d", b"e"]
    assert _split(a.comments[0], a.comments[1], 5) == [b"", b"\r", b" x y", b"t\tu", b""]


def test_fasta_through_the_new_loader_equals_the_fasta_loader(tmp_path):
    rng = np.random.default_rng(2)
    p = str(tmp_path / "r.fa")
    with open(p, "wb") as f:
        for i in range(20000):
            f.write(b">r%d%s\n" % (i, b" c%d" % i if i % 2 else b"") + rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=int(rng.integers(1, 200))).tobytes() + b"\n")
    a, b = read_reads(p, comments=True), read_fasta_reads(p)
    for k in ("ascii", "codes", "offs", "lens", "name_blob", "name_off"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.qual is None and _split(a.comments[0], a.comments[1], 4) == [b"", b"c1", b"", b"c3"]
    from bwamem_hip.lib import fasta_scan, reads_scan
    assert reads_scan(p) == fasta_scan(p)


@pytest.mark.parametrize("text,what", [
    (b"@a\nACGT\n+\nIII\n", "quality line whose length differs"),
    (b"@a\nACGT\n@b\nACGT\n+\nIIII\n", r"without its '\+' line"),
    (b"@a\nACGT\n+\nIIII\n@b\nACGT\n", "truncated"),
    (b"@a\nACGT\n+\n", "truncated"),
    (b"@a\nACGT\nACGT\n+\nIIIIIIII\n", "multi-line"),
    (b"@a\nACGT\n+\nIIII\nIIII\n", "multi-line"),
    (b"@a\nACGT\n+\nIIII\n>b\nACGT\n", "mixed"),
    (b">a\nACGT\n@b\nACGT\n+\nIIII\n", "mixed"),
])
def test_fastq_loader_refuses_malformed_files(tmp_path, text, what):
    p = str(tmp_path / "bad.fq")
    open(p, "wb").write(text)
    with pytest.raises(ValueError, match=what):
        read_reads(p)
    from bwamem_hip.lib import reads_scan
    with pytest.raises(ValueError, match=what):
        reads_scan(p)
    with pytest.raises(ValueError, match="alternating"):             # the FASTA loader keeps its one refusal
        read_fasta_reads(p)


def test_copy_comment_option():
    import ctypes as C
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import ChainOpt, ExtParams, PeOpt, PostOpt, load_library

    class _Opts:
        def __init__(self):
            L = load_library()
            self.copt = ChainOpt(); L.bmh_chain_opt_default(C.byref(self.copt))
            self.ep = ExtParams.default()
            self.po = PostOpt(); L.bmh_post_opt_default(C.byref(self.po))
            self.pe = PeOpt(); L.bmh_pe_opt_default(C.byref(self.pe))
    o = _Opts()
    assert o.po.copy_comment == 0
    Aligner.set_options(o, ["-a"])
    assert o.po.copy_comment == 0
    Aligner.set_options(o, ["-C", "-k", "21"])
    assert o.po.copy_comment == 1 and o.copt.min_seed_len == 21


def test_read_set_from_lists_quals_and_comments():
    rs = ReadSet.from_lists(["a", "b", "c"], ["ACG", "T", "GGGG"], quals=["I#I", "@", "+III"], comments=["", "BC:Z:A", "x y"])
    assert bytes(rs.qual) == b"I#I@+III"
    s = rs.slice(1, 3)
    assert bytes(s.qual) == b"@+III" and _split(s.comments[0], s.comments[1], 2) == [b"BC:Z:A", b"x y"]
    with pytest.raises(ValueError):
        ReadSet.from_lists(["a"], ["ACG"], quals=["II"])


# ---------------------------------------------------------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _genome(tmp_path, n=1_200_000, contigs=None, alt=0):
    from bwamem_hip import fmindex, synth
    g = synth.make_genome(n, seed=42, repeat_frac=0.2)
    prefix = str(tmp_path / "g.fa")
    fmindex.write_index(prefix, fmindex.build_fmd_index(g)); fmindex.write_bns(prefix, g, contigs=contigs)
    if alt:
        with open(prefix + ".alt", "w") as f:
            for c in contigs[-alt:]:
                f.write("%s\t0\t%s\t1\t60\t100M\t*\t0\t0\t*\t*\n" % (c[0], contigs[0][0]))
    return g, prefix


def _hard_reads(g, n, L, paired, seed=7):
    """diverged, chimeric and unmappable reads among plain ones: supplementary records with hard clips, reverse strands, unmapped reads and mates"""
    from bwamem_hip import synth
    reads = (synth.make_pairs(g, n // 2, L, seed=seed, sub_rate=0.02)[0] if paired else synth.make_reads(g, n, L, seed=seed, sub_rate=0.02)[0]).copy()
    rng = np.random.default_rng(seed + 1)
    for i in range(n):
        kind = i % 10
        if kind == 3:
            q = rng.random(L) < 0.12; reads[i][q] = (reads[i][q] + rng.integers(1, 4, size=int(q.sum()))) & 3
        elif kind == 5:
            k = int(rng.integers(50, 100)); p1 = int(rng.integers(0, len(g) - L)); b = g[p1:p1 + L - k].copy()
            reads[i][k:] = synth.revcomp(b) if rng.random() < 0.5 else b
        elif kind == 7:
            reads[i] = rng.integers(0, 4, size=L).astype(np.uint8)
    return reads


def _write_pair_files(tmp_path, reads, paired, tag, comments=None, crlf=False):
    """the same reads as FASTQ (random qualities, some lines starting with '@' / '+') and as FASTA; names p<k>/1 p<k>/2 for pairs.
    A comment "<blank>" writes a header that ends in a blank; crlf: CR LF line ends"""
    from bwamem_hip import synth
    fq, fa = str(tmp_path / (tag + ".fq")), str(tmp_path / (tag + ".fa"))
    quals = synth.random_quals([len(r) for r in reads], seed=3)
    asc = [synth.codes_to_ascii(np.asarray(r)).tobytes() for r in reads]
    names = [(b"p%d/%d" % (i // 2, i % 2 + 1)) if paired else (b"r%d" % i) for i in range(len(reads))]
    if comments is None:
        comments = ["" if i % 4 == 0 else ("BC:Z:ACGT\tRX:Z:GG%d" % i if i % 4 == 1 else "free text %d" % i) for i in range(len(reads))]
    e = b"\r\n" if crlf else b"\n"
    with open(fq, "wb") as f, open(fa, "wb") as g:
        for i, a in enumerate(asc):
            c = b" " if comments[i] == "<blank>" else (b" " + comments[i].encode()) if comments[i] else b""
            f.write(b"@" + names[i] + c + e + a + e + b"+" + e + quals[i].tobytes() + e)
            g.write(b">" + names[i] + c + e + a + e)
    return fq, fa, quals, comments


def _body(text):
    if isinstance(text, bytes):
        text = text.decode()
    return [l for l in text.split("\n") if l and l[0] != "@"]


def _expected_qual(rec, qual):
    """QUAL by the rule of mem_aln2sam (src/bwamem.c:1575-1612): '*' on 0x100 records, else the qualities of SEQ's bases -- those the hard clips
    leave -- reversed on the reverse strand"""
    import re
    f = rec.split("\t")
    flag = int(f[1])
    if flag & 0x100:
        return "*"
    ops = re.findall(r"(\d+)([MIDSH])", f[5]) if f[5] != "*" else []
    h0 = int(ops[0][0]) if ops and ops[0][1] == "H" else 0
    h1 = int(ops[-1][0]) if len(ops) > 1 and ops[-1][1] == "H" else 0
    q = bytes(qual)[::-1] if flag & 0x10 else bytes(qual)
    return q[h0:len(q) - h1].decode()


def _check_fastq_against_fasta(fa_recs, fq_recs, quals, comments, copy_comment, names_to_idx):
    assert len(fa_recs) == len(fq_recs)
    n_rev = n_hard = n_unmapped = 0
    for a, b in zip(fa_recs, fq_recs):
        fb = b.split("\t")
        i = names_to_idx(fb[0], int(fb[1]))
        if copy_comment and comments[i]:
            suffix = "\t" + comments[i]
            assert b.endswith(suffix), (b, comments[i])
            b = b[:-len(suffix)]
            fb = b.split("\t")
        assert fb[10] == _expected_qual(b, quals[i]), b
        assert "\t".join(fb[:10] + ["*"] + fb[11:]) == a
        flag = int(fb[1])
        n_rev += bool(flag & 0x10); n_hard += "H" in fb[5]; n_unmapped += bool(flag & 4)
    return n_rev, n_hard, n_unmapped


def _pe_index(name, flag):
    return 2 * int(name[1:]) + (1 if flag & 0x80 else 0)


@pytest.mark.gpu
def test_dropin_seeding_reads_fastq(hip, tmp_path):
    """seed_gpu (the drop-in seeding library) on a FASTQ file gives the seeds of the same reads in FASTA"""
    from bwamem_hip import synth
    g, prefix = _genome(tmp_path, n=600_000)
    reads, _ = synth.make_reads(g, 3000, 150, seed=4)
    fq, fa, _, _ = _write_pair_files(tmp_path, list(reads), False, "s")
    a, b = hip.seed_file(prefix, fa, 19), hip.seed_file(prefix, fq, 19)
    assert len(a["n_ref_pos"]) == len(b["n_ref_pos"]) == 3000 and len(a["rbeg"]) > 3000
    for k in ("rbeg", "qbeg", "score", "n_ref_pos", "prefix"):
        assert np.array_equal(a[k], b[k]), k
    assert b["file_bytes"] == os.path.getsize(fq)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["se", "pe", "se_hard", "pe_hard", "se_edge"])
def test_reference_parity_fastq(hip, tmp_path, mode):
    """the reference's host code (oracle/_ref/dropin/bwa-gasal2, linked on this library) and Aligner.align_file on the same FASTQ file write
    the same SAM, byte for byte: with and without -C, and once with -a -Y.  se_edge: CR LF line ends and the comments' edge cases -- a tab or a
    second blank behind the name, a header that ends in a blank (kseq keeps its CR as the comment), a comment that ends in a blank"""
    if not os.path.exists(DROPIN):
        pytest.skip("oracle/_ref/dropin/bwa-gasal2 not built (needs the reference sources at build time)")
    from bwamem_hip import synth
    from bwamem_hip.aligner import Aligner
    paired, hard = mode.startswith("pe"), mode.endswith("hard")
    g, prefix = _genome(tmp_path)
    n, L = 4000, 150
    reads = _hard_reads(g, n, L, paired) if hard else (synth.make_pairs(g, n // 2, L, seed=7)[0] if paired else synth.make_reads(g, n, L, seed=7)[0])
    edge = mode == "se_edge"
    cm = ["", " lead", "a\tb", "tail ", "<blank>", "BC:Z:ACGT\tRX:Z:GG"] * (n // 6 + 1) if edge else None
    fq, _, _, _ = _write_pair_files(tmp_path, list(reads), paired, "r", comments=cm[:n] if edge else None, crlf=edge)
    al = Aligner(prefix, n_threads=4)
    for opts in ([], ["-C"]) + ((["-a", "-Y", "-C"],) if hard else ()):
        sam = str(tmp_path / "ref.sam")
        with open(sam, "w") as f:
            r = subprocess.run([DROPIN, "gase_aln", "-t", "1", "-K", "2000000000", "-l", str(L)] + opts + (["-p"] if paired else []) + [prefix, fq],
                               stdout=f, stderr=subprocess.PIPE, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        theirs = _body(open(sam, "rb").read())                          # (bytes: a comment may hold a CR)
        al.po.flag_all = al.po.softclip = al.po.copy_comment = 0
        al.set_options(opts)
        buf = io.BytesIO()
        al.align_file(fq, buf, batch_reads=1 << 30, paired=paired)
        ours = _body(buf.getvalue())
        diff = [(a, b) for a, b in zip(ours, theirs) if a != b]
        assert len(ours) == len(theirs) and not diff, (opts, len(ours), len(theirs), diff[:2])
        assert all(l.split("\t")[10] != "*" for l in ours if not int(l.split("\t")[1]) & 0x100)
        if "-C" in opts:
            assert sum("\tBC:Z:ACGT\tRX:Z:GG" in l for l in ours) > n // 8
            if edge:
                assert any(l.endswith("\t\r") for l in ours) and any(l.endswith("\t lead") for l in ours)
        if hard:
            flags = [int(l.split("\t")[1]) for l in ours]
            assert any(f & 0x800 for f in flags) and any(f & 4 for f in flags) and any(f & 0x10 for f in flags)
            assert any("H" in l.split("\t")[5] for l in ours) or "-Y" in opts
    al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_fastq_records_are_fasta_records_plus_qual_and_comment(hip, tmp_path, paired):
    """no oracle: the same reads as FASTA and as FASTQ -- every FASTQ record is its FASTA record with QUAL derived from the qualities by the
    rule of src/bwamem.c:1575-1612 and, with -C, a tab and the comment at its end; on an index with ALT contigs (no hard clips on ALT hits)"""
    from bwamem_hip.aligner import Aligner
    contigs = [("chr1", 500_000), ("chr2", 400_000), ("chr1_alt", 150_000), ("chr2_alt", 150_000)]
    g, prefix = _genome(tmp_path, n=1_200_000, contigs=contigs, alt=2)
    n, L = 6000, 150
    reads = _hard_reads(g, n, L, paired, seed=11)
    fq, fa, quals, comments = _write_pair_files(tmp_path, list(reads), paired, "r")
    al = Aligner(prefix, n_threads=4)
    assert al.has_alt
    idx = _pe_index if paired else (lambda name, flag: int(name[1:]))
    for opts in ([], ["-C"]):
        al.set_options(opts)
        out = {}
        for p in (fa, fq):
            buf = io.BytesIO()
            al.align_file(p, buf, batch_reads=1 << 30 if paired else 0, paired=paired)
            out[p] = _body(buf.getvalue())
        if opts:                                              # (-C on the FASTA file: the comments too; without them QUAL is all that differs)
            fa_plain = []
            for l in out[fa]:
                f = l.split("\t"); i = idx(f[0], int(f[1]))
                fa_plain.append(l[:-len(comments[i]) - 1] if comments[i] else l)
            out[fa] = fa_plain
        n_rev, n_hard, n_unmapped = _check_fastq_against_fasta(out[fa], out[fq], quals, comments, bool(opts), idx)
        assert n_rev > 100 and n_hard > 5 and n_unmapped > 5, (n_rev, n_hard, n_unmapped)
        assert any("pa:f:" in l or "chr1_alt" in l.split("\t")[2] for l in out[fq])
    al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_fastq_device_text_equals_host_text(hip, tmp_path, paired, monkeypatch):
    """on FASTQ with -C: the native pipeline (QUAL and comments written by sam_text_*_kernel), its host formatter (BMH_ALIGNER_HOST_FORMAT)
    and the batch-by-batch loop (BMH_ALIGNER_NATIVE=0: bmh_format_sam_ex / _pe_ex) write the same bytes"""
    from bwamem_hip.aligner import Aligner
    contigs = [("chrA", 500_000), ("chrB", 400_000), ("chrC", 300_000)]
    g, prefix = _genome(tmp_path, contigs=contigs)
    reads = _hard_reads(g, 8000, 250, paired, seed=21)
    fq, _, _, _ = _write_pair_files(tmp_path, list(reads), paired, "r")
    al = Aligner(prefix, n_threads=4)
    al.set_options(["-C"])
    texts = {}
    for env in ("", "BMH_ALIGNER_HOST_FORMAT", "BMH_ALIGNER_NATIVE"):
        if env:
            monkeypatch.setenv(env, "0" if env == "BMH_ALIGNER_NATIVE" else "1")
        buf = io.BytesIO()
        al.align_file(fq, buf, batch_reads=3000, paired=paired)
        texts[env] = buf.getvalue()
        if env:
            monkeypatch.delenv(env)
    body = texts[""]
    assert b"\tSA:Z:" in body and b"\tBC:Z:ACGT" in body
    for env in ("BMH_ALIGNER_HOST_FORMAT", "BMH_ALIGNER_NATIVE"):
        assert texts[env] == body, env
    al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_fastq_streamed_equals_loaded(hip, tmp_path, paired, monkeypatch):
    """bmh_aligner_run_file (a loader thread cuts the FASTQ file -- quality lines beginning with '@' and '+' among them -- and fills pinned
    batches with letters, qualities and comments) equals bmh_reads_load + bmh_aligner_run, at several batch sizes (odd ones too) and -K cuts"""
    from bwamem_hip import synth
    from bwamem_hip.aligner import Aligner
    g, prefix = _genome(tmp_path, n=800_000)
    n = 9000
    reads = synth.make_pairs(g, n // 2, 150, seed=8)[0] if paired else synth.make_reads(g, n, 150, seed=8)[0]
    fq, _, _, _ = _write_pair_files(tmp_path, list(reads), paired, "r")
    al = Aligner(prefix, n_threads=4)
    al.set_options(["-C"])
    for batch_reads, chunk in ((0, 150_001), (0, 400_000), (997, 0), (2001, 0), (4096, 0)):
        res = []
        for stream in ("1", "0"):
            monkeypatch.setenv("BMH_ALIGNER_STREAM", stream)
            buf = io.BytesIO()
            al.align_file(fq, buf, batch_reads=batch_reads, paired=paired, chunk_bases=chunk)
            res.append(buf.getvalue())
        assert res[0] == res[1], (batch_reads, chunk)
        assert len(_body(res[0])) >= n
    al.close()


@pytest.mark.gpu
def test_fastq_long_reads_qual(hip, tmp_path):
    """Aligner(long_reads=True) on FASTQ reads of 1 000 - 2 500 bp: QUAL of every record by the rule (trimmed by hard clips, reversed on the
    reverse strand), the rest of the record as for the same reads in FASTA"""
    from bwamem_hip import synth
    from bwamem_hip.aligner import Aligner
    g, prefix = _genome(tmp_path, n=1_000_000)
    rng = np.random.default_rng(4)
    reads = []
    for i in range(120):
        ln = int(rng.integers(1000, 2501)); p0 = int(rng.integers(0, len(g) - ln))
        x = g[p0:p0 + ln].copy()
        q = rng.random(ln) < 0.01; x[q] = (x[q] + 1) & 3
        if i % 6 == 1:                                        # chimeric: a supplementary record with hard clips
            p1 = int(rng.integers(0, len(g) - ln)); x[ln // 2:] = g[p1:p1 + ln - ln // 2]
        reads.append(x if i % 2 else synth.revcomp(x))
    fq, fa, quals, comments = _write_pair_files(tmp_path, reads, False, "long")
    al = Aligner(prefix, n_threads=4, long_reads=True)
    al.set_options(["-C"])
    out = {}
    for p in (fa, fq):
        buf = io.BytesIO()
        al.align_file(p, buf)
        out[p] = _body(buf.getvalue())
    fa_plain = []
    for l in out[fa]:
        f = l.split("\t"); i = int(f[0][1:])
        fa_plain.append(l[:-len(comments[i]) - 1] if comments[i] else l)
    n_rev, n_hard, _ = _check_fastq_against_fasta(fa_plain, out[fq], quals, comments, True, lambda name, flag: int(name[1:]))
    assert n_rev >= 50 and n_hard >= 5, (n_rev, n_hard)
    al.close()
