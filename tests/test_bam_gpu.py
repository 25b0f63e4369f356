"""BAM output on the device: the record and member corpora of test_bam_core.py through the kernels (device bytes equal the host cores' bytes), reads -> BAM end
to end against the Python record encoder applied to the SAM text of the same run, and the `python -m bwamem_hip.mem --bam` command."""
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import common
from test_bam_core import CONTIGS, ENOEOL, PIECE, check_members, encode_text, golden_sam_texts, member_corpus, record_corpus, split_members

PREFIX = os.path.join(common.GOLDEN, "ref_index_g20011")


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.mark.gpu
def test_device_records_equal_host_records(hip):
    from bwamem_hip.lib import sam_to_bam
    text = record_corpus()
    want, want_st = encode_text(text, CONTIGS)
    for t in (text, text[:-1], text[:4000] * 40, b"\n", b""):
        h, hs = sam_to_bam(t, CONTIGS, host=True)
        d, ds = sam_to_bam(t, CONTIGS)
        assert ds.tolist() == hs.tolist() and d == h
    d, ds = sam_to_bam(text, CONTIGS)
    assert d == want and ds.tolist() == want_st.tolist()
    assert sam_to_bam(text[:-1], CONTIGS)[1][-1] == ENOEOL
    for what, full, body in golden_sam_texts():
        contigs = [(l.split(b"\t")[1][3:].decode(), int(l.split(b"\t")[2][3:])) for l in full.split(b"\n") if l.startswith(b"@SQ")]
        if not contigs:
            contigs = sorted({(l.split(b"\t")[k].decode(), 1 << 29) for l in body.split(b"\n") if l for k in (2, 6) if l.split(b"\t")[k] not in (b"*", b"=")})
        d, ds = sam_to_bam(body, contigs)
        w, ws = encode_text(body, contigs)
        assert not ds.any() and d == w, what


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1])
def test_device_members_equal_host_members(hip, level):
    from bwamem_hip.lib import bgzf_compress
    for name, data in member_corpus():
        h = bgzf_compress(data, level, host=True)
        d = bgzf_compress(data, level)
        assert d == h, name
        if data:
            check_members(d, data, level, name)
        assert bgzf_compress(data, level) == d, name


# ---------------------------------------------------------------------------------------------------------------- end to end

def _golden_genome():
    with open(PREFIX + ".fa", "rb") as f:
        seq = b"".join(l.strip() for l in f if not l.startswith(b">"))
    lut = np.full(256, 0, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i; lut[c + 32] = i
    return lut[np.frombuffer(seq, np.uint8)]


def _reads_files(tmp_path, paired, n=600, L=150):
    """n synthetic reads of the golden genome, a tenth of them chimeric or random: FASTA (single-end) or interleaved FASTQ whose comments are BC:Z: tags (paired)"""
    from bwamem_hip import synth
    g = _golden_genome()
    reads = (synth.make_pairs(g, n // 2, L, seed=3, sub_rate=0.02)[0] if paired else synth.make_reads(g, n, L, seed=3, sub_rate=0.02)[0]).copy()
    rng = np.random.default_rng(4)
    for i in range(0, n, 10):
        k = int(rng.integers(50, 100)); p = int(rng.integers(0, len(g) - L))
        reads[i][k:] = synth.revcomp(g[p:p + L - k]) if i % 20 else rng.integers(0, 4, L - k)
    asc = [synth.codes_to_ascii(np.asarray(r)).tobytes() for r in reads]
    path = str(tmp_path / ("r.fq" if paired else "r.fa"))
    with open(path, "wb") as f:
        if paired:
            quals = [bytes(q) for q in synth.random_quals([len(a) for a in asc], seed=3)]
            for i, a in enumerate(asc):
                f.write(b"@p%d/%d BC:Z:ACGT-%d\n%s\n+\n%s\n" % (i // 2, 1 + (i & 1), i % 7, a, quals[i]))
        else:
            for i, a in enumerate(asc):
                f.write(b">r%d\n%s\n" % (i, a))
    return path


def _records(blob: bytes, al, n_min_members=1) -> bytes:
    """the record stream of a BAM file: every member inflated by zlib, the end-of-file member last and no other empty, the header as bmh_bam_header writes it"""
    from bwamem_hip.lib import bam_header, bgzf_eof
    ms = split_members(blob)
    assert ms[-1] == bgzf_eof() and len(ms) - 1 >= n_min_members
    for m in ms[:-1]:
        assert struct.unpack("<I", m[-4:])[0] > 0
    data = b"".join(zlib.decompress(m, 31) for m in ms)
    hdr = bam_header(al.header(), al.contigs)
    assert data.startswith(hdr)
    return data[len(hdr):]


def _sam_body(al, run) -> bytes:
    buf = io.BytesIO(); run(buf)
    assert buf.getvalue().startswith(al.header().encode())
    return b"".join(l + b"\n" for l in buf.getvalue().split(b"\n") if l and not l.startswith(b"@"))


def _check_run(al, run_sam, run_bam, monkeypatch, tags=(), min_members=2):
    body = _sam_body(al, run_sam)
    want, st = encode_text(body, al.contigs)
    assert not st.any() and body.count(b"\n") >= 600
    for t in tags:
        assert t in body, t
    streams = {}
    for level in (0, 1):
        buf = io.BytesIO(); run_bam(buf, level)
        got = _records(buf.getvalue(), al, min_members)
        assert got == want, level
        streams[level] = buf.getvalue()
    assert len(streams[1]) < len(streams[0])                          # (level 0 stores; level 1 never writes a larger member, and this text compresses)
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")
    buf = io.BytesIO(); run_bam(buf, 1)
    assert _records(buf.getvalue(), al, 1) == want, "host format"
    monkeypatch.delenv("BMH_ALIGNER_HOST_FORMAT")
    assert _sam_body(al, run_sam) == body                              # the SAM run after the BAM runs: the output is switched back


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["se_fasta", "se_batches", "pe_fastq_comments", "read_group", "files"])
def test_reads_to_bam(hip, tmp_path, monkeypatch, case):
    from bwamem_hip.aligner import Aligner
    paired = case == "pe_fastq_comments"
    path = _reads_files(tmp_path, paired)
    al = Aligner(PREFIX, n_threads=4)
    al.set_options({"pe_fastq_comments": ["-C"], "read_group": ["-R", "@RG\\tID:grp1\\tSM:s"]}.get(case, []))
    kw = dict(paired=paired)
    if case == "se_batches":
        kw["chunk_bases"] = 25_000                                    # (-K: at least three batches, every batch ends its last member short)
    if case == "files":
        run_sam = lambda o: al.align_files(path, out=o, **kw)
        run_bam = lambda o, lv: al.align_files(path, out=o, fmt="bam", level=lv, **kw)
    else:
        run_sam = lambda o: al.align_file(path, o, **kw)
        run_bam = lambda o, lv: al.align_file(path, o, fmt="bam", level=lv, **kw)
    tags = {"pe_fastq_comments": (b"\tBC:Z:ACGT-3\n",), "read_group": (b"\tRG:Z:grp1",)}.get(case, ())
    _check_run(al, run_sam, run_bam, monkeypatch, tags, min_members=3 if case == "se_batches" else 2)
    if case == "se_batches":
        assert al.last_stats.n_batches >= 3
    if case == "se_fasta":                                             # align_batch: the batch's members alone
        from bwamem_hip.aligner import read_reads
        rs = read_reads(path)
        text = al.align_batch(rs, as_bytes=True)
        mem = al.align_batch(rs, fmt="bam", level=1)
        assert b"".join(zlib.decompress(m, 31) for m in split_members(mem)) == encode_text(bytes(text), al.contigs)[0]
        with pytest.raises(ValueError):
            al.align_file(path, io.StringIO(), fmt="bam")
    al.close()


@pytest.mark.gpu
def test_reads_to_bam_alt_index(hip, tmp_path, monkeypatch):
    """an index with ALT contigs named in <prefix>.alt (the genome and reads of tests/golden/alt_golden.npz): pa:f, XA and SA tags"""
    import ast
    from bwamem_hip import fmindex, synth
    from bwamem_hip.aligner import Aligner
    z = np.load(os.path.join(common.GOLDEN, "alt_golden.npz"))
    n = int(z["n_genome"]); bits = np.unpackbits(z["genome_packed"])[: 2 * n].reshape(n, 2)
    g = (bits[:, 0] * 2 + bits[:, 1]).astype(np.uint8)
    prefix = str(tmp_path / "g.fa")
    fmindex.write_index(prefix, fmindex.build_fmd_index(g)); fmindex.write_bns(prefix, g, contigs=ast.literal_eval(str(z["contigs"])))
    with open(prefix + ".alt", "wb") as f:
        f.write(bytes(z["alt_file"]))
    asc = synth.codes_to_ascii(z["reads"])
    path = str(tmp_path / "r.fa")
    with open(path, "wb") as f:
        for i in range(len(asc)):
            f.write(b">r%d\n%s\n" % (i, asc[i].tobytes()))
    al = Aligner(prefix, n_threads=4)
    assert al.has_alt
    _check_run(al, lambda o: al.align_file(path, o, batch_reads=256), lambda o, lv: al.align_file(path, o, batch_reads=256, fmt="bam", level=lv), monkeypatch,
               (b"pa:f:", b"XA:Z:", b"SA:Z:"), min_members=2)
    al.close()


@pytest.mark.gpu
def test_mem_command_bam(hip, tmp_path):
    path = _reads_files(tmp_path, True)
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(common.GOLDEN), "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def mem(*args):
        return subprocess.run([sys.executable, "-m", "bwamem_hip.mem", *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    sam, bam = str(tmp_path / "o.sam"), str(tmp_path / "o.sam.bam.txt")            # (the name does not choose the format)
    r = mem("-C", "-p", PREFIX, path, "-o", sam)
    assert r.returncode == 0, r.stderr.decode()
    r = mem("-C", "-p", "--bam", "--bam-level", "1", PREFIX, path, "-o", bam)
    assert r.returncode == 0, r.stderr.decode()
    with open(sam, "rb") as f:
        text = f.read()
    with open(bam, "rb") as f:
        blob = f.read()
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import bam_header
    al = Aligner(PREFIX)
    hdr_text = b"".join(l + b"\n" for l in text.split(b"\n") if l.startswith(b"@"))
    body = text[len(hdr_text):]
    data = b"".join(zlib.decompress(m, 31) for m in split_members(blob))
    hdr = bam_header(hdr_text.decode(), al.contigs)
    assert data.startswith(hdr) and data[len(hdr):] == encode_text(body, al.contigs)[0] and body.count(b"\n") >= 600
    al.close()
    # a -C comment that is no tag cannot be a BAM record: status 1, the read named
    bad = str(tmp_path / "bad.fq")
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    lines[4 * 10] = b"@p5/1 1:N:0:ACGT"
    with open(bad, "wb") as f:
        f.write(b"\n".join(lines))
    r = mem("-C", "-p", "--bam", PREFIX, bad, "-o", bam)
    assert r.returncode == 1 and b"read 'p5" in r.stderr and b"tag" in r.stderr, r.stderr.decode()
    r = mem("--bam-level", "2", PREFIX, path)
    assert r.returncode == 2
