"""The device record parser (csrc/reads_parse.hip) and the paths above it: bmh_reads_load_files on the device equals the host walker and the reference's
records at every window size; Aligner.align_files writes the bytes Aligner.align_file writes for the same reads in the one layout that takes; the
`python -m bwamem_hip.mem` command."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from test_reads_input import FIX, FIXTURES, bgzf, check_expected, fixture_text, forms, gzip_member, same_read_sets

CHUNKS = [None, 4093, 1531, 1000, 257, 64]


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(FIX, "expected.npz"))


def _set_chunk(chunk):
    import ctypes as C
    from bwamem_hip.lib import load_library
    L = load_library()
    L.bmh_tune_set.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.bmh_tune_set(b"READS_CHUNK_BYTES", int(chunk or 0), 0 if chunk else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_device_parser_equals_walker_and_reference(hip, tmp_path, expected, name):
    from bwamem_hip.aligner import read_reads_files
    from bwamem_hip.lib import reads_last_counts
    ff = forms(tmp_path, name, fixture_text(name))
    host = read_reads_files(ff["plain"], comments=True, host=True)
    try:
        for chunk in CHUNKS:
            _set_chunk(chunk)
            for tag, p in ff.items():
                dev = read_reads_files(p, comments=True)
                cnt = reads_last_counts()
                check_expected(expected, name, dev)
                same_read_sets(dev, host, (name, chunk, tag))
                if name == "ml.fq":                      # multi-line FASTQ is the host walker's
                    assert cnt["host_windows"] > 0, (chunk, tag, cnt)
                elif name in ("ml60.fa", "ml80_crlf.fa", "single.fa", "four.fq", "r1.fq", "r2.fq") and chunk is None:
                    assert cnt["host_windows"] == 0 and cnt["device_windows"] > 0, (name, tag, cnt)
                if name == "ml60.fa" and chunk is not None and chunk >= 1000:
                    assert cnt["host_windows"] == 0 and cnt["device_windows"] >= 1, (chunk, tag, cnt)
                    if chunk < len(fixture_text(name)):        # (the file is cut into several windows: records straddle them)
                        assert cnt["device_windows"] > 1, (chunk, tag, cnt)
            same_read_sets(read_reads_files(ff["plain"]), read_reads_files(ff["plain"], host=True), (name, chunk, "no comments"))
    finally:
        _set_chunk(0)


@pytest.mark.gpu
def test_device_parser_two_files(hip, tmp_path, expected):
    from bwamem_hip.aligner import read_reads_files
    from bwamem_hip.lib import reads_last_counts
    f1, f2 = forms(tmp_path, "r1.fq", fixture_text("r1.fq")), forms(tmp_path, "r2.fq", fixture_text("r2.fq"))
    try:
        for chunk in CHUNKS:
            _set_chunk(chunk)
            for t1, t2 in (("plain", "plain"), ("gz", "bgzf"), ("bgzf", "bgzf")):
                check_expected(expected, "r1.fq+r2.fq", read_reads_files(f1[t1], f2[t2], comments=True))
                assert reads_last_counts()["host_windows"] == 0
        _set_chunk(1000)
        short = str(tmp_path / "short.fq")
        with open(short, "wb") as f:
            f.write(b"\n".join(fixture_text("r2.fq").split(b"\n")[:4 * 9]) + b"\n")
        for a, b in ((f1["plain"], short), (short, f2["bgzf"])):
            with pytest.raises(ValueError, match=r"short.fq ends before .* \(after 9 pairs\)") as ei:
                read_reads_files(a, b)
            assert len(ei.value.partial) == 18
        with pytest.raises(ValueError, match="holds FASTQ records and .* FASTA records"):
            read_reads_files(f1["plain"], os.path.join(FIX, "single.fa"))
        bad = str(tmp_path / "q.fq")
        with open(bad, "wb") as f:
            f.write(fixture_text("four.fq") + b"@a\nACGT\n+\nIIIII\n")
        with pytest.raises(ValueError, match="quality line whose length differs"):
            read_reads_files(bad)
    finally:
        _set_chunk(0)


# ---------------------------------------------------------------------------------------------------------------- file -> SAM

def _genome(tmp_path, n=1_000_000):
    from bwamem_hip import fmindex, synth
    g = synth.make_genome(n, seed=42, repeat_frac=0.2)
    prefix = str(tmp_path / "g.fa")
    fmindex.write_index(prefix, fmindex.build_fmd_index(g)); fmindex.write_bns(prefix, g)
    return g, prefix


def _mixed_reads(g, n, paired, lengths=(50, 100, 150, 250, 400, 600)):
    """n reads (or n / 2 pairs) of several lengths, shuffled as pairs"""
    from bwamem_hip import synth
    rows = []
    per = n // len(lengths)
    for k, L in enumerate(lengths):
        if paired:
            r = synth.make_pairs(g, per // 2, L, seed=20 + k, insert_mean=max(350.0, 1.6 * L))[0]
            rows += [(r[2 * i], r[2 * i + 1]) for i in range(per // 2)]
        else:
            r = synth.make_reads(g, per, L, seed=20 + k)[0]
            rows += [(r[i],) for i in range(per)]
    order = np.random.default_rng(5).permutation(len(rows))
    return [x for i in order for x in rows[i]]


def _write_forms(tmp_path, reads, paired, tag):
    """the same reads as: single-line FASTA, 70-column FASTA, single-line (interleaved) FASTQ, FASTQ as BGZF -- one file, or R1 / R2 when paired"""
    from bwamem_hip import synth
    asc = [synth.codes_to_ascii(np.asarray(r)).tobytes() for r in reads]
    quals = [bytes(q) for q in synth.random_quals([len(a) for a in asc], seed=3)]
    def hdr(i):
        j = i // 2 if paired else i
        return b"%s%d%s%s" % (tag.encode(), j, (b"/%d" % (1 + (i & 1))) if paired else b"", b" BC:Z:%d\tx y" % (i % 97) if i % 3 else b"")
    fa1 = b"".join(b">" + hdr(i) + b"\n" + a + b"\n" for i, a in enumerate(asc))
    fa70 = b"".join(b">" + hdr(i) + b"\n" + b"".join(a[k:k + 70] + b"\n" for k in range(0, len(a), 70)) for i, a in enumerate(asc))
    rec = [b"@" + hdr(i) + b"\n" + a + b"\n+\n" + quals[i] + b"\n" for i, a in enumerate(asc)]
    out = {}
    def put(name, data):
        out[name] = str(tmp_path / f"{tag}.{name}")
        with open(out[name], "wb") as f:
            f.write(data)
    put("fa1", fa1); put("fa70", fa70); put("fq", b"".join(rec))
    if paired:
        put("r1.bgzf", bgzf(b"".join(rec[0::2]), 60000)); put("r2.bgzf", bgzf(b"".join(rec[1::2]), 60000))
        put("r1.fq", b"".join(rec[0::2])); put("r2.fq.gz", gzip_member(b"".join(rec[1::2])))
    else:
        put("fq.bgzf", bgzf(b"".join(rec), 60000))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_align_files_equals_align_file(hip, tmp_path, paired):
    """20 000 reads of 50 .. 600 bp: align_files on the plain single-line file, on 70-column FASTA and on BGZF FASTQ (R1 / R2 when paired) writes the bytes
    align_file writes for the single-line interleaved file, with and without -C, in several batches"""
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import reads_last_counts
    g, prefix = _genome(tmp_path)
    reads = _mixed_reads(g, 20_000, paired)
    ff = _write_forms(tmp_path, reads, paired, "m")
    for opts in ([], ["-C"]):
        al = Aligner(prefix, n_threads=8)
        al.set_options(opts)
        def run_file(p):
            buf = io.BytesIO(); al.align_file(p, buf, paired=paired, chunk_bases=700_001); return buf.getvalue()
        def run_files(p, q=None):
            buf = io.BytesIO(); n = al.align_files(p, q, out=buf, paired=paired, chunk_bases=700_001)
            assert n == len(reads) and al.last_stats.n_batches >= 5
            c = reads_last_counts()
            assert c["host_windows"] == 0 and c["device_windows"] >= 5, c
            return buf.getvalue()
        want_fa, want_fq = run_file(ff["fa1"]), run_file(ff["fq"])
        assert want_fa.count(b"\n") >= len(reads) and want_fq != want_fa
        assert run_files(ff["fa1"]) == want_fa, ("plain single-line", opts)
        assert run_files(ff["fa70"]) == want_fa, ("70-column FASTA", opts)
        assert run_files(ff["fq"]) == want_fq, ("plain FASTQ", opts)
        if paired:
            assert run_files(ff["r1.bgzf"], ff["r2.bgzf"]) == want_fq, ("R1 / R2 BGZF", opts)
            assert run_files(ff["r1.fq"], ff["r2.fq.gz"]) == want_fq, ("R1 plain, R2 gzip", opts)
        else:
            assert run_files(ff["fq.bgzf"]) == want_fq, ("BGZF", opts)
        al.close()


@pytest.mark.gpu
def test_align_files_long_reads(hip, tmp_path):
    from bwamem_hip.aligner import Aligner
    g, prefix = _genome(tmp_path)
    rng = np.random.default_rng(9)
    reads = []
    for i in range(90):
        ln = int(rng.integers(2000, 4001)); p0 = int(rng.integers(0, len(g) - ln))
        x = g[p0:p0 + ln].copy()
        q = rng.random(ln) < 0.01; x[q] = (x[q] + 1) & 3
        reads.append(x)
    ff = _write_forms(tmp_path, reads, False, "long")
    al = Aligner(prefix, n_threads=8, long_reads=True)
    out = {}
    for k in ("fa1", "fq"):
        buf = io.BytesIO(); al.align_file(ff[k], buf, chunk_bases=60_000); out[k] = buf.getvalue()
    for k, want in (("fa70", "fa1"), ("fq.bgzf", "fq")):
        buf = io.BytesIO(); al.align_files(ff[k], out=buf, chunk_bases=60_000)
        assert buf.getvalue() == out[want], k
    al.close()


@pytest.mark.gpu
def test_align_files_delivers_pairs_before_a_short_file(hip, tmp_path):
    from bwamem_hip.aligner import Aligner
    g, prefix = _genome(tmp_path)
    reads = _mixed_reads(g, 1200, True, lengths=(100, 150))
    ff = _write_forms(tmp_path, reads, True, "s")
    short = str(tmp_path / "short.fq")
    with open(ff["r1.fq"], "rb") as f:
        lines = f.read().split(b"\n")
    with open(short, "wb") as f:
        f.write(b"\n".join(lines[:4 * 500]) + b"\n")
    al = Aligner(prefix, n_threads=8)
    buf = io.BytesIO()
    with pytest.raises(ValueError, match=r"short.fq ends before .* \(after 500 pairs\)"):
        al.align_files(short, ff["r2.bgzf"], out=buf)
    names = [l.split(b"\t")[0] for l in buf.getvalue().split(b"\n") if l and not l.startswith(b"@")]
    assert len(set(names)) == 500
    al.close()


@pytest.mark.gpu
def test_mem_command(hip, tmp_path):
    g, prefix = _genome(tmp_path, n=600_000)
    reads = _mixed_reads(g, 1200, True, lengths=(100, 150))
    ff = _write_forms(tmp_path, reads, True, "c")
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(FIX), "..", "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def mem(*args):
        return subprocess.run([sys.executable, "-m", "bwamem_hip.mem", *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    from bwamem_hip.aligner import Aligner
    al = Aligner(prefix)
    al.set_options(["-C"])
    buf = io.BytesIO(); al.align_file(ff["fq"], buf, paired=True); want = buf.getvalue()
    buf = io.BytesIO(); al.align_file(ff["fa1"], buf, paired=True); want_fa = buf.getvalue()
    al.close()
    for inputs in ([ff["r1.bgzf"], ff["r2.bgzf"]], ["-p", ff["fq"]], ["-p", ff["fa70"]]):
        o = str(tmp_path / "o.sam")
        r1 = mem("-C", prefix, *inputs, "-o", o)
        assert r1.returncode == 0, r1.stderr.decode()
        r2 = mem("-C", prefix, *inputs)
        assert r2.returncode == 0, r2.stderr.decode()
        with open(o, "rb") as f:
            text = f.read()
        assert text == r2.stdout and len(text) > 0
        assert text == (want_fa if inputs[-1] == ff["fa70"] else want), inputs
    r = mem("-I", "300", prefix, ff["fq"])
    assert r.returncode == 2 and b"option -I is not taken" in r.stderr
    r = mem(prefix, ff["r1.bgzf"], ff["fa1"])
    assert r.returncode != 0 and b"holds FASTQ records and" in r.stderr
    r = mem(prefix, str(tmp_path / "absent.fq"))
    assert r.returncode != 0 and b"cannot open" in r.stderr
