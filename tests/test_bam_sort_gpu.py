"""Coordinate-sorted BAM on the device: the corpora of test_bam_sort.py through the kernels (device bytes equal the host forms' bytes), a sort over several blocks,
reads -> sorted BAM + BAI end to end against the Python sorter, BAI builder and region queries of test_bam_sort.py applied to the SAM text of the same run, the run
store spilled to its temporary file, and the `python -m bwamem_hip.mem --sort` command."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import common
from test_bam_core import encode_text
from test_bam_gpu import PREFIX, _reads_files, _sam_body
from test_bam_sort import BamFile, check_file, corpus, py_sort

HD = "@HD\tVN:1.6\tSO:coordinate\n"


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.mark.gpu
@pytest.mark.parametrize("window", [0, 1, 7, 100])
def test_sorted_file_device_equals_host(hip, window):
    """every set of the corpus at every window, one-record windows included: there a record beyond one BGZF piece is alone in its window (two members, the
    chunk's end in the next window's first member) and every record is a window's first, so each is a head on the device that the host joins to its chunk"""
    from bwamem_hip.lib import bam_sorted_file
    for what, contigs, stream in corpus():
        assert bam_sorted_file("@CO\tx\n", contigs, stream, 1, window) == bam_sorted_file("@CO\tx\n", contigs, stream, 1, window, host=True), (what, window)


@pytest.mark.gpu
def test_device_equals_host(hip):
    from bwamem_hip.lib import bam_sort, bam_sorted_file
    for what, contigs, stream in corpus():
        assert bam_sort(stream) == bam_sort(stream, host=True), what
    what, contigs, stream = corpus()[0]
    assert bam_sorted_file("", contigs, stream, 0, 100) == bam_sorted_file("", contigs, stream, 0, 100, host=True)
    with pytest.raises(ValueError):
        bam_sort(stream[:-1])


@pytest.mark.gpu
def test_larger_sort(hip):
    """70 000 records with random references (-1 among them) and positions: several blocks of the sort and of the gather, many equal keys"""
    from bwamem_hip.lib import bam_sort, bam_sorted_file
    rng = np.random.default_rng(2)
    n = 70_000
    rec = np.zeros((n, 48), np.uint8)                                     # block_size 44: the fixed fields, a 4-byte name, one operation, l_seq 2 -> 1 + 2 bytes, one spare
    rid = rng.integers(-1, 4, n).astype(np.int32); pos = rng.integers(0, 3000, n).astype(np.int32)
    pos[rid < 0] = -1
    flag = (rng.integers(0, 2, n) * 16).astype(np.uint16)
    rec[:, 0:4] = np.frombuffer(struct.pack("<I", 44), np.uint8)
    rec[:, 4:8] = rid.view(np.uint8).reshape(n, 4); rec[:, 8:12] = pos.view(np.uint8).reshape(n, 4)
    rec[:, 12] = 4; rec[:, 14:16] = np.frombuffer(struct.pack("<H", 4681), np.uint8); rec[:, 16] = 1
    rec[:, 18:20] = flag.view(np.uint8).reshape(n, 2); rec[:, 20] = 2
    rec[:, 36:39] = np.frombuffer(b"abc", np.uint8)
    rec[:, 40:44] = np.frombuffer(struct.pack("<I", 2 << 4), np.uint8)
    rec[:, 47] = (np.arange(n) % 251).astype(np.uint8)                    # tells equal keys apart: stability is visible
    stream = rec.tobytes()
    want = py_sort(stream)
    assert bam_sort(stream) == want
    contigs = [("a", 5000), ("b", 5000), ("c", 5000), ("d", 5000)]
    bam, bai = bam_sorted_file(HD, contigs, stream, 1, 20_000)
    check_file(bam, bai, HD, contigs, stream, "70 000 records", n_regions=5)


# ---------------------------------------------------------------------------------------------------------------- end to end

def _sorted_run(al, path, level=1, **kw):
    out, idx = io.BytesIO(), io.BytesIO()
    al.align_file(path, out, fmt="bam", level=level, sort=True, index=idx, **kw)
    return out.getvalue(), idx.getvalue()


def _check_sorted(al, path, monkeypatch, tmp_path, **kw):
    body = _sam_body(al, lambda o: al.align_file(path, o, **kw))
    unsorted = io.BytesIO(); al.align_file(path, unsorted, fmt="bam", **kw)
    stream, st = encode_text(body, al.contigs)
    assert not st.any() and body.count(b"\n") >= 600
    files = {}
    for level in (0, 1):
        bam, bai = _sorted_run(al, path, level, sort_window=100, **kw)
        assert al.last_stats.n_batches >= 3
        f = check_file(bam, bai, HD + al.header(), al.contigs, stream, level)
        assert len(f.coff) >= 8                                            # (several windows: every one ends its last member short)
        files[level] = (bam, bai)
    spill = tmp_path / "spill"; spill.mkdir()
    assert _sorted_run(al, path, 1, sort_window=100, sort_mem=1, sort_tmp=str(spill), **kw) == files[1]      # every run through the temporary file
    assert os.listdir(spill) == []
    bam, bai = _sorted_run(al, path, 1, **kw)                             # the default window: one
    check_file(bam, bai, HD + al.header(), al.contigs, stream, "one window")
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")
    assert BamFile(_sorted_run(al, path, 1, sort_window=100, **kw)[0]).stream == py_sort(stream)
    monkeypatch.delenv("BMH_ALIGNER_HOST_FORMAT")
    assert _sam_body(al, lambda o: al.align_file(path, o, **kw)) == body   # the output is switched back
    again = io.BytesIO(); al.align_file(path, again, fmt="bam", **kw)
    assert again.getvalue() == unsorted.getvalue()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_reads_to_sorted_bam(hip, tmp_path, monkeypatch, paired):
    from bwamem_hip.aligner import Aligner
    path = _reads_files(tmp_path, paired)
    al = Aligner(PREFIX, n_threads=4)
    if paired:
        al.set_options(["-C"])
    _check_sorted(al, path, monkeypatch, tmp_path, paired=paired, batch_reads=256)
    if not paired:
        out = io.BytesIO(); al.align_files(path, out=out, fmt="bam", sort=True, batch_reads=256)                 # align_files, no index asked for
        assert BamFile(out.getvalue()).stream == BamFile(_sorted_run(al, path, batch_reads=256)[0]).stream
        good = _sorted_run(al, path, sort_window=100, batch_reads=256)

        class Full(io.BytesIO):                                            # a sink that refuses the third window: the run fails with a part of its file written
            calls = 0

            def write(self, b):
                self.calls += 1
                if self.calls > 3:
                    raise OSError("no space")
                return super().write(b)
        with pytest.raises(OSError, match="no space"):
            al.align_file(path, Full(), fmt="bam", sort=True, index=io.BytesIO(), sort_window=100, batch_reads=256)
        with pytest.raises(ValueError, match="failed"):                    # ... and leaves no index of that part
            al._native.sort_index(0)
        assert _sorted_run(al, path, sort_window=100, batch_reads=256) == good
    al.close()


@pytest.mark.gpu
def test_reads_to_sorted_bam_alt_index(hip, tmp_path, monkeypatch):
    """several contigs, ALT contigs among them (the genome and reads of tests/golden/alt_golden.npz)"""
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
    assert al.has_alt and len(al.contigs) > 1
    _check_sorted(al, path, monkeypatch, tmp_path, batch_reads=256)
    al.close()


@pytest.mark.gpu
def test_mem_command_sort(hip, tmp_path):
    from bwamem_hip.aligner import Aligner
    path = _reads_files(tmp_path, True)
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(common.GOLDEN), "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def mem(*args):
        return subprocess.run([sys.executable, "-m", "bwamem_hip.mem", *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    bam = str(tmp_path / "x.bam")
    r = mem("-C", "-p", "--sort", "--sort-tmp", str(tmp_path), "--sort-mem", "100000", PREFIX, path, "-o", bam)
    assert r.returncode == 0, r.stderr.decode()
    al = Aligner(PREFIX)
    al.set_options(["-C"])
    body = _sam_body(al, lambda o: al.align_file(path, o, paired=True))   # the same reads and options in this process
    stream, st = encode_text(body, al.contigs)
    assert not st.any()
    with open(bam, "rb") as f, open(bam + ".bai", "rb") as g:
        check_file(f.read(), g.read(), HD + al.header(), al.contigs, stream, "command")
    al.close()
    assert sorted(os.listdir(tmp_path)) == sorted(["x.bam", "x.bam.bai", os.path.basename(path)])
    assert mem("--index", "x", PREFIX, path).returncode == 2 and mem("--sort", "--sort-mem", "lots", PREFIX, path).returncode == 2
