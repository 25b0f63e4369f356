"""The CSI index on the device: the cases of test_bam_csi.py through the kernels (device bytes equal the host forms' bytes, BAM and index), a stream of 70 000
records across a contig of 2^31 - 1 bases, reads -> sorted BAM + CSI end to end, and the `python -m bwamem_hip.mem --csi` command."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import common
from test_bam_csi import BIG, HDR, check_csi, check_twelve, dup_pairs, inflate_csi, parse_csi, twelve_records
from test_bam_gpu import PREFIX, _reads_files
from test_bam_sort import BamFile, check_file, corpus, split_records


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.mark.gpu
@pytest.mark.parametrize("window", [0, 1, 7, 100])
def test_csi_device_equals_host(hip, window):
    from bwamem_hip.lib import bam_sorted_file
    for what, contigs, stream in list(corpus()) + [("twelve records", *twelve_records())]:
        dev = bam_sorted_file(HDR, contigs, stream, 1, window, index_format="csi")
        assert dev == bam_sorted_file(HDR, contigs, stream, 1, window, host=True, index_format="csi"), (what, window)
        assert inflate_csi(dev[1])[:4] == b"CSI\1"
    check_twelve(*dev)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [10, 24])
def test_csi_other_shifts_device_equal_host(hip, shift):
    from bwamem_hip.lib import bam_sorted_file
    for what, contigs, stream in [c for c in corpus() if c[0] in ("mixed", "a record over three members", "placed mates")] + [("twelve records", *twelve_records())]:
        dev = bam_sorted_file(HDR, contigs, stream, 1, 100, index_format="csi", csi_min_shift=shift)
        assert dev == bam_sorted_file(HDR, contigs, stream, 1, 100, host=True, index_format="csi", csi_min_shift=shift), (what, shift)
        check_csi(*dev, contigs, stream, shift, (what, shift), n_regions=10)
    check_twelve(*dev, shift)


@pytest.mark.gpu
def test_csi_markdup_device_equals_host(hip):
    from bwamem_hip.lib import bam_sorted_file
    top = (1 << 30) - (1 << 24)
    stream = dup_pairs(1 << 29)
    dev = bam_sorted_file(HDR, [("wheat_3B", top)], stream, 1, 3, markdup=True, index_format="csi")
    assert dev == bam_sorted_file(HDR, [("wheat_3B", top)], stream, 1, 3, host=True, markdup=True, index_format="csi")
    assert dev[2]["duplicate_pairs"] == 1 and dev[2]["duplicate_fragments"] == 1
    with pytest.raises(ValueError, match="wheat_3B"):
        bam_sorted_file(HDR, [("wheat_3B", top + 1)], stream, 1, 3, markdup=True, index_format="csi")
    groups = [("g", "lib")]
    tagged = b"".join(struct.pack("<I", len(r) - 4 + 5) + r[4:] + b"RGZg\0" for r in split_records(stream))
    dev = bam_sorted_file(HDR, [("wheat_3B", top)], tagged, 1, 0, markdup=True, read_groups=groups, index_format="csi")
    assert dev == bam_sorted_file(HDR, [("wheat_3B", top)], tagged, 1, 0, host=True, markdup=True, read_groups=groups, index_format="csi")
    assert dev[2]["libraries"]["lib"]["duplicate_pairs"] == 1


@pytest.mark.gpu
def test_csi_across_a_contig_of_2_31(hip):
    """70 000 records on a contig of 2^31 - 1 bases, positions across its whole range: 300 share one window of 2^14 bases (a whole workgroup sees one bin); a stretch
    of the input alternates between two references record by record; and 600 contigs of one record each follow, so that in the sorted file -- where the index
    pass's blocks see them -- the reference changes with every record and the count reduction takes its per-lane path"""
    from bwamem_hip.lib import bam_sorted_file
    rng = np.random.default_rng(29)
    n, tiny = 70_000, 600
    rid = np.zeros(n, np.int32)
    pos = rng.integers(0, BIG - 100, n).astype(np.int64)
    pos[1000:1300] = (5 << 28) + 7 * (1 << 14) + rng.integers(0, (1 << 14) - 60, 300)            # one window, beyond 2^30
    rid[2000:3000:2] = 1; pos[2000:3000:2] = rng.integers(0, 4000, 500)                          # 0, 1, 0, 1, ...
    rid[4000:4000 + tiny] = 2 + np.arange(tiny); pos[4000:4000 + tiny] = rng.integers(0, 40, tiny)
    rid[5000:5040] = -1; pos[5000:5040] = -1
    pos = pos.astype(np.int32)
    rec = np.zeros((n, 48), np.uint8)                                     # block_size 44: the fixed fields, a 4-byte name, one operation (50M), l_seq 2 -> 1 + 2 bytes, one spare
    flag = (rng.integers(0, 2, n) * 16).astype(np.uint16)
    flag[rid < 0] = 4
    rec[:, 0:4] = np.frombuffer(struct.pack("<I", 44), np.uint8)
    rec[:, 4:8] = rid.view(np.uint8).reshape(n, 4); rec[:, 8:12] = pos.view(np.uint8).reshape(n, 4)
    rec[:, 12] = 4; rec[:, 14:16] = np.frombuffer(struct.pack("<H", 4681), np.uint8); rec[:, 16] = 1
    rec[:, 18:20] = flag.view(np.uint8).reshape(n, 2); rec[:, 20] = 2
    rec[:, 36:39] = np.frombuffer(b"abc", np.uint8)
    rec[:, 40:44] = np.frombuffer(struct.pack("<I", 50 << 4), np.uint8)
    rec[:, 47] = (np.arange(n) % 251).astype(np.uint8)
    stream = rec.tobytes()
    contigs = [("big", BIG), ("b", 5000)] + [("t%d" % k, 100) for k in range(tiny)]
    dev = bam_sorted_file(HDR, contigs, stream, 1, 20_000, index_format="csi")
    assert dev == bam_sorted_file(HDR, contigs, stream, 1, 20_000, host=True, index_format="csi")
    f = check_csi(*dev, contigs, stream, 14, "70 000 records", n_regions=3)
    shift, depth, refs, no_coor = parse_csi(inflate_csi(dev[1]))
    assert depth == 6 and no_coor == 40 and all(len(b) == 2 for b in refs[2:]) and len(refs[0]) > 10_000
    one = 37449 + (((5 << 28) + 7 * (1 << 14)) >> 14)                     # the shared window's bin holds the 300 (and whoever else fell there) in one chunk
    assert len(refs[0][one][1]) == 1 and len(f.read_chunk(*refs[0][one][1][0])) >= 300


# ---------------------------------------------------------------------------------------------------------------- end to end

@pytest.mark.gpu
def test_reads_to_sorted_bam_and_csi(hip, tmp_path):
    from bwamem_hip.aligner import Aligner
    path = _reads_files(tmp_path, True)
    al = Aligner(PREFIX, n_threads=4)
    out, idx = io.BytesIO(), io.BytesIO()
    al.align_files(path, out=out, paired=True, fmt="bam", sort=True, index=idx, index_format="csi", sort_window=100, batch_reads=256)
    assert al.last_stats.n_batches >= 3
    bam, csi = out.getvalue(), idx.getvalue()
    f = BamFile(bam)
    assert len(f.recs) >= 600 and len(f.coff) >= 8
    check_csi(bam, csi, al.contigs, f.stream, 14, "end to end")
    out2, idx2 = io.BytesIO(), io.BytesIO()
    al.align_files(path, out=out2, paired=True, fmt="bam", sort=True, index=idx2, sort_window=100, batch_reads=256)
    assert out2.getvalue() == bam and idx2.getvalue()[:4] == b"BAI\1"       # the same records (the same file) under either index
    check_file(bam, idx2.getvalue(), f.header_text.decode(), al.contigs, f.stream, "the BAI run")
    assert al._native.sort_index(al._bam_header_bytes) == idx2.getvalue()    # the index of the last run, in that run's format
    out3, idx3 = io.BytesIO(), io.BytesIO()
    al.align_files(path, out=out3, paired=True, fmt="bam", sort=True, index=idx3, index_format="csi", csi_min_shift=10, markdup=True, sort_window=100, batch_reads=256)
    check_csi(out3.getvalue(), idx3.getvalue(), al.contigs, BamFile(out3.getvalue()).stream, 10, "shift 10, marked")
    al.close()


@pytest.mark.gpu
def test_mem_command_csi(hip, tmp_path):
    path = _reads_files(tmp_path, True)
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(common.GOLDEN), "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def mem(*args):
        return subprocess.run([sys.executable, "-m", "bwamem_hip.mem", *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    bam = str(tmp_path / "x.bam")
    r = mem("-p", "--csi", PREFIX, path, "-o", bam)
    assert r.returncode == 0, r.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == sorted(["x.bam", "x.bam.csi", os.path.basename(path)])
    with open(bam, "rb") as f, open(bam + ".csi", "rb") as g:
        blob, csi = f.read(), g.read()
    from bwamem_hip.aligner import Aligner
    al = Aligner(PREFIX)
    contigs = list(al.contigs)
    al.close()
    fb = BamFile(blob)
    assert b"SO:coordinate" in fb.header_text and len(fb.recs) >= 600
    check_csi(blob, csi, contigs, fb.stream, 14, "command")
    r = mem("-p", "--csi", "--csi-min-shift", "12", "--index", str(tmp_path / "named.csi"), PREFIX, path, "-o", bam)
    assert r.returncode == 0, r.stderr.decode()
    with open(bam, "rb") as f, open(tmp_path / "named.csi", "rb") as g:
        blob2, csi2 = f.read(), g.read()
    assert blob2 == blob and parse_csi(inflate_csi(csi2))[0] == 12
    assert mem("--sort", "--csi-min-shift", "12", PREFIX, path).returncode == 2
