"""BAM as read input on the device (csrc/bam_in_kernels.hip): the kernels equal the host form on every case of test_bam_input.py at every window size, the refusals
come with the host form's messages, and Aligner.align_files / `python -m bwamem_hip.mem` write for a BAM the bytes they write for the FASTQ of the same reads --
single-end and paired, with qualities, with -C and tags, in several batches, and for the aligner's own BAM output given back as input (reverse-strand records,
supplementary lines to skip, the aligner's tags to leave out)."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from test_bam_input import CASE_NAMES, _write, bam_file, bam_record, cases, refusals, split_records, stored, tag
from test_reads_input import FIX, same_read_sets
from test_reads_input_gpu import CHUNKS, _genome, _mixed_reads, _set_chunk


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


# ---------------------------------------------------------------------------------------------------------------- device = host at every window size

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_equals_host_at_every_window_size(hip, tmp_path, name):
    from bwamem_hip.aligner import bam_to_reads, read_reads_files
    from bwamem_hip.lib import reads_last_bam_counts, reads_last_counts
    records, want, counts = cases()[name]
    p = _write(tmp_path, "in.bam", bam_file(records))
    host = read_reads_files(p, comments=True, host=True)
    same_read_sets(host, want, (name, "host"))
    longest = max(len(r) for r in split_records(records))
    try:
        for chunk in CHUNKS:
            _set_chunk(chunk)
            dev = read_reads_files(p, comments=True)
            cnt, bc = reads_last_counts(), reads_last_bam_counts()
            same_read_sets(dev, host, (name, chunk))
            assert cnt["host_windows"] == 0 and cnt["device_windows"] > 0 and cnt["records"] == len(host), (name, chunk, cnt)
            assert cnt["device_inflate_members"] == 0 and cnt["host_inflate_members"] > 0, (name, chunk, cnt)      # BAM takes the host inflate
            if chunk is not None and chunk <= 257 and len(records) > 8 * longest:
                assert cnt["device_windows"] > 1, (name, chunk, cnt)                # (a window grows to a few records at the most: the file takes several)
            if counts is not None:
                assert bc == counts, (name, chunk, bc)
            same_read_sets(bam_to_reads(records, comments=True), host, (name, chunk, "records"))
            if counts is not None:
                assert reads_last_bam_counts() == counts, (name, chunk, "records")
        nc = read_reads_files(p)
        same_read_sets(nc, read_reads_files(p, host=True), (name, "no comments"))
        assert nc.comments is None
    finally:
        _set_chunk(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(refusals()))
def test_device_refusals_are_the_hosts(hip, tmp_path, name):
    from bwamem_hip.aligner import bam_to_reads, read_reads_files
    records = refusals()[name][0]
    p = _write(tmp_path, "bad.bam", bam_file(records))
    with pytest.raises(ValueError) as eh:
        read_reads_files(p, comments=True, host=True)
    with pytest.raises(ValueError) as er:
        bam_to_reads(records, comments=True, host=True)
    try:
        for chunk in (None, 257, 64):
            _set_chunk(chunk)
            with pytest.raises(ValueError) as e:
                read_reads_files(p, comments=True)
            assert str(e.value) == str(eh.value), (name, chunk)
            with pytest.raises(ValueError) as e:
                bam_to_reads(records, comments=True)
            assert str(e.value) == str(er.value), (name, chunk)
    finally:
        _set_chunk(0)


# ---------------------------------------------------------------------------------------------------------------- file -> SAM

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """a 1 Mbase genome with its index, and 3000 reads of 51 .. 251 bases single-end and as pairs: the FASTQ (comments in tag form) and the BAM of the same reads --
    every third record stored reverse-complemented, the pairs in either order, secondary and supplementary records strewn in"""
    from bwamem_hip import synth
    d = tmp_path_factory.mktemp("bam_in")
    g, prefix = _genome(d)
    out = dict(prefix=prefix, dir=d)
    for paired in (False, True):
        reads = _mixed_reads(g, 3000, paired, lengths=(51, 100, 151, 251))
        asc = [synth.codes_to_ascii(np.asarray(r)).tobytes() for r in reads]
        quals = [bytes(q) for q in synth.random_quals([len(a) for a in asc], seed=3)]
        fq, recs = [], []
        junk = [bam_record(b"junk", b"ACGTA", b"IIIII", 0x900), bam_record(b"junk", b"", None, 0x100 | 0x41)]
        for i, (a, q) in enumerate(zip(asc, quals)):
            name = b"r%d" % (i // 2 if paired else i)
            cm = b"BC:Z:%d-x y\tXQ:i:%d" % (i % 97, i % 300) if i % 3 else b""
            tags = tag(b"BC", b"Z", b"%d-x y" % (i % 97)) + tag(b"XQ", b"S" if i % 300 > 255 else b"C", i % 300) if i % 3 else tag(b"f0", b"f", 0.5) + tag(b"NM", b"C", 1)
            fq.append(b"@" + name + (b"/%d" % (1 + (i & 1)) if paired else b"") + (b" " + cm if cm else b"") + b"\n" + a + b"\n+\n" + q + b"\n")
            recs.append(stored(name, a, q, flag=(0x4D if not i & 1 else 0x8D) if paired else 4, tags=tags, rev=i % 3 == 1))
        if paired:
            recs = [x for i in range(0, len(recs), 2) for x in ((recs[i], recs[i + 1]) if (i // 2) % 2 else (recs[i + 1], junk[1], recs[i]))]
        recs = [x for i, r in enumerate(recs) for x in ((junk[0], r) if i % 50 == 7 else (r,))]
        key = "pe" if paired else "se"
        out[key + ".fq"] = _write(d, key + ".fq", b"".join(fq))
        out[key + ".bam"] = _write(d, key + ".bam", bam_file(b"".join(recs), 60000))
        out[key + ".n"] = len(reads)
    return out


def _sam(al, path, **kw):
    buf = io.BytesIO()
    n = al.align_files(path, out=buf, **kw)
    return n, buf.getvalue()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [[], ["-C"]])
def test_align_files_bam_equals_fastq(hip, world, opts):
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import reads_last_bam_counts, reads_last_counts
    al = Aligner(world["prefix"], n_threads=8)
    al.set_options(opts)
    try:
        for key, paired in (("se", False), ("pe", True)):
            n, want = _sam(al, world[key + ".fq"], paired=paired)
            assert n == world[key + ".n"] and want.count(b"\n") >= n
            n, got = _sam(al, world[key + ".bam"])                       # (pairs are found in the file: paired is not given)
            c, bc = reads_last_counts(), reads_last_bam_counts()
            assert n == world[key + ".n"] and got == want, (key, opts)
            assert c["host_windows"] == 0 and c["device_windows"] > 0 and bc["records_skipped"] > 0 and bc["tags_left_out"] == (n + 2) // 3, (key, c, bc)
            if paired:
                assert _sam(al, world[key + ".bam"], paired=True)[1] == want, (key, opts, "paired=True")
            # in at least five batches
            n, want5 = _sam(al, world[key + ".fq"], paired=paired, batch_reads=500)
            assert al.last_stats.n_batches >= 5
            n, got5 = _sam(al, world[key + ".bam"], batch_reads=500)
            assert al.last_stats.n_batches >= 5 and got5 == want5, (key, opts, "batches")
            assert reads_last_counts()["host_windows"] == 0
        with pytest.raises(ValueError, match="do not carry flag 0x1"):
            _sam(al, world["se.bam"], paired=True)
        with pytest.raises(ValueError, match="no mates file is taken beside it"):
            al.align_files(world["se.bam"], world["se.fq"], out=io.BytesIO())
    finally:
        al.close()


@pytest.mark.gpu
def test_round_trip_through_the_aligners_own_bam(hip, world):
    """FASTQ -> BAM (unsorted) -> align again: the SAM of the second run equals the SAM of the FASTQ.  The BAM holds reverse-strand records, supplementary lines
    and the aligner's own tags in front of the comment's."""
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import reads_last_bam_counts
    al = Aligner(world["prefix"], n_threads=8)
    al.set_options(["-C"])
    try:
        for key, paired in (("se", False), ("pe", True)):
            n, want = _sam(al, world[key + ".fq"], paired=paired)
            buf = io.BytesIO()
            al.align_files(world[key + ".fq"], out=buf, paired=paired, fmt="bam")
            p = _write(world["dir"], key + ".aligned.bam", buf.getvalue())
            n2, got = _sam(al, p)
            assert n2 == n and got == want, key
            flags = [int(l.split(b"\t")[1]) for l in want.split(b"\n") if l and not l.startswith(b"@")]
            assert any(f & 0x10 for f in flags) and reads_last_bam_counts()["records_skipped"] == sum(1 for f in flags if f & 0x900), key
    finally:
        al.close()


@pytest.mark.gpu
def test_mem_command_takes_a_bam(hip, world):
    from bwamem_hip.aligner import Aligner
    al = Aligner(world["prefix"])
    want = _sam(al, world["se.fq"])[1]
    al.close()
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(FIX), "..", "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    o = str(world["dir"] / "cmd.sam")
    r = subprocess.run([sys.executable, "-m", "bwamem_hip.mem", world["prefix"], world["se.bam"], "-o", o], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    with open(o, "rb") as f:
        assert f.read() == want
