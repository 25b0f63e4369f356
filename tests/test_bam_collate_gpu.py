"""Mates collated by name on the device (csrc/bam_in_kernels.hip: bcl_*): the tables of tests/test_bam_collate.py through the device form, which must give what the
host form -- the definition -- gives at every window size, refusals word for word; equal hashes forced by a narrow hash; and Aligner.align_files(collate=True) on
the aligner's own sorted BAM against a run on the name-grouped BAM of the same pairs."""
import io

import numpy as np
import pytest

from test_bam_collate import CASES, GROUPS, REFUSALS, RG_HEADER, _file, as_reads, blob, cases, check_counts, group_case, groups_through_the_file_reader, model, refusals, run_refusal
from test_bam_input import reads_of
from test_bam_sort import BamFile
from test_reads_input import bgzf
from test_reads_input_gpu import CHUNKS, _genome, _mixed_reads, _set_chunk, _write_forms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _tune(name, value):
    import ctypes as C
    from bwamem_hip.lib import load_library
    L = load_library()
    L.bmh_tune_set.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.bmh_tune_set(name, int(value or 0), 0 if value else 1)


@pytest.mark.parametrize("name", CASES)
def test_device_equals_host(hip, tmp_path, name):
    from bwamem_hip.aligner import bam_to_reads, read_reads_files
    from bwamem_hip.lib import reads_last_counts
    recs = cases()[name]
    m = model(recs)
    want = as_reads(m.reads)
    apart = m.adjacent < m.pairs
    host = bam_to_reads(blob(recs), comments=True, host=True, collate=True)
    assert reads_of(host) == want
    dev = bam_to_reads(blob(recs), comments=True, collate=True)
    assert reads_of(dev) == want, (name, "one window")
    c = check_counts(m, (name, "one window"))
    assert c["windows_to_host_for_hash_runs"] == 0
    assert np.array_equal(dev.codes, host.codes)
    path = _file(tmp_path, name, recs)
    try:
        for chunk in CHUNKS:
            _set_chunk(chunk)
            got = read_reads_files(path, comments=True, collate=True)
            assert reads_of(got) == want, (name, chunk)
            c, w = check_counts(m, (name, chunk)), reads_last_counts()
            assert w["host_windows"] == 0 and w["device_windows"] > 0 and c["windows_to_host_for_hash_runs"] == 0, (name, chunk, w, c)
            if chunk is not None and chunk <= 257 and apart:
                assert c["open_records_peak"] > 0, (name, chunk, c)
            if chunk is not None and len(blob(recs)) > 4 * chunk and m.pairs > 8:
                assert w["device_windows"] > 1, (name, chunk, w)
        _set_chunk(257)
        assert reads_of(read_reads_files(path, collate=True, comments=True, host=True)) == want
    finally:
        _set_chunk(0)


def test_device_read_groups(hip, tmp_path):
    from bwamem_hip.aligner import bam_to_reads
    recs = group_case()
    m = model(recs)
    got = bam_to_reads(blob(recs), comments=True, collate=True, read_groups=GROUPS)
    assert reads_of(got) == as_reads(m.reads)
    assert [GROUPS[g].encode() for g in got.groups] == [r.rg for r in m.reads]
    check_counts(m, "read groups")
    from bwamem_hip.lib import reads_last_counts
    for chunk in CHUNKS:
        groups_through_the_file_reader(tmp_path, False, (chunk,))
        w = reads_last_counts()
        assert w["host_windows"] == 0 and w["device_windows"] > 0, (chunk, w)


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_are_the_hosts(hip, tmp_path, name):
    for chunk in (None, 257, 64):
        want = run_refusal(name, True, tmp_path, chunk, file_only=chunk is not None)
        got = run_refusal(name, False, tmp_path, chunk, file_only=chunk is not None)
        assert got == want and len(got) >= 1, (name, chunk)


def test_forced_equal_hashes(hip, tmp_path):
    """a hash of four bits: every window holds runs of many names under one hash, and the host form decodes them -- no collision makes a wrong pair"""
    from bwamem_hip.aligner import bam_to_reads, read_reads_files
    from bwamem_hip.lib import reads_last_collate_counts, reads_last_counts
    recs = cases()["2000 pairs, random order"]
    want = as_reads(model(recs).reads)
    path = _file(tmp_path, "narrow", recs)
    try:
        _tune(b"COLLATE_HASH_BITS", 4)
        assert reads_of(bam_to_reads(blob(recs), comments=True, collate=True)) == want
        assert reads_last_collate_counts()["windows_to_host_for_hash_runs"] > 0
        for chunk in (None, 4093):
            _set_chunk(chunk)
            assert reads_of(read_reads_files(path, comments=True, collate=True)) == want, chunk
            assert reads_last_collate_counts()["windows_to_host_for_hash_runs"] > 0 and reads_last_counts()["host_windows"] > 0
        # a hash of 12 bits: most windows have no run beyond a pair, some do -- the forms alternate over one pool
        _tune(b"COLLATE_HASH_BITS", 12)
        _set_chunk(1531)
        assert reads_of(read_reads_files(path, comments=True, collate=True)) == want
        w = reads_last_counts()
        assert w["host_windows"] > 0 and w["device_windows"] > 0, w
    finally:
        _tune(b"COLLATE_HASH_BITS", 0)
        _set_chunk(0)


def test_collate_off_is_todays_refusal(hip, tmp_path):
    from bwamem_hip.aligner import bam_to_reads, read_reads_files
    recs = cases()["A1 B1 A2 B2"]
    want = r"BAM records 0 and 1 carry different names \(A and B\): is the file grouped by read name\?"
    with pytest.raises(ValueError, match=want):
        bam_to_reads(blob(recs))
    with pytest.raises(ValueError, match=want):
        read_reads_files(_file(tmp_path, "off", recs))


# ---------------------------------------------------------------------------------------------------------------- end to end

def _grouped(records: list) -> list:
    """the definition over raw records: the kept records of the pairs in the order of completion, the 0x40 record first"""
    import struct
    open_, out = {}, []
    for r in records:
        flag = struct.unpack_from("<H", r, 18)[0]
        if flag & 0x900:
            continue
        nm = r[36:36 + r[12]]
        if nm in open_:
            o = open_.pop(nm)
            assert (struct.unpack_from("<H", o, 18)[0] ^ flag) & 0xc0 == 0xc0
            out += [o, r] if flag & 0x80 else [r, o]
        else:
            open_[nm] = r
    assert not open_
    return out


@pytest.fixture(scope="module")
def e2e(hip, tmp_path_factory):
    """an aligner on the synthetic genome, about 400 pairs of mixed lengths as FASTQ"""
    from bwamem_hip.aligner import Aligner
    d = tmp_path_factory.mktemp("collate")
    g, prefix = _genome(d, 300_000)
    reads = _mixed_reads(g, 800, True)
    ff = _write_forms(d, reads, True, "c")
    ff2 = _write_forms(d, _mixed_reads(g, 240, True, lengths=(100, 150)), True, "k")        # a second read group's reads, under names of their own
    return d, prefix, ff, ff2


def _bam_pair(d, tag, sorted_bam: bytes):
    """the sorted BAM as a file, and the name-grouped BAM of the same pairs under the same header"""
    f = BamFile(sorted_bam)
    grouped = _grouped(f.recs)
    assert len(grouped) >= 700 and grouped != [r for r in f.recs if not r[19] & 0x9]
    ps, pg = str(d / (tag + ".sorted.bam")), str(d / (tag + ".grouped.bam"))
    with open(ps, "wb") as o:
        o.write(sorted_bam)
    with open(pg, "wb") as o:
        o.write(bgzf(f.data[:f.first] + b"".join(grouped), 60000))
    return ps, pg, len(grouped)


@pytest.mark.parametrize("variant", ["plain", "-C", "keep_rg", "markdup"])
def test_realign_sorted_bam(hip, e2e, variant):
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import reads_last_collate_counts, reads_last_counts
    d, prefix, ff, ff2 = e2e
    al = Aligner(prefix, n_threads=4)
    try:
        first = io.BytesIO()
        if variant == "keep_rg":
            al.align_groups([("@RG\\tID:one\\tLB:l1", ff["r1.fq"], ff["r2.fq.gz"]), ("@RG\\tID:two\\tLB:l2", ff2["fq"], None)], out=first, paired=True, fmt="bam", sort=True)
        else:
            al.align_files(ff["fq"], out=first, paired=True, fmt="bam", sort=True)
        ps, pg, n_kept = _bam_pair(d, variant, first.getvalue())
        if variant == "-C":
            al.set_options(["-C"])
        kw = dict(batch_reads=128)
        if variant == "keep_rg":
            kw.update(keep_rg=True)
        if variant == "markdup":
            kw.update(fmt="bam", sort=True, markdup=True)
        want = io.BytesIO()
        assert al.align_files(pg, out=want, **kw) == n_kept
        want_counts = dict(al.markdup_counts) if variant == "markdup" else None
        try:
            for chunk in (None, 257):
                _set_chunk(chunk)
                got = io.BytesIO()
                assert al.align_files(ps, out=got, collate=True, **kw) == n_kept
                assert got.getvalue() == want.getvalue(), (variant, chunk)
                c, w = reads_last_collate_counts(), reads_last_counts()
                assert c["pairs"] == n_kept // 2 and c["open_records_peak"] > 1 and c["windows_to_host_for_hash_runs"] == 0 and w["host_windows"] == 0 and w["device_windows"] > 0, (variant, chunk, c, w)
                if variant == "markdup":
                    assert dict(al.markdup_counts) == want_counts
        finally:
            _set_chunk(0)
        # without the option the sorted file is refused as ever
        with pytest.raises(ValueError, match="carry different names .* is the file grouped by read name"):
            al.align_files(ps, out=io.BytesIO(), **kw)
    finally:
        al.close()


def test_mem_command_collate(hip, e2e):
    """the command realigns the program's own sorted output: --collate --sort --markdup writes what align_files(collate=True, ...) writes"""
    import os
    import subprocess
    import sys
    from bwamem_hip.aligner import Aligner
    from test_reads_input import FIX
    d, prefix, ff, _ff2 = e2e
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(FIX), "..", "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def mem(*args):
        return subprocess.run([sys.executable, "-m", "bwamem_hip.mem", *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    al = Aligner(prefix, n_threads=4)
    try:
        first = io.BytesIO()
        al.align_files(ff["fq"], out=first, paired=True, fmt="bam", sort=True)
        ps = str(d / "cmd.sorted.bam")
        with open(ps, "wb") as f:
            f.write(first.getvalue())
        want, want_idx = io.BytesIO(), io.BytesIO()
        al.align_files(ps, out=want, collate=True, fmt="bam", sort=True, markdup=True, index=want_idx)
    finally:
        al.close()
    o = str(d / "cmd.out.bam")
    r = mem("--collate", "--sort", "--markdup", prefix, ps, "-o", o)
    assert r.returncode == 0, r.stderr.decode()
    with open(o, "rb") as f:
        assert f.read() == want.getvalue() and len(want.getvalue()) > 10_000
    with open(o + ".bai", "rb") as f:
        assert f.read() == want_idx.getvalue()
    r = mem("--collate-mem", "1024", prefix, ps)
    assert r.returncode == 2 and b"--collate-mem needs --collate" in r.stderr
    o2 = str(d / "cmd.text.sam")
    r = mem("--collate", "-p", prefix, ff["fq"], "-o", o2)
    assert r.returncode == 1 and b"in BAM input only" in r.stderr and os.path.getsize(o2) == 0
    r = mem("--collate", "--collate-mem", "600", prefix, ps, "-o", o2)
    assert r.returncode == 1 and b"--collate-mem 600 bytes" in r.stderr            # (one record of a 600 bp read is more)


def test_two_groups_refused_through_align_files(hip, e2e, monkeypatch):
    """align_files(keep_rg=True, collate=True) on the two-group case with thirty pairs in front of the record that closes it, in batches of one pair, so that the
    first record waits in the pool when its partner comes: the device form's refusal is the host form's (BMH_READS_HOST), word for word, at every window size.
    (A window that holds a pair of two groups is the host form's, so without small windows the device form delivers none here.)"""
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import reads_last_counts
    d, prefix, _ff, _ff2 = e2e
    from test_bam_collate import _pair
    recs, _frags, _kw, _partial = refusals()["a pair of two read groups"]
    rng = np.random.default_rng(31)
    recs = recs[:3] + [r for k in range(30) for r in _pair(rng, b"between%d" % k, rg=b"lane2")] + recs[3:]
    frags = ["BAM records 0 and 63 (G) name different read groups (lane1 and lane2)"]
    path = _file(d, "two groups", recs, header_text=RG_HEADER)
    al = Aligner(prefix, n_threads=4)
    try:
        for chunk in (None, 257, 64):
            _set_chunk(chunk)
            msgs = []
            for host in (False, True):
                if host:
                    monkeypatch.setenv("BMH_READS_HOST", "1")
                try:
                    with pytest.raises(ValueError) as ei:
                        al.align_files(path, out=io.BytesIO(), keep_rg=True, collate=True, batch_reads=2)
                finally:
                    monkeypatch.delenv("BMH_READS_HOST", raising=False)
                msgs.append(str(ei.value))
                w = reads_last_counts()
                assert w["device_windows"] == 0 if host else (chunk is None or w["device_windows"] > 0), (chunk, host, w)
            assert msgs[0] == msgs[1] and all(f in msgs[0] for f in frags), (chunk, msgs)
    finally:
        _set_chunk(0)
        al.close()
