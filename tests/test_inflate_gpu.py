"""The device inflate (csrc/inflate_kernels.hip) and the read-file path above it: the corpus and the damaged members of test_inflate.py through the kernel give
zlib's text and the host decoder's statuses at every launch size; read_reads_files and align_files on BGZF input inflate on the device (the counter says so)
and give the read sets and the SAM text of the same reads as a plain file; BMH_INFLATE_HOST=1 keeps the host inflate; the refusals read as before."""
import io
import json
import os
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

from test_inflate import OK, corpus, damaged, handmade, synthetic_fastq, zlib_verdict
from test_reads_input import FIX, FIXTURES, bgzf, check_expected, fixture_text, gzip_member, same_read_sets
from test_reads_input_gpu import _genome, _mixed_reads, _write_forms


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _tune(name: bytes, value):
    """bmh_tune_set: what BMH_<name> in the environment would give this process; None clears it"""
    import ctypes as C
    from bwamem_hip.lib import load_library
    L = load_library()
    L.bmh_tune_set.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.bmh_tune_set(name, int(value or 0), 1 if value is None else 0)


@pytest.fixture
def device_inflate(hip):
    """BMH_INFLATE_DEVICE=1 for one test: BGZF read files inflate on the device (opt-in)"""
    _tune(b"INFLATE_DEVICE", 1)
    yield
    _tune(b"INFLATE_DEVICE", None)


def _table(cases):
    """cases: (data, isize, crc32) -> the bytes back to back (a gap between them) and their member table"""
    from bwamem_hip.lib import INFLATE_MEMBER
    tab = np.zeros(len(cases), INFLATE_MEMBER)
    blob, text = bytearray(), 0
    for i, (data, isize, crc) in enumerate(cases):
        blob += b"\xff\xff\xff"
        tab[i] = (len(blob), text, len(data), isize, crc & 0xFFFFFFFF, 0)
        blob += data
        text += min(isize, 65536)
    return bytes(blob), tab, text


@pytest.mark.gpu
def test_corpus_on_the_device(hip):
    from bwamem_hip.lib import inflate_members
    members = corpus()
    blob, tab, nbytes = _table([(data, len(text), zlib.crc32(text)) for _, text, data in members])
    want = b"".join(text for _, text, _ in members)
    assert want == b"".join(zlib.decompress(d, -15) for _, _, d in members)
    host, host_st = inflate_members(blob, tab, nbytes, host=True)
    assert not host_st.any() and host.tobytes() == want
    for per_launch in (0, 65, 2, 1):
        out, st = inflate_members(blob, tab, nbytes, per_launch=per_launch)
        bad = [(members[i][0], int(st[i])) for i in np.nonzero(st)[0]]
        assert not bad, (per_launch, bad[:10])
        assert out.tobytes() == want, per_launch


@pytest.mark.gpu
def test_damaged_members_on_the_device(hip):
    """the statuses of the host decoder (which test_inflate.py runs on these members under the sanitizers), and zlib's text where zlib takes the member"""
    from bwamem_hip.lib import inflate_members
    hand = [(n, d, isize, crc) for n, d, isize, crc, _ in handmade()]
    cases = hand + damaged(corpus(), 4000, seed=3)
    blob, tab, nbytes = _table([(d, isize, crc) for _, d, isize, crc in cases])
    host, host_st = inflate_members(blob, tab, nbytes, host=True)
    out, st = inflate_members(blob, tab, nbytes)
    diff = [(cases[i][0], int(st[i]), int(host_st[i])) for i in np.nonzero(st != host_st)[0]]
    assert not diff, diff[:10]
    for (_, want), (name, _, _, _), s in zip(handmade_status(), hand, st):
        assert s == want, (name, s, want)
    for i, (name, d, isize, crc) in enumerate(cases):
        text = zlib_verdict(d, isize, crc)
        assert (st[i] == OK) == (text is not None), name
        if text is not None:
            o = int(tab["out_off"][i])
            assert out[o:o + isize].tobytes() == text, name
    # a table that points outside the buffers is refused member by member
    bad = tab[:4].copy(); bad["in_off"][0] = len(blob) + 1; bad["out_off"][1] = nbytes + 1; bad["in_len"][2] = 1 << 31
    _, st = inflate_members(blob, bad, nbytes)
    assert list(st[:3]) == [9, 9, 9] and st[3] == host_st[3]


@pytest.mark.gpu
def test_limit_members_on_the_device(hip):
    """the members of tests/inflate_limits.py, host and device, at every launch size: OK exactly where zlib takes the member, with zlib's text"""
    import inflate_limits
    from bwamem_hip.lib import inflate_members
    cases = inflate_limits.members()
    blob, tab, nbytes = _table([(d, isize, crc) for _, d, isize, crc, _ in cases])
    want = [zlib_verdict(d, isize, crc) for _, d, isize, crc, _ in cases]
    runs = [("host", inflate_members(blob, tab, nbytes, host=True))] + [(per_launch, inflate_members(blob, tab, nbytes, per_launch=per_launch)) for per_launch in (0, 65, 2, 1)]
    for how, (out, st) in runs:
        for i, (name, d, isize, crc, status) in enumerate(cases):
            assert st[i] == status and (st[i] == OK) == (want[i] is not None), (how, name, int(st[i]), status)
            if want[i] is not None:
                o = int(tab["out_off"][i])
                assert out[o:o + isize].tobytes() == want[i], (how, name)


def handmade_status():
    return [(n, want) for n, _, _, _, want in handmade()]


@pytest.mark.gpu
def test_inflate_bgzf_on_the_device(hip):
    from bwamem_hip.lib import inflate_bgzf
    fq = synthetic_fastq(4 << 20, 9)
    for block in (777, 60000, 65280):
        assert inflate_bgzf(bgzf(fq, block)) == fq
    z = bytearray(bgzf(fq[:200000], 60000)); z[len(z) // 2] ^= 0x10
    with pytest.raises(ValueError, match=r"damaged BGZF member 1 \("):
        inflate_bgzf(bytes(z))


# ---------------------------------------------------------------------------------------------------------------- read files

def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
from bwamem_hip.aligner import read_reads_files
from bwamem_hip.lib import reads_last_counts
import numpy as np
out = {{}}
for p in {files!r}:
    rs = read_reads_files(p, comments=True)
    out[p] = dict(counts=reads_last_counts(), lens=rs.lens.tolist(), ascii=bytes(rs.ascii).hex(), names=bytes(rs.name_blob).hex(), comments=bytes(rs.comments[0]).hex(),
                  qual=None if rs.qual is None else bytes(rs.qual).hex())
print(json.dumps(out))
"""


@pytest.mark.gpu
def test_read_files_inflate_on_the_device(hip, tmp_path, device_inflate):
    """every fixture as BGZF with small and with large members: the device inflates (counter), the read sets are the host walker's and the reference's"""
    from bwamem_hip.aligner import read_reads_files
    from bwamem_hip.lib import reads_last_counts
    expected = np.load(os.path.join(FIX, "expected.npz"))
    files = []
    for name in FIXTURES:
        text = fixture_text(name)
        host = read_reads_files(os.path.join(FIX, name), comments=True, host=True)
        for block in (777, 60000):
            p = _write(tmp_path, f"{name}.{block}.bgzf", bgzf(text, block))
            files.append(p)
            dev = read_reads_files(p, comments=True)
            cnt = reads_last_counts()
            assert cnt["device_inflate_members"] == -(-len(text) // block) + 1 and cnt["host_inflate_members"] == 0, (name, block, cnt)
            assert cnt["text_bytes"] == len(text), (name, block, cnt)
            check_expected(expected, name, dev)
            same_read_sets(dev, host, (name, block))
            # the host walker inflates on the host
            same_read_sets(read_reads_files(p, comments=True, host=True), host, (name, block, "host"))
            cnt = reads_last_counts()
            assert cnt["device_inflate_members"] == 0 and cnt["host_inflate_members"] > 0, (name, block, cnt)
    # in fresh processes: BMH_INFLATE_DEVICE=1 in the environment inflates on the device; BMH_INFLATE_HOST=1 beside it, and no switch at all, keep the host
    # inflate; the read sets are the same
    code = _CHILD.format(paths=[p for p in sys.path if p], files=files)
    base = {k: v for k, v in os.environ.items() if k not in ("BMH_INFLATE_DEVICE", "BMH_INFLATE_HOST")}
    for extra, on_device in ((dict(BMH_INFLATE_DEVICE="1"), True), (dict(BMH_INFLATE_DEVICE="1", BMH_INFLATE_HOST="1"), False), ({}, False)):
        r = subprocess.run([sys.executable, "-c", code], env=dict(base, **extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        got = json.loads(r.stdout)
        _check_child(got, files, on_device, extra)


def _check_child(got, files, on_device, extra):
    from bwamem_hip.aligner import read_reads_files
    for p in files:
        g = got[p]
        assert (g["counts"]["device_inflate_members"] > 0) == on_device and (g["counts"]["host_inflate_members"] > 0) != on_device, (p, extra, g["counts"])
        rs = read_reads_files(p, comments=True)
        assert g["lens"] == rs.lens.tolist() and g["ascii"] == bytes(rs.ascii).hex() and g["names"] == bytes(rs.name_blob).hex(), p
        assert g["comments"] == bytes(rs.comments[0]).hex() and g["qual"] == (None if rs.qual is None else bytes(rs.qual).hex()), p


@pytest.mark.gpu
def test_read_files_two_files_and_windows(hip, tmp_path, device_inflate):
    """R1 / R2 with one file BGZF and the other plain, gzip or BGZF, at window sizes that members and records straddle; a pipe"""
    import ctypes as C
    from bwamem_hip.aligner import read_reads_files
    from bwamem_hip.lib import load_library, reads_last_counts
    expected = np.load(os.path.join(FIX, "expected.npz"))
    L = load_library()
    L.bmh_tune_set.argtypes = [C.c_char_p, C.c_int, C.c_int]
    t1, t2 = fixture_text("r1.fq"), fixture_text("r2.fq")
    f1 = {"plain": _write(tmp_path, "r1.fq", t1), "gz": _write(tmp_path, "r1.gz", gzip_member(t1)), "bgzf": _write(tmp_path, "r1.bgzf", bgzf(t1, 333))}
    f2 = {"plain": _write(tmp_path, "r2.fq", t2), "gz": _write(tmp_path, "r2.gz", gzip_member(t2)), "bgzf": _write(tmp_path, "r2.bgzf", bgzf(t2, 777))}
    try:
        for chunk in (None, 4093, 1000, 257, 64):
            L.bmh_tune_set(b"READS_CHUNK_BYTES", int(chunk or 0), 0 if chunk else 1)
            for a, b in (("bgzf", "bgzf"), ("bgzf", "plain"), ("gz", "bgzf"), ("plain", "bgzf")):
                check_expected(expected, "r1.fq+r2.fq", read_reads_files(f1[a], f2[b], comments=True))
                cnt = reads_last_counts()
                assert cnt["device_inflate_members"] > 0 and cnt["host_inflate_members"] == 0 and cnt["host_windows"] == 0, (chunk, a, b, cnt)
            for name in ("ml60.fa", "four.fq", "ml.fq"):
                p = _write(tmp_path, name + ".bgzf", bgzf(fixture_text(name), 500))
                check_expected(expected, name, read_reads_files(p, comments=True))
                assert reads_last_counts()["device_inflate_members"] > 0
    finally:
        L.bmh_tune_set(b"READS_CHUNK_BYTES", 0, 1)
    for name in ("ml60.fa", "four.fq"):
        fifo = str(tmp_path / "fifo")
        os.mkfifo(fifo)
        data = bgzf(fixture_text(name), 400)

        def feed():
            with open(fifo, "wb") as f:
                for k in range(0, len(data), 1000):
                    f.write(data[k:k + 1000]); f.flush()
        t = threading.Thread(target=feed)
        t.start()
        try:
            check_expected(expected, name, read_reads_files(fifo, comments=True))
            assert reads_last_counts()["device_inflate_members"] > 0
        finally:
            t.join()
            os.unlink(fifo)


@pytest.mark.gpu
def test_read_files_refusals(hip, tmp_path, device_inflate):
    from bwamem_hip.aligner import read_reads_files
    fq = synthetic_fastq(400_000, 2)
    z = bgzf(fq, 60000)
    bad = bytearray(z); bad[len(z) // 2] ^= 0x40
    with pytest.raises(ValueError, match=r"flip\.bgzf: damaged BGZF member \(inflate, length or CRC\)"):
        read_reads_files(_write(tmp_path, "flip.bgzf", bytes(bad)))
    with pytest.raises(ValueError, match=r"cut\.bgzf: the gzip stream is truncated"):
        read_reads_files(_write(tmp_path, "cut.bgzf", z[:len(z) // 2 + 5]))
    with pytest.raises(ValueError, match=r"mixed\.bgzf: a gzip member without the BGZF size field behind BGZF members"):
        read_reads_files(_write(tmp_path, "mixed.bgzf", bgzf(fq[:100_000], 60000)[:-28] + gzip_member(fq[100_000:])))
    # a damaged end-of-file member (no text) is refused too
    eof = bytearray(z); eof[-10] ^= 1
    with pytest.raises(ValueError, match="damaged BGZF member"):
        read_reads_files(_write(tmp_path, "eof.bgzf", bytes(eof)))


# ---------------------------------------------------------------------------------------------------------------- file -> SAM

@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_align_files_bgzf_equals_plain(hip, tmp_path, paired, device_inflate):
    """BGZF in, in every arrangement: the SAM text of the same reads as a plain file"""
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import reads_last_counts
    g, prefix = _genome(tmp_path)
    reads = _mixed_reads(g, 12_000, paired)
    ff = _write_forms(tmp_path, reads, paired, "z")
    with open(ff["fq"], "rb") as f:
        whole = f.read()
    small = _write(tmp_path, "small.bgzf", bgzf(whole, 777))
    for opts in ([], ["-C"]):
        al = Aligner(prefix, n_threads=8)
        al.set_options(opts)

        def run(p, q=None, chunk=700_001, device=True, pair=paired):
            buf = io.BytesIO(); n = al.align_files(p, q, out=buf, paired=pair, chunk_bases=chunk)
            assert n == len(reads)
            c = reads_last_counts()
            assert c["host_windows"] == 0 and c["host_inflate_members"] == 0 and (c["device_inflate_members"] > 0) == device, c
            return buf.getvalue()
        want = run(ff["fq"], device=False)
        assert want.count(b"\n") >= len(reads)
        if paired:
            assert run(ff["r1.bgzf"], ff["r2.bgzf"]) == want, ("R1 / R2 BGZF", opts)
            assert run(ff["r1.bgzf"], ff["r2.fq.gz"]) == want, ("BGZF beside plain gzip", opts)
            assert run(ff["r1.fq"], ff["r2.bgzf"]) == want, ("plain beside BGZF", opts)
        else:
            assert run(ff["fq.bgzf"]) == want, ("BGZF", opts)
        assert run(small) == want, ("interleaved BGZF, small members", opts)
        # small batches: the windows shrink to a batch's text, and members, records and windows straddle each other
        want_small = run(ff["fq"], chunk=30_011, device=False)
        assert run(small, chunk=30_011) == want_small, ("small windows", opts)
        if not opts:
            fifo = str(tmp_path / "fifo")
            os.mkfifo(fifo)
            with open(small, "rb") as f:
                data = f.read()

            def feed():
                with open(fifo, "wb") as f:
                    f.write(data)
            t = threading.Thread(target=feed)
            t.start()
            try:
                assert run(fifo) == want, "from a pipe"
            finally:
                t.join()
                os.unlink(fifo)
        al.close()


@pytest.mark.gpu
def test_align_files_bgzf_long_reads(hip, tmp_path, device_inflate):
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import reads_last_counts
    g, prefix = _genome(tmp_path)
    rng = np.random.default_rng(9)
    reads = []
    for i in range(60):
        ln = int(rng.integers(2000, 4001)); p0 = int(rng.integers(0, len(g) - ln))
        x = g[p0:p0 + ln].copy()
        q = rng.random(ln) < 0.01; x[q] = (x[q] + 1) & 3
        reads.append(x)
    ff = _write_forms(tmp_path, reads, False, "long")
    al = Aligner(prefix, n_threads=8, long_reads=True)
    buf = io.BytesIO(); al.align_files(ff["fq"], out=buf, chunk_bases=60_000); want = buf.getvalue()
    buf = io.BytesIO(); al.align_files(ff["fq.bgzf"], out=buf, chunk_bases=60_000)
    assert buf.getvalue() == want and reads_last_counts()["device_inflate_members"] > 0
    al.close()


@pytest.mark.gpu
def test_align_files_refusals_keep_the_batches_before(hip, tmp_path, device_inflate):
    from bwamem_hip.aligner import Aligner
    g, prefix = _genome(tmp_path)
    reads = _mixed_reads(g, 12_000, False, lengths=(100, 150))
    ff = _write_forms(tmp_path, reads, False, "d")
    with open(ff["fq"], "rb") as f:
        whole = f.read()
    z = bgzf(whole, 60000)
    al = Aligner(prefix, n_threads=8)
    buf = io.BytesIO(); al.align_files(ff["fq"], out=buf, chunk_bases=100_000); want = buf.getvalue()

    def names(sam):
        return [l.split(b"\t")[0] for l in sam.split(b"\n") if l and not l.startswith(b"@")]
    bad = bytearray(z); bad[len(z) * 3 // 4] ^= 0x08
    cases = ((bytes(bad), r"flip\.bgzf: damaged BGZF member \(inflate, length or CRC\)", "flip.bgzf"),
             (z[:len(z) * 3 // 4], r"cut\.bgzf: the gzip stream is truncated", "cut.bgzf"),
             (bgzf(whole[:len(whole) * 3 // 4], 60000)[:-28] + gzip_member(whole[len(whole) * 3 // 4:]), r"mixed\.bgzf: a gzip member without the BGZF size field behind BGZF members", "mixed.bgzf"))
    for data, msg, fname in cases:
        buf = io.BytesIO()
        with pytest.raises(ValueError, match=msg):
            al.align_files(_write(tmp_path, fname, data), out=buf, chunk_bases=100_000)
        got = buf.getvalue()
        n = len(set(names(got)))
        # the batches before the damage are written, and they are the text of the undamaged file
        assert 1000 < n < len(reads), (fname, n)
        assert want.startswith(got), fname
    al.close()
