"""`bwa index` on the device (bmh_index_fasta, bwamem_hip.index_fasta): FASTA / .fa.gz in, the five index files out, byte for byte
what the reference's two-pass CLI writes (fixtures recorded by scripts/record_fasta_index.py under tests/golden/fasta_index/).
The numpy restatement of the packer (tests/fasta_pack_numpy.py) is checked against the fixtures and glibc on the CPU, and the
device's packer against it."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import common
import fasta_pack_numpy as FP

FIX = os.path.join(common.GOLDEN, "fasta_index")
EXTS = (".bwt", ".sa", ".pac", ".ann", ".amb")
RECORDED = [("mixed", 16), ("crlf", 16), ("repeats", 16), ("repeats", 32)]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


# ---------------------------------------------------------------- CPU

@pytest.mark.parametrize("name,r", RECORDED + [("crlf.fa.gz", 16)])
def test_host_restatement_reproduces_the_recorded_files(name, r):
    src = name if name.endswith(".gz") else name + ".fa"
    stem = name.split(".")[0]
    got = FP.pack_fasta(_read(os.path.join(FIX, src)))
    for ext in (".pac", ".ann", ".amb"):
        assert got["files"][ext] == _read(os.path.join(FIX, f"{stem}_r{r}{ext}")), (name, ext)


def test_issue_probe_tables():
    """the probe of the issue: empty records, CR rules, ' ' and '\\t' as sequence"""
    got = FP.pack_fasta(b">e1\n>e2 c\r\n\r\nACGT\r\nNN\n>e3\nAC GT\tAc")
    assert got["names"] == [b"e1", b"e2", b"e3"] and list(got["lens"]) == [0, 7, 8] and got["comments"][1] == b"c"
    assert list(zip(got["hole_off"], got["hole_len"], got["hole_char"])) == [(0, 1, 13), (5, 2, 78), (9, 1, 32), (12, 1, 9)]


def test_lrand48_jump_ahead_equals_glibc():
    libc = C.CDLL(ctypes.util.find_library("c"))
    libc.lrand48.restype = C.c_long
    libc.srand48(C.c_long(11))
    n = 1_000_000
    want = np.array([libc.lrand48() for _ in range(n)], dtype=np.int64)
    assert np.array_equal(FP.lrand48_first(n), want)
    ks = np.array([0, 1, 2, 999_999, 123_456], dtype=np.uint64)
    assert np.array_equal(FP.lrand48_at(ks), want[ks.astype(np.int64)])
    # far beyond 2^32: the jump equals the closed form, and glibc's nrand48 carries on from the jumped state as the jump does
    libc.nrand48.restype = C.c_long
    libc.nrand48.argtypes = [C.POINTER(C.c_ushort * 3)]
    for k in (2 ** 32 - 1, 2 ** 32 + 7, 5_000_000_017, 2 ** 40 + 3, 2 ** 47 + 11):
        assert int(FP.lrand48_at(np.array([k], np.uint64))[0]) == FP.lrand48_closed_form(k), k
        x = int(FP.lrand48_states_at(np.array([k], np.uint64))[0])
        xs = (C.c_ushort * 3)(x & 0xFFFF, (x >> 16) & 0xFFFF, (x >> 32) & 0xFFFF)
        nxt = [libc.nrand48(C.byref(xs)) for _ in range(5)]
        assert nxt == list(FP.lrand48_at(np.arange(k + 1, k + 6, dtype=np.uint64))), k


def test_c_entry_points_return_enodev_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from bwamem_hip.index import FastaPacked, IndexFastaStats, _lib
    L = _lib()
    fa = os.path.join(FIX, "mixed.fa").encode()
    assert L.bmh_index_fasta(fa, b"/nonexistent/x", 16, 0, 0, C.byref(IndexFastaStats())) == -1
    assert L.bmh_fasta_pack(fa, 0, C.byref(FastaPacked()), None) == -1


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _same_files(prefix, want_prefix):
    return [ext for ext in EXTS if _read(prefix + ext) != _read(want_prefix + ext)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,r", RECORDED)
@pytest.mark.parametrize("chunk", [None, 4093, 64])
def test_index_fasta_writes_the_recorded_files(hip, tmp_path, name, r, chunk):
    if chunk == 64 and name == "repeats":
        chunk = 1531
    p = str(tmp_path / "ix")
    st = hip.index_fasta(os.path.join(FIX, name + ".fa"), p, sa_intv=r, verify=True, chunk_bytes=chunk)
    assert st["verified"] == 1
    assert _same_files(p, os.path.join(FIX, f"{name}_r{r}")) == []


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1000])
def test_index_fasta_from_gzip(hip, tmp_path, chunk):
    p = str(tmp_path / "ix")
    hip.index_fasta(os.path.join(FIX, "crlf.fa.gz"), p, chunk_bytes=chunk)
    assert _same_files(p, os.path.join(FIX, "crlf_r16")) == []


@pytest.mark.gpu
def test_index_fasta_cli(hip, tmp_path):
    from bwamem_hip import index as IX
    p = str(tmp_path / "cli")
    assert IX.main(["-p", p, "-r", "32", os.path.join(FIX, "repeats.fa")]) == 0
    assert _same_files(p, os.path.join(FIX, "repeats_r32")) == []


def _hg38_like_fasta(path, n_bases, device):
    """make_genome_device's genome as a multi-contig FASTA with 'N' in its holes; mixed line widths"""
    from bwamem_hip import synth
    g, meta = synth.make_genome_device(n_bases, device, seed=3, return_meta=True)
    asc = synth.codes_to_ascii(g.cpu().numpy()).copy()
    for a, b in meta["holes"]:
        asc[a:b] = ord("N")
    with open(path, "wb") as f:
        off = 0
        for i, (name, ln) in enumerate(meta["contigs"]):
            w = (60, 70, 80)[i % 3]
            s = asc[off:off + ln]
            f.write(b">%s AC:CM0006%02d.2 hg38-like\n" % (name.encode(), i))
            body = s[: (ln // w) * w].reshape(-1, w)
            f.write(np.concatenate([body, np.full((body.shape[0], 1), 10, np.uint8)], axis=1).tobytes())
            if ln % w:
                f.write(s[(ln // w) * w:].tobytes() + b"\n")
            off += ln
    return meta


@pytest.mark.gpu
def test_packer_equals_host_restatement_on_hg38_like_genome(hip, tmp_path):
    fa = str(tmp_path / "hg.fa")
    meta = _hg38_like_fasta(fa, 50_000_000, "cuda:0")
    want = FP.pack_fasta(_read(fa))
    got = hip.fasta_pack(fa, chunk_bytes=8 << 20)
    assert got["l_pac"] == want["l_pac"] == sum(c[1] for c in meta["contigs"])
    assert got["n_ambig"] == want["n_ambig"] > 0
    assert np.array_equal(got["pac"], want["pac"])
    assert [s.encode("latin-1") for s in got["names"]] == want["names"]
    assert [s.encode("latin-1") for s in got["comments"]] == want["comments"]
    for k in ("offsets", "lens", "n_ambs", "hole_off", "hole_len", "hole_char"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.gpu
def test_n_free_genome_equals_the_existing_path(hip, tmp_path):
    import torch
    from bwamem_hip import fmindex as F, synth
    g = synth.make_genome(300_007, seed=9)
    contigs = [("c1", 100_000), ("c2", 1), ("c3", 150_000), ("c4", 50_006)]
    fa = str(tmp_path / "nf.fa")
    asc = synth.codes_to_ascii(g)
    with open(fa, "wb") as f:
        off = 0
        for name, ln in contigs:
            f.write(b">" + name.encode() + b"\n")
            for i in range(off, off + ln, 60):
                f.write(asc[i:min(i + 60, off + ln)].tobytes() + b"\n")
            off += ln
    p_new, p_old = str(tmp_path / "new"), str(tmp_path / "old")
    hip.index_fasta(fa, p_new)
    pac = F.pack_pac_device(torch.from_numpy(g).cuda())
    d = F.build_fmd_index_device(pac, len(g), sa_intv=16)
    F.write_index(p_old, F.device_index_to_host(d, 16))
    F.write_bns(p_old, g, contigs=contigs)
    assert _same_files(p_new, p_old) == []


@pytest.mark.gpu
@pytest.mark.parametrize("data", [b"ACGT\nACGT\n", b">r1\nACGT\n+\nIIII\n", b"", b">a\n>b desc\n\n", b">a\nAC\x80GT\n"],
                         ids=["no_record", "plus_line", "empty_file", "all_empty", "high_byte"])
def test_malformed_inputs_fail_and_leave_no_files(hip, tmp_path, data):
    fa = tmp_path / "bad.fa"
    fa.write_bytes(data)
    p = str(tmp_path / "out")
    with pytest.raises(ValueError):
        hip.index_fasta(str(fa), p)
    assert sorted(os.listdir(tmp_path)) == ["bad.fa"]


@pytest.mark.gpu
def test_sa_interval_must_be_a_power_of_two(hip, tmp_path):
    with pytest.raises(ValueError):
        hip.index_fasta(os.path.join(FIX, "crlf.fa"), str(tmp_path / "x"), sa_intv=10)
    assert os.listdir(tmp_path) == []


@pytest.mark.gpu
def test_aligner_on_a_fresh_index_equals_the_recorded_one(hip, tmp_path):
    """Aligner(prefix) on the files just built from repeats.fa (5 contigs, N runs) writes the SAM it writes on the recorded files;
    reads drawn beside the holes map to their contigs and positions"""
    from bwamem_hip.aligner import Aligner
    p = str(tmp_path / "rep")
    hip.index_fasta(os.path.join(FIX, "repeats.fa"), p)
    host = FP.pack_fasta(_read(os.path.join(FIX, "repeats.fa")))
    text = host["text"]
    amb = FP.NT4[text] >= 4
    rng = np.random.default_rng(1)
    L = 120
    names, seqs, truth = [], [], []
    for o, ln in zip(host["hole_off"], host["hole_len"]):
        for start in (int(o) - L - int(rng.integers(0, 40)), int(o + ln) + int(rng.integers(0, 40))):
            if start < 0 or start + L > len(text) or amb[start:start + L].any():
                continue
            ci = int(np.searchsorted(host["offsets"] + host["lens"], start, side="right"))
            if start + L > host["offsets"][ci] + host["lens"][ci]:
                continue
            names.append(f"r{len(names)}")
            seqs.append(text[start:start + L].tobytes().decode().upper())
            truth.append((host["names"][ci].decode(), start - int(host["offsets"][ci]) + 1))
    assert len(names) >= 10
    sam_new = Aligner(p, n_threads=2).align_batch(names, seqs)
    sam_old = Aligner(os.path.join(FIX, "repeats_r16"), n_threads=2).align_batch(names, seqs)
    assert sam_new == sam_old
    recs = [ln.split("\t") for ln in sam_new.splitlines() if ln and not ln.startswith("@")]
    prim = {r[0]: (r[2], int(r[3])) for r in recs if not int(r[1]) & 0x900}
    hits = sum(prim[f"r{i}"] == t for i, t in enumerate(truth))
    assert hits >= 0.9 * len(truth), (hits, len(truth))
