"""CPU tests of the one SAM record writer (csrc/sam_core.h): the core as plain C++ over a trivial array-backed source (tests/sam_core_host.cpp, also under the
sanitizers as a program of its own), on a hand-made table of records whose lines are written out in tests/sam_table.py, against those lines and against the
library's host formatter (bmh_format_sam[_pe][_ex]: fixed CIGAR slots; bmh_format_sam_parts over the packed words through tests/sam_parts_host.cpp); the
selection bmh_sam_need_cigar[_pe] against the one the table implies; and the host's pa:f tag against printf."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sam_table
from bwamem_hip.lib import _err, _i32p, _np_ptr, _u32p, _u8p, load_library

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")


def _stale(out, src):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in src)


def core_exe(tag, flags):
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sam_core_host_" + tag)
    src = [os.path.join(HERE, "sam_core_host.cpp"), os.path.join(CSRC, "sam_core.h")]
    if _stale(exe, src):
        subprocess.check_call(["g++", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer"] + flags + [src[0], "-o", exe])
    return exe


def parts_lib():
    """bmh_format_sam_parts (internal: the native pipeline's host formatter) over packed words and 32-bit slots, behind a C function"""
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "sam_parts_host.so")
    pkg = os.path.abspath(os.path.join(HERE, "..", "bwa-mem_gpu_amd"))
    src = [os.path.join(HERE, "sam_parts_host.cpp"), os.path.join(CSRC, "bmh_internal.h"), os.path.join(pkg, "libbwamem_hip.so")]
    if _stale(so, src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-std=c++17", "-shared", "-fPIC", src[0], "-o", so, "-L" + pkg, "-lbwamem_hip", "-Wl,-rpath,$ORIGIN/../../bwa-mem_gpu_amd"])
    load_library()
    lib = C.CDLL(so)
    lib.sam_parts_packed.restype = C.c_void_p
    return lib


def packed_text(lib, T, po, with_quals, with_comments) -> bytes:
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    nb, no = T.blob(T.names); cb, co = T.blob(T.comments)
    cn = (C.c_char_p * len(T.contigs))(*[c[0].encode() for c in T.contigs])
    coff = np.concatenate([[0], np.cumsum([c[1] for c in T.contigs])[:-1]]).astype(np.int64)
    keep = [nb, no, T.codes, T.offs, T.lens, T.quals, cb, co, coff, T.fin, T.fpr, T.h_rec, T.unflag, T.slot.astype(np.int32), T.aln, T.cig_off, T.packed]
    k = [p(a) for a in keep]
    ln = C.c_size_t()
    r = lib.sam_parts_packed(C.byref(po), C.c_uint32(T.n), k[0], k[1], k[2], k[3], k[4], k[5] if with_quals else None, k[6] if with_comments else None,
                             k[7] if with_comments else None, len(T.contigs), cn, k[8], k[9], k[10], k[11] if T.paired else None, k[12] if T.paired else None,
                             k[13], k[14], k[15], k[16], C.byref(ln))
    assert r, _err(load_library())
    raw = C.string_at(r, ln.value)
    load_library().bmh_free(C.c_void_p(r))
    return raw


@pytest.mark.parametrize("case", list(sam_table.CASES))
def test_record_table_core_equals_lines_and_host_formatter(tmp_path, case):
    reads, lines, opts, paired = sam_table.CASES[case]
    T = sam_table.Table(reads, flag_all=bool(opts.get("flag_all")), paired=paired)
    want = ("\n".join(lines) + "\n").encode()
    tags = "copy_comment" in opts
    tab = str(tmp_path / "table.bin")
    T.write(tab, opts, with_quals=tags)
    # the core: for every read the counted length equals the bytes written (the program checks it and allocates exactly the count), and the text is the lines
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    for tag, flags in (("plain", ["-O2"]), ("asan", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        r = subprocess.run([core_exe(tag, flags), tab], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        err = r.stderr.decode(errors="replace")
        assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (tag, r.returncode, err[-3000:])
        assert r.stdout == want, (tag, [(a, b) for a, b in zip(r.stdout.split(b"\n"), want.split(b"\n")) if a != b][:2])
    # the library's host formatter on the same table, fixed CIGAR slots and packed words
    po = sam_table.post_opt(opts)
    assert T.host_text(po, with_quals=tags, with_comments=tags) == want
    assert packed_text(parts_lib(), T, po, tags, tags) == want
    # the selection
    L = load_library()
    need = np.zeros(max(len(T.fin), 1), np.uint8)
    fin, fpr = np.ascontiguousarray(T.fin), np.ascontiguousarray(T.fpr)
    if paired:
        k = L.bmh_sam_need_cigar_pe(C.byref(po), _np_ptr(fin, _i32p), _np_ptr(fpr, _u32p), _np_ptr(T.h_rec, _i32p), T.n, _np_ptr(need, _u8p))
    else:
        k = L.bmh_sam_need_cigar(C.byref(po), _np_ptr(fin, _i32p), _np_ptr(fpr, _u32p), T.n, _np_ptr(need, _u8p))
    assert k == int(T.need.sum()) and np.array_equal(need[:len(T.fin)], T.need), (k, need, T.need)


def test_host_pa_tag_rounds_like_printf():
    """The pa:f tag of the host formatter (sam_core's integer routine in place of snprintf) for every pair of scores 1..300: Python's "%.3f", which is C's (exact
    value of the nearest double, ties to even: 1/16 -> 0.062, 3/16 -> 0.188).  The records are those of test_device_text_pa_tag_rounds_like_printf."""
    from bwamem_hip.lib import format_sam
    po = sam_table.post_opt({})
    A, Bm = np.meshgrid(np.arange(1, 301), np.arange(1, 301), indexing="ij")
    a, b = A.reshape(-1).astype(np.int32), Bm.reshape(-1).astype(np.int32)
    n, L = len(a), 10
    fin = np.zeros((n, 16), np.int32)
    fin[:, 0] = np.arange(n); fin[:, 1] = a; fin[:, 3] = L; fin[:, 6] = L; fin[:, 8] = a; fin[:, 9] = 100; fin[:, 10] = -1; fin[:, 12] = -1; fin[:, 13] = 60
    fin[:, 15] = 1 | (b << 2)
    aln = np.zeros((n, 8), np.int32); aln[:, 3] = 1; aln[:, 6] = 2                      # position 0, forward, one operation, NM 0, MD "10"
    cigar = np.zeros((n, 4), np.uint32); cigar[:, 0] = L << 4
    md = np.zeros((n, 4), np.uint8); md[:, :2] = np.frombuffer(b"10", np.uint8)
    txt = format_sam(po, [f"r{i}" for i in range(n)], np.tile(np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], np.uint8), n), np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32),
                     [("c", 1000)], fin, np.ones(n, np.uint32), np.arange(n, dtype=np.int64), aln, cigar, md, as_bytes=True)
    got = [l.split(b"pa:f:")[1].split(b"\t")[0].decode() for l in txt.split(b"\n") if l]
    want = ["%.3f" % (float(x) / float(y)) for x, y in zip(a.tolist(), b.tolist())]
    assert len(got) == n
    bad = [(int(x), int(y), g, w) for x, y, g, w in zip(a, b, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    assert "0.062" in got and "0.188" in got
