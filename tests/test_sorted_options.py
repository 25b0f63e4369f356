"""The options of sorted output as one record (bmh_sorted_opt_t, bmh_sorted_results_t): marking under each of its twelve option combinations (and
off), coverage off and on, statistics off and on, a BAI and a CSI index, through bam_sorted_file on test_markdup_options' stream in windows of 7 records, on the
host.  What the combinations must agree on follows from what each part reads: the file's bytes depend on the marking alone, the index on the file and its
format, the coverage and the statistics on the records and their 0x400 flags -- so each equals the call that computes it alone.  One refused call per part leaves
every pointer of a C caller NULL.  The same matrix runs on the device, and the aligner's one setter is tested, in test_sorted_options_gpu.py."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from bwamem_hip.lib import bam_coverage, bam_sort, bam_sorted_file, bam_stats
from test_bam_dup import CONTIGS
from test_bam_stats import srec
from test_markdup_options import COMBOS, HDR, host_markdup, kw_id, stream

HERE = os.path.dirname(os.path.abspath(__file__))
WINDOW = 7                                                         # (about a hundred records: some fifteen windows)
COVERAGE, STATS = dict(bin=100_000, min_mapq=1), dict(insert_cap=300)      # (chr1 holds 4 * 10^8 bases: some 4000 bins)
INDEXES = (dict(), dict(index_format="csi", csi_min_shift=10))
MARKING = [None] + COMBOS                                          # None: no marking
PARTS = list(itertools.product((False, True), (False, True), INDEXES))


def marking_id(kw) -> str:
    return "unmarked" if kw is None else kw_id(kw)


def sorted_file(kw, coverage: bool, stats: bool, ix: dict, host: bool = True) -> dict:
    """bam_sorted_file under one combination -> its results by name"""
    mark = dict(markdup=True, **kw) if kw is not None else {}
    r = list(bam_sorted_file(HDR, CONTIGS, stream(), window=WINDOW, host=host, coverage=COVERAGE if coverage else None, stats=STATS if stats else None, **ix, **mark))
    out = dict(bam=r.pop(0), index=r.pop(0))
    for name, on in (("markdup", kw is not None), ("coverage", coverage), ("stats", stats)):
        if on:
            out[name] = r.pop(0)
    assert not r
    return out


def same_arrays(a: dict, b: dict) -> bool:
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def check_combination(kw, host: bool):
    """every part of every call equals the call that computes that part alone (host forms: the device's are compared with the same)"""
    if kw is not None and "optical_distance" in kw:                # a stand-alone file has no optical step, whatever else is asked for
        for coverage, stats, ix in PARTS:
            with pytest.raises(ValueError, match="a stand-alone sorted file has no optical step"):
                sorted_file(kw, coverage, stats, ix, host)
        return
    marked = host_markdup(kw)[0] if kw is not None else stream()
    in_order = bam_sort(marked, host=True)
    want_cov = bam_coverage(in_order, CONTIGS, host=True, **COVERAGE)
    want_stats = bam_stats(in_order, len(CONTIGS), host=True, **STATS)
    alone = {k: sorted_file(kw, False, False, ix) for k, ix in enumerate(INDEXES)}
    assert alone[0]["bam"] == alone[1]["bam"] and alone[0]["index"][:4] == b"BAI\1" and alone[1]["index"] != alone[0]["index"]
    if kw is not None:
        assert alone[0]["markdup"] == host_markdup(kw)[1]
    assert int(want_stats["flag"][0, 4]) == (alone[0]["markdup"]["records_flagged"] if kw is not None else 0)      # (the statistics see the marking's flags)
    for coverage, stats, ix in PARTS:
        got, base = sorted_file(kw, coverage, stats, ix, host), alone[INDEXES.index(ix)]
        what = (marking_id(kw), coverage, stats, ix)
        assert got["bam"] == base["bam"] and got["index"] == base["index"] and got.get("markdup") == base.get("markdup"), what
        assert set(got) == {"bam", "index"} | ({"markdup"} if kw is not None else set()) | ({"coverage"} if coverage else set()) | ({"stats"} if stats else set()), what
        assert not coverage or same_arrays(got["coverage"], want_cov), what
        assert not stats or same_arrays(got["stats"], want_stats), what


@pytest.mark.parametrize("kw", MARKING, ids=marking_id)
def test_every_part_equals_its_single_feature_call(kw):
    check_combination(kw, host=True)


def test_the_stream_exercises_every_part():
    full = sorted_file(dict(barcode_tag="RX", barcode_edits=1), True, True, INDEXES[1])
    plain = sorted_file(None, True, True, INDEXES[1])
    assert full["markdup"]["records_flagged"] > 0 and full["bam"] != plain["bam"]
    assert int(full["coverage"]["n_reads"].sum()) < int(plain["coverage"]["n_reads"].sum())      # (marked duplicates are counted out)
    assert len(full["coverage"]["bin_sum"]) > len(CONTIGS) and int(full["coverage"]["bin_sum"].sum()) > 0
    assert int(full["stats"]["flag"][0, 0]) > 10 * WINDOW and int(full["stats"]["flag"][0, 4]) == full["markdup"]["records_flagged"] and int(plain["stats"]["flag"][0, 4]) == 0


def test_the_keywords_refuse_as_before():
    s = stream()
    for kw, words in ((dict(barcode_edits=1), r"barcode_edits needs markdup=True \(barcodes are grouped where duplicates are marked\)$"),
                      (dict(barcode_tag="RX"), r"barcode_tag / barcode_name need markdup=True \(barcodes are compared where duplicates are marked\)$"),
                      (dict(optical_distance=5), r"optical_distance needs markdup=True"), (dict(index_format="csi", csi_min_shift=9), "10 .. 24"),
                      (dict(stats=dict(insert_cap=1)), "insert_cap"), (dict(coverage=dict(tile=5000)), "tile")):
        with pytest.raises(ValueError, match="^bam_sorted_file: .*" + words):
            bam_sorted_file(HDR, CONTIGS, s, host=True, **kw)


_REFUSED_CALLS = r"""
import ctypes as C, sys
import bwamem_hip
from bwamem_hip.lib import (BamPostOpt, BamPostResult, BamStats, BamStatsOpt, Coverage, CoverageOpt, MarkdupCounts, MarkdupOpt, SortedOpt, SortedResults, _SINK, _markdup_api,
                            _sorted_file_api, _u64p)
L = _sorted_file_api(_markdup_api(bwamem_hip.load_library()))
devices = (False, True) if sys.argv[1] == "both" else (False,)
bad_nm, path = bytes.fromhex(sys.argv[2]), sys.argv[3].encode()
names, lens = (C.c_char_p * 1)(b"c"), (C.c_int32 * 1)(1000)
GARBAGE = 0xdeadbee0


def records():
    mo, mc, co, so, cov, st = MarkdupOpt(), MarkdupCounts(), CoverageOpt(0, 0, 10, 0), BamStatsOpt(100), Coverage(), BamStats()
    L.bmh_markdup_opt_default(C.byref(mo))
    cov.hist = cov.n_reads = cov.bin_sum = C.cast(GARBAGE, _u64p)
    st.flag = st.insert_hist = st.mapq = C.cast(GARBAGE, _u64p)
    opt = SortedOpt(1, 7, 0, 14, 0, None, C.pointer(mo), C.pointer(co), C.pointer(so))
    return mo, co, so, cov, st, opt, SortedResults(C.pointer(mc), C.pointer(cov), C.pointer(st)), mc


def all_null(cov, st):
    return not (cov.hist or cov.n_reads or cov.bin_sum or cov.cov_bases or cov.sum_depth or cov.max_depth or cov.sum_mapq or st.flag or st.insert_hist or st.mapq or st.summary or
                st.contig_mapped or st.contig_unmapped)


def spoil(part, mo, co, so, opt):
    if part == "index":
        opt.index_format, opt.min_shift = 1, 9
    elif part == "stats":
        so.insert_cap = 1
    elif part == "coverage":
        co.tile = 5000
    elif part == "markdup":
        mo.optical_distance = 25                                    # (refused in a stand-alone file; the post-processor takes it: there the barcode mode is spoiled)


for device in devices:
    for part in ("index", "stats", "coverage", "markdup", "record", "none"):
        if device and part in ("record", "none"):
            continue                                                # (what reaches the records runs on the device: test_sorted_options_gpu.py)
        mo, co, so, cov, st, opt, res, mc = records()
        spoil(part, mo, co, so, opt)
        recs = bad_nm if part == "record" else b""
        bam, idx, nb, ni = C.c_void_p(GARBAGE), C.c_void_p(GARBAGE), C.c_uint64(7), C.c_uint64(7)
        head = [b"@CO\tx\n", 1, names, C.addressof(lens), recs, len(recs), C.byref(opt)] + ([None] if device else [])
        rc = (L.bmh_bam_sorted_file_device if device else L.bmh_bam_sorted_file_host)(*head, C.byref(bam), C.byref(nb), C.byref(idx), C.byref(ni), C.byref(res))
        if part == "none":                                          # the same records, nothing spoiled: every part is there, and is released
            assert rc == 0 and bam.value and idx.value and cov.hist and st.flag and res.parts == 1 | 16 | 32, (rc, res.parts)
            L.bmh_free.argtypes = [C.c_void_p]
            L.bmh_bam_stats_free.argtypes = [C.POINTER(BamStats)]
            for p in (bam, idx, cov.n_reads, cov.cov_bases, cov.sum_depth, cov.max_depth, cov.sum_mapq, cov.hist, cov.bin_sum):
                L.bmh_free(C.cast(p, C.c_void_p))
            L.bmh_bam_stats_free(C.byref(st))
            continue
        assert rc == -2 and bam.value is None and idx.value is None and all_null(cov, st), (device, part, rc, bam.value, idx.value)
        assert res.parts == 0 and res.coverage_ms == 0 and res.stats_windows == 0
    # the post-processor: the same record inside its own, the same promise about out's pointers and the results' arrays
    L.bmh_bam_post_file_host.argtypes = [C.c_char_p, C.POINTER(BamPostOpt), _SINK, C.c_void_p, C.POINTER(BamPostResult), C.POINTER(SortedResults)]
    L.bmh_bam_post_file_device.argtypes = [C.c_char_p, C.POINTER(BamPostOpt), C.c_void_p, _SINK, C.c_void_p, C.POINTER(BamPostResult), C.POINTER(SortedResults)]
    written = []
    sink = _SINK(lambda _u, p, n: written.append(n) or 0)
    for part in ("index", "stats", "coverage", "markdup", "record"):
        if device and part == "record":
            continue
        mo, co, so, cov, st, opt, res, mc = records()
        spoil(part, mo, co, so, opt)
        if part == "markdup":
            mo.optical_distance, mo.barcode_mode = -1, 7
        out = BamPostResult()
        out.index = out.header_text = GARBAGE
        po = BamPostOpt(opt, 0, 0, 0)
        src = path if part == "record" else b"/nonexistent/never-opened.bam"      # (the options are refused before the input is touched)
        args = [src, C.byref(po)] + ([None] if device else []) + [sink, None, C.byref(out), C.byref(res)]
        rc = (L.bmh_bam_post_file_device if device else L.bmh_bam_post_file_host)(*args)
        assert rc == -2 and not out.index and not out.header_text and not out.contig_names and all_null(cov, st), (device, part, rc)
        assert part == "record" or not written
print("ok")
"""


def test_one_refused_call_per_part_leaves_every_pointer_null(tmp_path):
    """a C caller's pointers are not initialised: a CSI shift of 9, an insert_cap of 1, a tile beyond 4096, an optical distance in a stand-alone file (the
    post-processor: a barcode mode of 7) and a record whose NM tag is no count each leave *bam, *index (out's pointers) and every array of the coverage and the
    statistics NULL.  The option refusals come before anything touches a device, so the device forms are called with them as well; a child process, since a
    free() of such a pointer ends the process"""
    from test_bam_post import bam_file
    bad = srec(b"b", pos=20, tag=b"NMZ1\0") + srec(b"ok")
    path = bam_file(tmp_path / "bad_nm.bam", "@HD\tVN:1.6\n", [("c", 1000)], bad)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(HERE, "..", "bwa-mem_gpu_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-c", _REFUSED_CALLS, "both", bad.hex(), str(path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stdout.decode().strip() == "ok", r.stderr.decode(errors="replace")[-3000:]


def test_host_forms_under_sanitizers(tmp_path):
    """bmh_bam_sorted_file_host and bmh_bam_post_file_host with every part on, one refused call per part and everything released, in a stand-alone program
    (tests/sorted_output_host.cpp) built from the library's host sources with -fsanitize=address,undefined: nothing for the sanitizers to report.  The two
    sources that hold kernels beside their host forms (the converter and the compressor) are compiled whole, with the sanitizers on their host side only; the
    program makes no device call."""
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    hipcc, cxx = "/opt/rocm/bin/hipcc", "/opt/rocm/llvm/bin/clang++"
    if not (os.path.exists(hipcc) and os.path.exists(cxx)):
        pytest.skip("no HIP compiler to build the host sources with")
    out = os.path.join(HERE, "_build", "sorted_output_host.d"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sorted_output_host")
    host = [os.path.join(HERE, "sorted_output_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_sort_host.cpp", "bam_dup_host.cpp", "bam_cov_host.cpp", "bam_stats_host.cpp", "bam_post.cpp",
                                                                                             "bam_tpl_host.cpp", "reads_src.cpp", "reads_io.cpp", "sam_format.cpp")]
    both = [os.path.join(csrc, f) for f in ("bam_kernels.hip", "deflate_kernels.hip")]
    dep = host + both + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(HERE, "..", "include", "bwamem_hip.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in dep):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        common = ["--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-c"]
        subprocess.check_call([cxx, "-x", "hip", "--offload-host-only", "-pthread"] + common + san + host, cwd=out)
        subprocess.check_call([hipcc] + common + [a for s in san for a in ("-Xarch_host", s)] + both, cwd=out)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-pthread"] + san + [os.path.splitext(os.path.basename(f))[0] + ".o" for f in host + both] + ["-o", exe, "-ldl"], cwd=out)
    r = subprocess.run([exe, str(tmp_path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and r.stdout.decode().strip() == "ok" and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the program) reported:\n" + err[-4000:]
