"""The mate rescue's local alignment on the hand-made jobs of tests/msw_cases.py, without a GPU.  The chain of evidence, every link exact:
the reference's compiled ksw_align2 (oracle/ref_harness.c: ref_align2) -> tests/golden/msw_cases.npz, what it returned for every job
(tests/golden/make_msw_golden.py) -> the host walk csrc/local_sw.cpp (bmh_local_sw_c) on the same jobs, here -> the four kernel forms of
csrc/pair_kernels.hip, in tests/test_msw_cases_gpu.py.  Where the reference's library was built the host walk is compared with it live as well, and a
program of its own (tests/msw_host.cpp) runs the host walk over the table under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import msw_cases
from bwamem_hip.lib import ExtParams, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "msw_cases.npz")


def ext_params(scoring):
    ep = ExtParams.default()
    ep.a, ep.b, ep.o_del, ep.e_del, ep.o_ins, ep.e_ins = scoring
    return ep


@pytest.fixture(scope="module")
def golden():
    """name -> the reference's rows for the case's jobs (read-only).  A table edited without regenerating the fixture is refused here."""
    z = np.load(FIXTURE)
    assert str(z["digest"]) == msw_cases.digest(), "tests/msw_cases.py changed: run tests/golden/make_msw_golden.py where the reference's library can be built"
    out = z["out"]
    sl = msw_cases.job_slices()
    assert out.dtype == np.int32 and out.shape == (sum(c.n for c in msw_cases.all_cases().values()), 7)
    out.setflags(write=False)
    return {name: out[s] for name, s in sl.items()}


_host = {}


def host_rows(name):
    """bmh_local_sw_c on every job of a case, computed once"""
    if name not in _host:
        c = msw_cases.get(name)
        L = load_library()
        L.bmh_local_sw_c.restype = None
        L.bmh_local_sw_c.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        ep = ext_params(c.scoring)
        text = msw_cases.text_of(c)
        res = np.zeros((c.n, 7), np.int32)
        for k in range(c.n):
            q, t = c.q[k].copy(), msw_cases.target_of(c, k, text)
            q0, t0 = q.copy(), t.copy()
            L.bmh_local_sw_c(len(q), q.ctypes.data_as(C.c_void_p), len(t), t.ctypes.data_as(C.c_void_p), C.byref(ep), int(c.xtra[k]), res[k].ctypes.data_as(C.c_void_p))
            assert np.array_equal(q, q0) and np.array_equal(t, t0)      # reversed in place for the second pass, and restored
        res.setflags(write=False)
        _host[name] = res
    return _host[name]


def check_must(c, res):
    assert c.must
    for what, f in c.must.items():
        assert f(res), (c.name, what, res[:12])


def test_the_table_covers_what_it_is_for():
    cases = msw_cases.all_cases()
    assert {c.family for c in cases.values()} == set(msw_cases.FAMILIES)
    n_jobs = sum(c.n for c in cases.values())
    assert 200 <= n_jobs <= 800 and all(1 <= c.n <= 40 for c in cases.values())
    assert sum(len(c.genome) for c in cases.values() if c.name != "tlen_65535") < 400_000
    by = lambda fam: [c for c in cases.values() if c.family == fam]
    assert {int(c.l_ms[0]) for c in by("lengths")} == set(msw_cases.LENGTHS)
    # byte mode ends at 249 bases, the LDS forms at 40 segments
    assert all((l < 250) == bool(x & msw_cases.XBYTE) for c in by("lengths") for l, x in zip(c.l_ms, c.xtra))
    assert max(msw_cases.slen_of(int(l), int(x)) for c in cases.values() for l, x in zip(c.l_ms, c.xtra)) == msw_cases.MSW_SLEN
    assert {c.n for c in by("batch_size")} == {1, 3, 4, 5, 8, 9}
    assert {int(t) for t in (cases["tlen_edges"].re - cases["tlen_edges"].rb)} == set(msw_cases.TLENS)
    assert {c.scoring for c in by("scorings")} == set(msw_cases.SCORINGS)
    assert {c.l_pac % 4 for c in by("text_edges")} == {1, 2, 3}
    for c in cases.values():                                        # windows on the reverse half in (nearly) every family
        c.on_reverse = int((c.rb >= c.l_pac).sum())
    assert sum(1 for f in msw_cases.FAMILIES if any(c.on_reverse for c in by(f))) >= 10
    # -b fits the reference's int8_t matrix
    assert all(c.scoring[1] <= 128 for c in cases.values())


@pytest.mark.parametrize("name", msw_cases.names())
def test_host_walk_equals_the_reference_fixture_and_the_case_holds(golden, name):
    c = msw_cases.get(name)
    res = host_rows(name)
    check_must(c, res)
    want = golden[name]
    # the overflow family, and nothing else, ends its byte pass at 255
    assert ((want[:, 0] == 255) == c.overflow).all()
    assert np.array_equal(want[c.overflow, 2:], np.full((int(c.overflow.sum()), 5), -1))
    bad = np.nonzero((res != want).any(1))[0]
    assert bad.size == 0, (name, bad[:5], res[bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("name", msw_cases.names())
def test_host_walk_equals_the_live_reference(ref, golden, name):
    """where oracle/_ref/libref.so was built: ref_align2 itself, and the fixture against it (an overflow job's first pass alone, as the generator takes it)"""
    if not hasattr(ref.lib, "ref_align2"):
        pytest.skip("oracle/_ref/libref.so has no ref_align2")
    c = msw_cases.get(name)
    want = msw_cases.reference_rows(ref, c)
    assert (want[c.overflow, 0] == 255).all() and (want[~c.overflow, 0] != 255).all()
    assert np.array_equal(want, golden[name])
    assert np.array_equal(host_rows(name), want)


def test_host_walk_under_the_sanitizers(golden, tmp_path):
    """tests/msw_host.cpp + csrc/local_sw.cpp built with -fsanitize=address,undefined, a plain child process: a clean exit, no report, the fixture's numbers.
    (An overflowing byte pass leaves qe = -1; the second pass over the empty query once read h0[-lanes + l - 1] of an empty vector.)"""
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "msw_host_san")
    csrc = os.path.join(ROOT, "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "msw_host.cpp"), os.path.join(csrc, "local_sw.cpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src + [os.path.join(csrc, "local_sw.h")]):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                               "-I", csrc, *src, "-o", exe])
    jobs = tmp_path / "jobs.txt"
    want = []
    with open(jobs, "w") as f:
        for name, c in msw_cases.all_cases().items():
            text = msw_cases.text_of(c)
            for k in range(c.n):
                t = msw_cases.target_of(c, k, text)
                f.write(" ".join(map(str, (*c.scoring, int(c.xtra[k]), len(c.q[k]), len(t)))) + "\n")
                f.write((c.q[k] + ord("0")).astype(np.uint8).tobytes().decode() + "\n" + (t + ord("0")).astype(np.uint8).tobytes().decode() + "\n")
            want.append(golden[name])
    want = np.concatenate(want)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([exe, str(jobs)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    got = np.array([[int(x) for x in line.split()] for line in r.stdout.splitlines()], np.int32)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])
