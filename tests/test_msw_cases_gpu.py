"""The mate rescue's local alignment on the device (csrc/pair_kernels.hip) on the hand-made jobs of tests/msw_cases.py: every batch through
bmh_matesw_batch_device with the register forms allowed (MSW_REG 1) and without (0), all seven result words against tests/golden/msw_cases.npz --
what the REFERENCE's ksw_align2 returned, not the host walk under test beside it (tests/test_msw_cases.py compares that one with the same file).
Which of the four kernels a batch reaches is restated here from msw_launch; the batches again in reverse order on the same stream (one scratch, the
bookkeeping words never cleared); and the jobs the device does not take, refused before a kernel is launched.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import common
import msw_cases
from test_msw_cases import ext_params, golden  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

BMH_EINVAL = -2


class Job(C.Structure):
    _fields_ = [("rb", C.c_int64), ("re", C.c_int64), ("read", C.c_uint32), ("l_ms", C.c_int32), ("is_rev", C.c_int32), ("xtra", C.c_int32), ("bl_off", C.c_uint32),
                ("pad", C.c_uint32)]


def expected_kernel(c, msw_reg):
    """msw_launch restated: the register forms take a batch whose jobs all run in byte mode with columns of at most 16 segments (<= 10: the smaller one), where
    a gap open costs something and a and b are below 100; the LDS forms take the rest, with the width compiled in where every job is in byte mode"""
    a, b, _, _, o_ins, e_ins = c.scoring
    byte_all = all(x & msw_cases.XBYTE for x in c.xtra)
    cap = max(msw_cases.slen_of(int(l), int(x)) for l, x in zip(c.l_ms, c.xtra))
    if byte_all and cap <= 16 and o_ins > 0 and e_ins > 0 and a < 100 and b < 100 and msw_reg:
        return "msw_reg_kernel<10>" if cap <= 10 else "msw_reg_kernel<16>"
    return "msw_kernel<true>" if byte_all else "msw_kernel<false>"


class Device:
    """the library, a stand-in FM index (the kernels read the 2-bit text of an index and nothing else of it) and every case's text and reads on the device"""

    def __init__(self):
        import torch
        import bwamem_hip as B
        assert torch.cuda.is_available(), "these tests need a GPU"
        self.torch, self.B = torch, B
        self.L = L = B.load_library()                               # raises if the HIP extension is missing: no fallback
        L.bmh_matesw_batch_device.restype = C.c_int
        L.bmh_matesw_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        _, self.idx = common.genome_and_index(2_000, seed=1)
        self.up = {}

    def of(self, c):
        if c.name not in self.up:
            t = self.torch
            self.up[c.name] = (self.B.Index.upload(self.idx, pac=c.pac, l_pac=c.l_pac), t.from_numpy(c.reads).cuda(),
                               t.from_numpy(c.offs.astype(np.int64).astype(np.int32)).cuda())
        return self.up[c.name]

    def jobs_of(self, c):
        jobs = (Job * c.n)()
        for k in range(c.n):
            jobs[k].rb, jobs[k].re, jobs[k].read, jobs[k].l_ms, jobs[k].is_rev, jobs[k].xtra = int(c.rb[k]), int(c.re[k]), k, int(c.l_ms[k]), int(c.is_rev[k]), int(c.xtra[k])
        return jobs

    def run(self, c, msw_reg, jobs=None, reads=None):
        """bmh_matesw_batch_device on the default stream -> (return code, rows [n, 7], prefilled with -7)"""
        dindex, r, o = self.of(c)
        if reads is not None:
            r, o = reads
        jobs = self.jobs_of(c) if jobs is None else jobs
        ep = ext_params(c.scoring)
        out = np.full((len(jobs), 7), -7, np.int32)
        self.L.bmh_tune_set(b"MSW_REG", msw_reg, 0)
        try:
            rc = self.L.bmh_matesw_batch_device(dindex.handle, r.data_ptr(), o.data_ptr(), C.byref(ep), C.byref(jobs), len(jobs), out.ctypes.data_as(C.c_void_p), None)
        finally:
            self.L.bmh_tune_set(b"MSW_REG", 0, 1)
        return rc, out

    def free(self):
        for dindex, _, _ in self.up.values():
            dindex.free()
        self.up = {}


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.free()


def assert_rows(c, out, want, what):
    bad = np.nonzero((out != want).any(1))[0]
    assert bad.size == 0, (c.name, what, bad[:5], [c.tags[k] for k in bad[:3]], out[bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("msw_reg", [1, 0])
@pytest.mark.parametrize("name", msw_cases.names())
def test_device_equals_the_reference_fixture(dev, golden, name, msw_reg):  # noqa: F811
    c = msw_cases.get(name)
    print(f"{name}: {c.n} jobs, MSW_REG {msw_reg} -> {expected_kernel(c, msw_reg)}")
    rc, out = dev.run(c, msw_reg)
    assert rc == 0, dev.L.bmh_last_error()
    assert_rows(c, out, golden[name], expected_kernel(c, msw_reg))


def test_the_table_reaches_all_four_kernels():
    reached = {knob: {} for knob in (1, 0)}
    for knob in (1, 0):
        for name, c in msw_cases.all_cases().items():
            reached[knob].setdefault(expected_kernel(c, knob), []).append(name)
        print(f"MSW_REG {knob}: " + ", ".join(f"{k}: {len(v)} batches" for k, v in sorted(reached[knob].items())))
    assert set(reached[1]) == {"msw_reg_kernel<10>", "msw_reg_kernel<16>", "msw_kernel<true>", "msw_kernel<false>"}
    assert set(reached[0]) == {"msw_kernel<true>", "msw_kernel<false>"}
    by = lambda knob, k: set(reached[knob][k])
    # the limits of the classes, each from both sides: 160 | 161 columns of ten, 249 | 250 byte and word, a free insertion open and b at the register forms' gate
    assert "len_160" in by(1, "msw_reg_kernel<10>") and "len_161" in by(1, "msw_reg_kernel<16>")
    assert "len_249" in by(1, "msw_reg_kernel<16>") and "len_250" in by(1, "msw_kernel<false>") and "mixed_249_250" in by(1, "msw_kernel<false>")
    assert {"scoring_1_4_6_1_0_1_byte", "scoring_1_100_6_1_6_1_byte", "overflow_1_100_6_1_6_1"} <= by(1, "msw_kernel<true>")
    assert {"overflow_1_6_6_1_6_1", "overflow_1_9_6_1_6_1", "ins_cross_16_default"} <= by(1, "msw_reg_kernel<16>")
    assert {"overflow_2_8_5_2_5_2", "overflow_1_99_6_1_6_1", "ins_cross_10_default", "ins_cross_10_default_beside_37", "ties"} <= by(1, "msw_reg_kernel<10>")
    assert "ties_long" in by(1, "msw_reg_kernel<16>") and {"ties_word", "overflow_mixed_width", "mixed_40_260"} <= by(1, "msw_kernel<false>")


@pytest.mark.parametrize("msw_reg", [1, 0])
def test_batches_again_in_reverse_order_on_the_same_stream(dev, golden, msw_reg):  # noqa: F811
    """one scratch per stream, grown and never cleared: the 65535-row window leaves 2 x 32 k words of bookkeeping behind that the small batches after it lie in"""
    order = list(msw_cases.names())
    assert order.index("tlen_65535") < len(order) - 20
    for names in (order, order[::-1]):
        for name in names:
            c = msw_cases.get(name)
            rc, out = dev.run(c, msw_reg)
            assert rc == 0, dev.L.bmh_last_error()
            assert_rows(c, out, golden[name], "reversed" if names is not order else "in order")


@pytest.mark.parametrize("what,bad,l_ms,tlen,word", msw_cases.refusals())
def test_a_job_the_device_does_not_take_is_refused(dev, golden, what, bad, l_ms, tlen, word):  # noqa: F811
    """bmh_matesw_device_takes on every job: BMH_EINVAL with a message that names the job, nothing launched (the result rows stay as they were), and a valid
    batch straight after comes out right.  The other four jobs are ordinary; all of them lie inside the text and the reads, whatever the kernel were to do."""
    c = msw_cases.get("tlen_65535")
    rng = np.random.default_rng(5)
    n, room = 5, 336
    reads = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n * room)].copy()
    r = dev.torch.from_numpy(reads).cuda()
    o = dev.torch.arange(n + 1, dtype=dev.torch.int32).cuda() * room
    jobs = (Job * n)()
    for k in range(n):
        jobs[k].rb, jobs[k].re, jobs[k].read, jobs[k].l_ms, jobs[k].is_rev = 1000 * k, 1000 * k + 400, k, 150, k & 1
        jobs[k].xtra = msw_cases.xtra_of(150, c.scoring)
    jobs[bad].l_ms, jobs[bad].re = l_ms, jobs[bad].rb + tlen
    jobs[bad].xtra = msw_cases.xtra_of(l_ms, c.scoring) & ~(msw_cases.XBYTE if word else 0)
    assert bool(jobs[bad].xtra & msw_cases.XBYTE) != word and 0 <= jobs[bad].rb <= jobs[bad].re <= 2 * c.l_pac and l_ms <= room
    assert not dev.L.bmh_matesw_device_takes(C.c_int(l_ms), C.c_int64(tlen), C.c_int(jobs[bad].xtra))
    for msw_reg in (1, 0):
        rc, out = dev.run(c, msw_reg, jobs=jobs, reads=(r, o))
        msg = dev.L.bmh_last_error().decode()
        assert rc == BMH_EINVAL and f"job {bad} " in msg and "bmh_matesw_device_takes" in msg, (what, rc, msg)
        assert (out == -7).all(), what
        after = msw_cases.get("batch_of_5")
        rc, out = dev.run(after, msw_reg)
        assert rc == 0, dev.L.bmh_last_error()
        assert_rows(after, out, golden["batch_of_5"], "after " + what)
