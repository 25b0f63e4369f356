"""The region tail on the device (csrc/regs_kernels.hip) on the hand-made cases of tests/regs_cases.py: bmh_finalize_regs_device against the host form
bit for bit, which kernel took which read, bmh_dedup_regs_device against the CPU core in dedup-only mode, one and two blocks per wave kernel (a block
then takes read after read through one LDS and one alignment scratch), and the two refusals with a valid batch straight after.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import common
import regs_cases
from test_regs_cases import check_must, host_arrays, host_result, options, run_cpu
from test_regs_core import core_lib

pytestmark = pytest.mark.gpu

_u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def dev():
    """an index handle that carries the cases' 2-bit genome (the tail reads nothing else of an index: its FM index is that of a small stand-in genome)"""
    import torch
    import bwamem_hip as B
    assert torch.cuda.is_available()
    _, idx = common.genome_and_index(2_000, seed=1)
    g, pac = regs_cases.genome()
    dindex = B.Index.upload(idx, pac=pac, l_pac=len(g))
    yield dindex
    dindex.free()


def device_arrays(case):
    import torch
    from bwamem_hip import synth
    flat, offs, _ = host_arrays(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = len(case.rpr)
    return dict(r=t(synth.codes_to_ascii(flat) if len(flat) else np.zeros(1, np.uint8)), o=t(offs.astype(np.int64).astype(np.int32)),
                regs=t(case.regs if len(case.regs) else np.zeros((1, 8), np.int32)), rpr=t(case.rpr.view(np.int32)), fr=t(case.frac_rep), n=n, nr=len(case.regs))


def run_device(dindex, case, d=None):
    """bmh_finalize_regs_device -> (records, out_per_read, class counts [5])"""
    from bwamem_hip.lib import finalize_regs_device, load_library
    co, ep, po = options(case)
    d = d or device_arrays(case)
    out, opr = finalize_regs_device(dindex, co, ep, po, d["r"], d["o"], d["regs"], d["nr"], d["rpr"].data_ptr(), d["fr"].data_ptr(), d["n"], contigs=case.contigs)
    cls = np.zeros(5, np.uint32)
    assert load_library().bmh_finalize_regs_device_last_classes(cls.ctypes.data_as(_u32p)) == 0
    return out.cpu().numpy(), opr.cpu().numpy().view(np.uint32)[:d["n"]], cls


def expected_classes(case):
    """the classification restated: (reads per wave class [5], reads the lane kernel finishes).  A read of up to FIN_NL regions is the lane kernel's unless
    its patch test reaches the alignment -- the CPU core without alignment scratch says so (NEED_DP) --, then it goes to wave class 0."""
    cls, lane = np.zeros(5, np.uint32), 0
    flat, offs, ctg_off = host_arrays(case)
    core = core_lib().regs_core_run
    for r, sl in enumerate(regs_cases.read_slices(case)):
        n = sl.stop - sl.start
        if n == 0:
            continue
        if n <= regs_cases.FIN_NL:
            one = (np.ascontiguousarray(case.reads[r]), np.zeros(1, np.uint64), ctg_off)
            got = run_cpu(core, case, 0, regs=np.ascontiguousarray(case.regs[sl]), rpr=np.array([n], np.uint32), reads=one, id0=case.po["id0"] + r)
            if isinstance(got, int):
                assert got == -1, got                               # regs_core::NEED_DP
                cls[0] += 1
            else:
                lane += 1
        else:
            cls[regs_cases.fin_class(n)] += 1
    return cls, lane


def assert_equal_host(case, out, opr):
    res = host_result(case.name)
    assert np.array_equal(opr, res.opr), np.nonzero(opr != res.opr)[0][:5]
    assert out.shape == res.out.shape and np.array_equal(out, res.out), np.nonzero((out != res.out).any(1))[0][:5]


ABOUT_ALL_CLASSES = ("scattered", "scattered_reversed", "ties", "ties_same", "tandem", "patch_w100", "contigs1", "contigs512", "contigs512_alt")


@pytest.mark.parametrize("name", regs_cases.NAMES)
def test_device_equals_host_and_every_read_takes_its_kernel(dev, name):
    from bwamem_hip.lib import CapacityError
    case = regs_cases.get(name)
    check_must(case, host_result(name))
    if case.device_error:
        # a refusal: BMH_ECAPACITY with its message; a valid batch on the same stream straight after comes out right (error word and counters start afresh)
        with pytest.raises(CapacityError, match=case.device_error):
            run_device(dev, case)
        after = regs_cases.get("mark_ab")
        out, opr, cls = run_device(dev, after)
        assert_equal_host(after, out, opr)
        assert np.array_equal(cls, expected_classes(after)[0])
        return
    out, opr, cls = run_device(dev, case)
    assert_equal_host(case, out, opr)
    want, lane = expected_classes(case)
    print(f"{name}: reads per wave class {cls.tolist()}, lane kernel {lane}, sizes {sorted(set(case.rpr.tolist()))}")
    assert np.array_equal(cls, want), (cls, want)
    if name in ABOUT_ALL_CLASSES:
        assert (cls > 0).all() and lane > 0
        for n in (8, 9, 32, 33, 128, 129, 256, 257, 512, 513):
            assert n in case.rpr or name == "patch_w100"
    if name == "scattered_class2_empty":
        assert cls[2] == 0 and (cls[[0, 1, 3, 4]] > 0).all()
    if "patch" in case.families and name != "patch_w0":
        assert cls[0] >= 4 and (case.rpr <= regs_cases.FIN_NL).sum() >= cls[0] - 2      # small reads handed on by the lane kernel (NEED_DP)


@pytest.mark.parametrize("name", ["ties", "ties_same", "tandem", "patch_w0", "patch_w5", "patch_w20", "patch_w100", "patch_scoring"])
def test_dedup_only_on_the_device_equals_the_core(dev, name):
    """bmh_dedup_regs_device: the fields the header specifies ([0] read, [1..9], [13] the sequence)"""
    import torch
    from bwamem_hip.lib import load_library, _err
    case = regs_cases.get(name)
    want = run_cpu(core_lib().regs_core_dedup, case, 1)
    co, ep, po = options(case)
    d = device_arrays(case)
    out = torch.full((max(d["nr"], 1), 16), -3, dtype=torch.int32, device="cuda"); opr = torch.zeros(max(d["n"], 1), dtype=torch.int32, device="cuda")
    L = load_library()
    m = L.bmh_dedup_regs_device(dev.handle, C.byref(co), C.byref(ep), C.byref(po), d["r"].data_ptr(), d["o"].data_ptr(), d["n"], d["regs"].data_ptr(), d["nr"],
                                d["rpr"].data_ptr(), 1, None, out.data_ptr(), opr.data_ptr(), 0)
    assert m >= 0, _err(L)
    keep = list(range(10)) + [13]
    assert np.array_equal(opr.cpu().numpy().view(np.uint32)[:d["n"]], want[1])
    got = out.cpu().numpy()[:m]
    assert m == len(want[0]) and np.array_equal(got[:, keep], want[0][:, keep]), np.nonzero((got[:, keep] != want[0][:, keep]).any(1))[0][:5]
    assert m < d["nr"]                                              # regions were removed or merged


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("name", ["scattered", "scattered_reversed", "ties", "tandem", "patch_w100", "contigs512_alt"])
def test_read_after_read_through_one_block(dev, name, grid):
    """knob FIN_GRID_MAX: one or two blocks per wave kernel take all the reads of a class one after the other -- a read of 512 regions and then one of 257
    through the same LDS arrays (and the other way round in the reversed batch), alignment after alignment through one scratch"""
    from bwamem_hip.lib import load_library
    case = regs_cases.get(name)
    L = load_library()
    L.bmh_tune_set(b"FIN_GRID_MAX", grid, 0)
    try:
        out, opr, cls = run_device(dev, case)
    finally:
        L.bmh_tune_set(b"FIN_GRID_MAX", 0, 1)
    assert_equal_host(case, out, opr)
    assert (cls >= 1).all() and (name == "patch_w100" or (cls >= 2).all())      # every kernel's block(s) took more than one read (patch_w100: but for one class)
