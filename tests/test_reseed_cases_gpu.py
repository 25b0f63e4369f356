"""The re-seeding kernels (csrc/reseed_kernels.hip) on the case table of tests/reseed_cases.py: bmh_seed_batch_reseed's output must equal
tests/golden/reseed_cases.npz -- what the REFERENCE returned for the case -- under common.assert_seeds_equal, the number of groups must agree, and
bmh_reseed_last_counts must report the path the restatement predicts: round-2 tasks, tasks sent through the second launch, groups per round.  Everything
exact, nothing skips.

Forms: the index forms of test_seed_cases_gpu.FORMS; one workspace for the whole table, in order and back, calls with re-seeding off between them; the
first launch's column size (knob RESEED_CAP) at 1, 2, 31, 33 and 100 000, so that every task, and none, takes the second launch; the overflow list's order,
which an atomic decides, twice."""
import functools

import numpy as np
import pytest

import common
import reseed_cases as rc
from test_seed_cases_gpu import FORMS, Indexes, on_device

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def bases():
    """the most bases a case of the table has"""
    return max(int(rc.get(n).lens.sum()) for n in rc.NAMES)


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()           # raises if the HIP extension is missing: no fallback
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.fixture(scope="module")
def golden():
    return rc.load_fixture()


@pytest.fixture(scope="module")
def indexes(hip):
    ix = Indexes(hip)
    yield ix
    ix.free()


def workspace(hip):
    n = max(bases(), 1 << 16)
    return hip.SeedWorkspace(300, n, max_cands=n, max_occ=64)


def run_case(ws, dindex, c, reseed=True):
    from bwamem_hip.lib import reseed_last_counts, seeds_to_host
    r, o, l = on_device(c)
    s = ws.seed_batch(dindex, r, o, l, c.msl, reseed=rc.reseed_opt(c) if reseed else None)
    out = seeds_to_host(s, len(c.lens))
    out["n_smems"], out["counts"] = int(s.n_smems), reseed_last_counts()
    return out


def check(c, got, golden, what="", cap=rc.CAP):
    want, S = golden[c.name], c.S
    common.assert_seeds_equal(got, want, f"{what}{c.name}: ")
    assert got["n_smems"] == want["n_smems"], (what, c.name)
    # the path: tasks, tasks whose forward list has more than `cap` entries, groups of rounds 1, 2 and 3; and the work: rank steps of rounds 2 and 3
    assert got["counts"] == dict(tasks=S.n_tasks, overflowed=int((S.lists > cap).sum()), rounds=tuple(want["rounds"].tolist()), steps=rc.device_steps(S, cap)), \
        (what, c.name, got["counts"], rc.device_steps(S, cap))
    assert tuple(want["rounds"].tolist()) == S.rounds


def check_off(c, got, what=""):
    """re-seeding off (bmh_seed_batch): the first round alone"""
    common.assert_seeds_equal(got, c.S.cols1, f"{what}{c.name}, re-seeding off: ")
    assert got["n_smems"] == c.S.cols1["n_smems"], (what, c.name)


def run_table(hip, indexes, golden, text, kbits, intv, names=rc.NAMES, what="", back=True, cap=rc.CAP, off_every=0):
    """one workspace for the whole table, in order and back: the buffers of the re-seeding state grow and are then larger than needed; with off_every, every
    off_every-th case runs without re-seeding first"""
    ws = workspace(hip)
    try:
        for i, name in enumerate(tuple(names) + (tuple(names)[::-1] if back else ())):
            c = rc.get(name)
            d = indexes.get(c.genome, text, kbits, intv)
            if off_every and i % off_every == 0:
                check_off(c, run_case(ws, d, c, reseed=False), what)
            check(c, run_case(ws, d, c), golden, what, cap)
    finally:
        ws.free()


@pytest.mark.parametrize("form", FORMS)
def test_table_in_every_index_form(hip, indexes, golden, form):
    run_table(hip, indexes, golden, *FORMS[form], what=form + ": ")


def test_one_workspace_with_reseeding_on_and_off(hip, indexes, golden):
    """nothing is carried over: not the overflow list, not the groups per task, not the counters"""
    import ctypes as C
    from bwamem_hip.lib import ReseedOpt, SeedsT, reseed_last_counts
    run_table(hip, indexes, golden, False, False, 16, what="on and off: ", off_every=2)
    # a batch whose every task overflows, one without a task, one without a group, the first again
    ws = workspace(hip)
    try:
        for name in ("overflow_all", "tasks_0", "overflow_65", "no_group", "overflow_all", "polyA_600", "tasks_257", "overflow_1"):
            c = rc.get(name)
            check(c, run_case(ws, indexes.get(c.genome, False, False, 16), c), golden, "mixed: ")
        last, c = reseed_last_counts(), rc.get("overflow_65")
        check_off(c, run_case(ws, indexes.get(c.genome, False, False, 16), c, reseed=False), "mixed: ")
        assert reseed_last_counts() == last                     # (bmh_seed_batch is not the call they describe)
        r, o, l = on_device(c)                                  # bmh_seed_batch_reseed with enable = 0 is: no task, no group counted
        ws.seed_batch(indexes.get(c.genome, False, False, 16), r, o, l, c.msl, reseed=None)
        s, off = SeedsT(), ReseedOpt.default(enable=0)
        d = indexes.get(c.genome, False, False, 16)
        assert hip.load_library().bmh_seed_batch_reseed(ws.handle, d.handle, r.data_ptr(), o.data_ptr(), l.data_ptr(), l.numel(), c.msl, C.byref(off), 0, C.byref(s)) == 0
        assert int(s.n_smems) == c.S.cols1["n_smems"] and reseed_last_counts() == dict(tasks=0, overflowed=0, rounds=(0, 0, 0), steps=(0, 0))
    finally:
        ws.free()


@pytest.mark.parametrize("cap", [1, 2, 31, 33, 100_000])
def test_first_launch_column_size(hip, indexes, golden, cap):
    """RESEED_CAP: the seeds are those at 32; at 1 every task whose list has more than one entry takes the second launch, at 100 000 none"""
    L = hip.load_library()
    L.bmh_tune_set(b"RESEED_CAP", cap, 0)
    try:
        run_table(hip, indexes, golden, False, False, 16, what="cap %d: " % cap, back=False, cap=cap)
    finally:
        L.bmh_tune_set(b"RESEED_CAP", 0, 1)
    lists = np.concatenate([rc.get(n).S.lists for n in rc.NAMES])
    assert cap != 1 or int((lists > 1).sum()) > 0.9 * len(lists)
    assert cap != 100_000 or int((lists > cap).sum()) == 0 < int((lists > rc.CAP).sum())


def test_the_overflow_lists_order_does_not_matter(hip, indexes, golden):
    """65 overflowing tasks: an atomic decides their order in the second launch; the columns are the same twice, and with every task in that launch"""
    c = rc.get("overflow_65")
    assert c.S.n_over == 65
    d = indexes.get(c.genome, False, False, 16)
    L = hip.load_library()
    ws = workspace(hip)
    try:
        a, b = run_case(ws, d, c), run_case(ws, d, c)
        L.bmh_tune_set(b"RESEED_CAP", 1, 0)
        e = run_case(ws, d, c)
    finally:
        L.bmh_tune_set(b"RESEED_CAP", 0, 1)
        ws.free()
    check(c, a, golden, "first: "); check(c, b, golden, "second: "); check(c, e, golden, "cap 1: ", cap=1)
    for k in rc.SEED_KEYS:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], e[k]), k
