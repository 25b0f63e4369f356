"""The CIGAR stage on the device (csrc/cigar_kernels.hip) on the hand-made regions of tests/cigar_cases.py: bmh_cigar_batch through ctypes with buffers the
test owns, every word of every row -- position, strand, operations, NM, score, MD length, MD bytes, flags -- against tests/golden/cigar_cases.npz, what the
REFERENCE's mem_reg2aln returned (the score word, which it does not return, from the oracle that tests/test_cigar_cases.py pins to the same file).  Each batch
on its own; every job alone, in a shuffled batch of the whole table, through a sel list and as records of 16 words (z_lds_bytes, max_len, long_split and the
slab stride are properties of the batch: a job's row must not depend on them); lists of 1, 3, 4 and 5 members and batches of 15, 16 and 17 jobs; the batches
again in reverse order and on a second stream; the class counts of BMH_CIGAR_STATS against the restated classifier; the whole table through the
wave-per-region forms alone (BMH_CIGAR_SLOW, a child process); and the CIGAR and MD slots.  All comparisons are exact."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cigar_cases as cc
import common
from test_cigar_cases import expected_rows, golden, small_flags  # noqa: F401  (golden: the fixture)

pytestmark = pytest.mark.gpu

SENT32, SENT8 = 0x5A5A5A5A, 0xEE
MAX_CIGAR, MD_CAP = 512, 1024


def ext_params(scoring):
    from bwamem_hip.lib import ExtParams
    ep = ExtParams.default()
    ep.a, ep.b, ep.o_del, ep.e_del, ep.o_ins, ep.e_ins = scoring
    return ep


class Pool:
    """jobs of one scoring and opt_w with their reads, as one batch: job k reads read k"""

    def __init__(self, dev, jobs, scoring, opt_w, stride):
        t = dev.torch
        self.jobs, self.scoring, self.opt_w, self.stride = list(jobs), scoring, opt_w, stride
        lens = np.array([len(j.read) for j in self.jobs], np.int64)
        self.reads = t.from_numpy(np.frombuffer(b"".join(j.read for j in self.jobs), np.uint8).copy()).cuda()
        self.offs = t.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)).cuda()
        self.lens = t.from_numpy(lens.astype(np.int32)).cuda()
        b = cc.batch_of(self.jobs[0])
        self.regs_np = cc.regs_of(b, self.jobs, stride=stride, read_of=list(range(len(self.jobs))))
        self.regs = t.from_numpy(self.regs_np).cuda()


class Device:
    """the library, a stand-in FM index that carries the table's 2-bit text (the kernels read nothing else of an index), and the pools on the device"""

    def __init__(self):
        import torch
        import bwamem_hip as B
        assert torch.cuda.is_available(), "these tests need a GPU"
        self.torch, self.B = torch, B
        self.L = B.load_library()                                   # raises if the HIP extension is missing: no fallback
        _, idx = common.genome_and_index(2_000, seed=1)
        self.dindex = B.Index.upload(idx, pac=cc.PAC.copy(), l_pac=cc.L_PAC)
        self.pools = {}

    def pool(self, key, jobs, scoring, opt_w, stride):
        if key not in self.pools:
            self.pools[key] = Pool(self, jobs, scoring, opt_w, stride)
        return self.pools[key]

    def batch_pool(self, name):
        b = cc.batches()[name]
        return self.pool(("batch", name), b.jobs, b.scoring, b.opt_w, b.stride)

    def run(self, pool, first=0, n=None, sel=None, max_cigar=MAX_CIGAR, md_cap=MD_CAP, stream=None):
        """bmh_cigar_batch on the records [first, first + n) of a pool (or on the records sel names) -> (cigar uint32 [n, max_cigar], aln int32 [n, 8], md uint8
        [n, md_cap]).  The output arrays are prefilled with a sentinel and have one slot more than the batch has jobs: it must come back untouched."""
        t = self.torch
        n = (len(pool.jobs) - first if sel is None else len(sel)) if n is None else n
        cg = t.full(((n + 1) * max_cigar,), SENT32, dtype=t.int32, device="cuda")
        aln = t.full(((n + 1) * 8,), SENT32, dtype=t.int32, device="cuda")
        md = t.full(((n + 1) * md_cap,), SENT8, dtype=t.uint8, device="cuda")
        sel_t = t.from_numpy(np.asarray(sel, np.int32)).cuda() if sel is not None else None
        t.cuda.synchronize()
        ep = ext_params(pool.scoring)
        rc = self.L.bmh_cigar_batch(self.dindex.handle, pool.reads.data_ptr(), pool.offs.data_ptr(), pool.lens.data_ptr(),
                                    pool.regs.data_ptr() + 4 * pool.stride * first, pool.stride, sel_t.data_ptr() if sel_t is not None else None, n, C.byref(ep), pool.opt_w,
                                    max_cigar, cg.data_ptr(), aln.data_ptr(), md_cap, md.data_ptr(), stream.cuda_stream if stream is not None else None)
        assert rc == 0, self.L.bmh_last_error()
        t.cuda.synchronize()
        cg, aln, md = cg.cpu().numpy().view(np.uint32).reshape(n + 1, max_cigar), aln.cpu().numpy().reshape(n + 1, 8), md.cpu().numpy().reshape(n + 1, md_cap)
        assert (cg[n] == SENT32).all() and (aln[n] == SENT32).all() and (md[n] == SENT8).all(), "the slot past the batch was written"
        return cg[:n], aln[:n], md[:n]

    def free(self):
        self.pools = {}
        self.dindex.free()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.free()


@pytest.fixture(scope="module")
def want(oracle, golden):  # noqa: F811
    return expected_rows(oracle, golden)


def row_error(j, w, cg, aln, md, flags=0):
    """None where the device's row of job j is the expected one, else what differs.  w: the expected row (None for a region the reference rejects: the
    flag-2 row); flags != 0: the job does not fit its slots, and the flag word is all that is expected"""
    if w is None:
        if list(aln) != [0, 0, 0, 0, -1, 0, 0, 2] or md[0] != 0:
            return f"flag-2 row {list(aln)} md[0] {md[0]}"
        return None
    if flags:
        return None if aln[7] == flags else f"flags {aln[7]} != {flags}"
    pos = int(np.uint32(aln[0])) | int(aln[1]) << 32
    got = (pos, int(aln[2]), int(aln[3]), int(aln[4]), int(aln[5]), int(aln[6]), int(aln[7]))
    exp = (w["pos"], w["is_rev"], len(w["cigar"]), w["NM"], w["score"], len(w["MD"]), 0)
    if got != exp:
        return f"(pos, is_rev, n_cigar, NM, score, md_len, flags) {got} != {exp}"
    if not np.array_equal(cg[:len(w["cigar"])], w["cigar"]):
        return f"cigar {cg[:len(w['cigar'])]} != {w['cigar']}"
    if md[:len(w["MD"])].tobytes() != w["MD"].encode() or md[len(w["MD"])] != 0:
        return f"MD {md[:len(w['MD']) + 1].tobytes()} != {w['MD']}"
    return None


def assert_rows(jobs, want, out, what, flags_of=None):  # noqa: F811
    cg, aln, md = out
    assert len(aln) == len(jobs)
    bad = []
    for k, j in enumerate(jobs):
        e = row_error(j, want.get(cc.key_of(j)), cg[k], aln[k], md[k], flags_of(j) if flags_of else 0)
        if e:
            bad.append((cc.key_of(j), j.route, e))
    assert not bad, (what, len(bad), bad[:4])


def groups():
    """(scoring, opt_w) -> the jobs of the whole table under it, in table order"""
    out = {}
    for b in cc.batches().values():
        out.setdefault((b.scoring, b.opt_w), []).extend(b.jobs)
    return out


GROUPS = groups()
GROUP_IDS = ["-".join(map(str, s)) + f"-w{w}" for s, w in GROUPS]


def native_stride(jobs, opt_w):
    return 8 if all(j.reg_w == opt_w for j in jobs) else 16


@pytest.mark.parametrize("name", cc.batch_names())
def test_each_batch_equals_the_reference_fixture(dev, want, name):
    b = cc.batches()[name]
    kinds = [j.route[3] for j in b.jobs]
    print(f"{name}: {b.n} jobs, stride {b.stride}, opt_w {b.opt_w}: " + ", ".join(f"{k} {kinds.count(k)}" for k in cc.KINDS if k in kinds))
    assert_rows(b.jobs, want, dev.run(dev.batch_pool(name)), name)


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_a_jobs_row_does_not_depend_on_its_batch(dev, want, key):
    """alone, in one shuffled batch of everything under the scoring and opt_w (long and short regions together: long_split, max_len and the LDS / slab choice
    change), through a sel list in reverse order, as records of 16 words"""
    scoring, opt_w = key
    jobs = GROUPS[key]
    stride = native_stride(jobs, opt_w)
    pool = dev.pool(("group", key, stride), jobs, scoring, opt_w, stride)
    for k, j in enumerate(jobs):
        assert_rows([j], want, dev.run(pool, first=k, n=1), "alone")
    order = np.random.default_rng(len(jobs)).permutation(len(jobs))
    shuffled = [jobs[k] for k in order]
    assert_rows(shuffled, want, dev.run(dev.pool(("shuffled", key, stride), shuffled, scoring, opt_w, stride)), "shuffled")
    sel = list(range(len(jobs)))[::-1]
    assert_rows([jobs[k] for k in sel], want, dev.run(pool, sel=sel), "sel, reversed")
    sel = [int(k) for k in order[: max(1, len(jobs) // 3)]]
    assert_rows([jobs[k] for k in sel], want, dev.run(pool, sel=sel), "sel, a third")
    pool16 = dev.pool(("group", key, 16), jobs, scoring, opt_w, 16)
    assert (pool16.regs_np[:, 1] == 7).all()                        # (the score word of a record of 16 is not truesc)
    assert_rows(jobs, want, dev.run(pool16), "stride 16")
    if key == (cc.DEFAULT, 100):
        n_long = sum(1 for j in jobs if cc.is_long(j.qe - j.qb, j.re - j.rb))
        assert 10 <= n_long <= len(jobs) // 4 and stride == 16


def of_kind(jobs, kind, m):
    out = [j for j in jobs if j.route[3] == kind][:m]
    assert len(out) == m
    return out


def stats_counts(dev, capfd, pool, **kw):
    """bmh_cigar_batch with BMH_CIGAR_STATS set for the call -> (the result, the six list counts of its [cigar] line)"""
    capfd.readouterr()
    os.environ["BMH_CIGAR_STATS"] = "1"
    try:
        out = dev.run(pool, **kw)
    finally:
        del os.environ["BMH_CIGAR_STATS"]
    err = capfd.readouterr().err
    m = re.findall(r"\[cigar\] (\d+) regions: band<=32 (\d+), <=48 (\d+), <=80 (\d+), <=160 (\d+), <=256 (\d+), wide/other (\d+);", err)
    assert len(m) == 1, err
    return out, int(m[0][0]), tuple(int(x) for x in m[0][1:])


@pytest.mark.parametrize("m", [1, 3, 4, 5])
def test_lists_that_do_not_fill_a_wave(dev, want, capfd, m):
    """m jobs of every kind: cigar_dp16_kernel takes four regions a wave"""
    jobs = GROUPS[(cc.DEFAULT, 100)]
    pick = [j for kind in ("F2", "F3", "F5", "F10", "F16", "slow", "trivial") for j in of_kind(jobs, kind, m)]
    pool = dev.pool(("tails", m), pick, cc.DEFAULT, 100, native_stride(pick, 100))
    out, n, counts = stats_counts(dev, capfd, pool)
    assert n == 7 * m and counts == (m,) * 6 == cc.class_counts(pick, cc.DEFAULT, 100)
    assert_rows(pick, want, out, f"lists of {m}")


@pytest.mark.parametrize("n", [15, 16, 17])
def test_batches_around_a_block_of_the_finish_kernel(dev, want, n):
    """cigar_finish_kernel: sixteen regions a block"""
    pool = dev.batch_pool("trace")
    for first in (0, 40):
        assert_rows(pool.jobs[first:first + n], want, dev.run(pool, first=first, n=n), f"n = {n}")


def test_class_counts_equal_the_restated_classifier(dev, want, capfd):
    """ties the routing restated in cigar_cases to what the device did: the list counts cigar_classify_kernel left, per batch"""
    total = np.zeros(6, np.int64)
    for name, b in cc.batches().items():
        out, n, counts = stats_counts(dev, capfd, dev.batch_pool(name))
        exp = cc.class_counts(b.jobs, b.scoring, b.opt_w)
        print(f"{name}: {n} regions, lists (F2, F3, F5, F10, F16, slow) {counts}")
        assert n == b.n and counts == exp, (name, counts, exp)
        assert_rows(b.jobs, want, out, name)
        total += counts
    assert (total > 0).all()
    # read per call: without the variable nothing is printed
    capfd.readouterr()
    dev.run(dev.batch_pool("kinds"))
    assert "[cigar]" not in capfd.readouterr().err


def test_scratch_reuse_in_reverse_order_and_on_a_second_stream(dev, want):
    """one scratch per stream, grown and never cleared: the long batches leave direction matrices, lists and slabs behind that the small ones after them lie in"""
    names = list(cc.batch_names())
    assert names.index("long") < len(names) - 5
    for order in (names, names[::-1]):
        for name in order:
            assert_rows(cc.batches()[name].jobs, want, dev.run(dev.batch_pool(name)), name + (" reversed" if order is not names else ""))
    s = dev.torch.cuda.Stream()
    try:
        for name in names[::-1] + names[:3]:
            assert_rows(cc.batches()[name].jobs, want, dev.run(dev.batch_pool(name), stream=s), name + " on a second stream")
    finally:
        s.synchronize()
        dev.L.bmh_cigar_release(C.c_void_p(s.cuda_stream))
    assert_rows(cc.batches()["kinds"].jobs, want, dev.run(dev.batch_pool("kinds")), "after the release")


def slot_flags(b):
    return lambda j: j.extra["small"]


def test_slots(dev, want, golden):  # noqa: F811
    """family e at max_cigar 16 and md_cap 24: flag 1 / flag 8 on exactly the jobs the table names, exact rows for their neighbours in the same wave; the same jobs
    with large slots give the fixture's rows (test_each_batch_equals_the_reference_fixture)"""
    b = cc.batches()["slots"]
    flags = [j.extra["small"] for j in b.jobs]
    assert flags == [small_flags(b, j, golden[cc.key_of(j)]) for j in b.jobs] and {0, 1, 8} == set(flags)
    pool = dev.batch_pool("slots")
    out = dev.run(pool, max_cigar=b.max_cigar, md_cap=b.md_cap)
    assert [int(f) for f in out[1][:, 7]] == flags
    assert_rows(b.jobs, want, out, "small slots", flags_of=slot_flags(b))
    # each one alone as well, and with room for the operations but not for the MD string (and the other way round)
    for k, j in enumerate(b.jobs):
        assert_rows([j], want, dev.run(pool, first=k, n=1, max_cigar=b.max_cigar, md_cap=b.md_cap), "small slots, alone", flags_of=slot_flags(b))
    assert_rows(b.jobs, want, dev.run(pool, max_cigar=MAX_CIGAR, md_cap=b.md_cap), "small MD", flags_of=lambda j: j.extra["small"] & 8)
    assert_rows(b.jobs, want, dev.run(pool, max_cigar=b.max_cigar, md_cap=MD_CAP), "small CIGAR", flags_of=lambda j: j.extra["small"] & 1)


def child_main():
    """the whole table in a process of its own (BMH_CIGAR_SLOW is read once per process): every batch, and the slots batch with its small slots"""
    import oracle_py
    assert os.environ.get("BMH_CIGAR_SLOW") == "1"
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cigar_cases.npz"))
    assert str(z["digest"]) == cc.digest()
    want_ = expected_rows(oracle_py.Oracle(), cc.unpack_rows(z))
    d = Device()
    n = 0
    try:
        for name, b in cc.batches().items():
            assert_rows(b.jobs, want_, d.run(d.batch_pool(name)), name + " (wave-per-region forms only)")
            n += b.n
        b = cc.batches()["slots"]
        assert_rows(b.jobs, want_, d.run(d.batch_pool("slots"), max_cigar=b.max_cigar, md_cap=b.md_cap), "small slots (wave-per-region forms only)", flags_of=slot_flags(b))
        for key, jobs in GROUPS.items():
            stride = native_stride(jobs, key[1])
            assert_rows(jobs, want_, d.run(d.pool(("group", key), jobs, key[0], key[1], stride)), "group (wave-per-region forms only)")
    finally:
        d.free()
    print(f"slow-only ok: {n} jobs")


def test_the_wave_per_region_forms_alone(dev):
    """BMH_CIGAR_SLOW=1 in a fresh child process: no classifier, no fast path -- every job goes through cigar_kernel<C, CLO> or the long form, and the child
    compares the same rows"""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, BMH_CIGAR_SLOW="1")
    env.pop("BMH_CIGAR_STATS", None)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(root, "bwa-mem_gpu_amd"), os.path.join(root, "oracle"), here] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-500:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"slow-only ok: {len(cc.all_jobs())} jobs" in r.stdout


if __name__ == "__main__":
    child_main()
