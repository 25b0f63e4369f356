"""The region tail on the hand-made cases of tests/regs_cases.py, without a GPU: the host form bmh_finalize_regs (csrc/regs_post.cpp; 1 and 4 threads)
against the CPU build of the device core (csrc/regs_core.h behind tests/regs_core_host.cpp) record for record, what every case is about (`must`), and
the host form against the reference's own mem_sort_dedup_patch / mem_mark_primary_se / mem_approx_mapq_se (oracle/ref_tail_harness.cpp) where that
library was built.  All comparisons are exact."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import common
import regs_cases
from bwamem_hip.lib import ChainOpt, ExtParams, PostOpt, load_library
from test_regs_core import core_lib


def options(case):
    """(ChainOpt, ExtParams, PostOpt) of a case; the ALT table (kept alive by the case) goes into both option structs"""
    L = load_library()
    co = ChainOpt(); L.bmh_chain_opt_default(C.byref(co))
    ep = ExtParams.default()
    po = PostOpt(); L.bmh_post_opt_default(C.byref(po))
    for s, over in ((co, case.co), (ep, case.ep), (po, case.po)):
        for k, v in over.items():
            setattr(s, k, v)
    if case.is_alt is not None:
        co.contig_is_alt = po.contig_is_alt = case.is_alt.ctypes.data_as(C.c_void_p).value
    return co, ep, po


def host_arrays(case):
    flat, offs, _ = common.ragged_reads(case.reads) if case.reads else (np.zeros(0, np.uint8), np.zeros(0, np.uint64), None)
    ctg_off = None
    if case.contigs and len(case.contigs) > 1:
        ctg_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([c[1] for c in case.contigs])[:-1]]), dtype=np.int64)
    return np.ascontiguousarray(flat, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint64), ctg_off


def run_cpu(fn, case, last, regs=None, rpr=None, reads=None, id0=None):
    """fn = bmh_finalize_regs (last: threads) or an entry of tests/regs_core_host.cpp (last: with_dp) on a case -> (records [m, 16], out_per_read) or the error code"""
    co, ep, po = options(case)
    if id0 is not None:
        po.id0 = id0
    flat, offs, ctg_off = host_arrays(case) if reads is None else reads
    regs = case.regs if regs is None else regs
    rpr = case.rpr if rpr is None else rpr
    fr = case.frac_rep if len(rpr) == len(case.frac_rep) else np.zeros(len(rpr), np.float32)
    n = len(rpr)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.full((max(len(regs), 1), 16), -3, np.int32); opr = np.zeros(max(n, 1), np.uint32)
    fn.restype = C.c_int64
    fn.argtypes = None
    nct = len(case.contigs) if ctg_off is not None else 1
    m = fn(C.byref(co), C.byref(ep), C.byref(po), C.c_int64(regs_cases.L_PAC), p(case.pac), C.c_uint32(n), p(flat), p(offs), p(regs), p(rpr), p(fr),
           C.c_int(nct), p(ctg_off) if ctg_off is not None else None, p(out), p(opr), C.c_int(last))
    if m < 0:
        return int(m)
    return out[:m].copy(), opr[:n].copy()


def result_of(case, out, opr):
    s = np.concatenate([[0], np.cumsum(opr.astype(np.int64))])
    return SimpleNamespace(case=case, out=out, opr=opr, per_read=[out[s[r]:s[r + 1]] for r in range(len(opr))])


_host = {}


def host_result(name):
    """bmh_finalize_regs on a case with one thread, computed once"""
    if name not in _host:
        case = regs_cases.get(name)
        got = run_cpu(load_library().bmh_finalize_regs, case, 1)
        assert not isinstance(got, int), got
        _host[name] = result_of(case, *got)
    return _host[name]


def check_must(case, res):
    assert case.must
    for what, v in case.must.items():
        assert (v(res) if callable(v) else v), (case.name, what)


def test_the_cases_cover_every_family_and_size():
    cases = regs_cases.all_cases()
    assert tuple(cases) == regs_cases.NAMES
    fam = {f for c in cases.values() for f in c.families}
    assert fam == {"scattered", "ties", "wide", "collision", "tandem", "patch", "mark", "emit", "contigs", "alt"}
    for f in ("scattered", "ties", "tandem", "contigs"):
        sizes = {int(n) for c in cases.values() if f in c.families for n in c.rpr}
        assert sizes >= set(regs_cases.SIZES), (f, sorted(set(regs_cases.SIZES) - sizes))
    c = cases["scattered_class2_empty"]
    assert {regs_cases.fin_class(int(n)) for n in c.rpr if n > regs_cases.FIN_NL} == {0, 1, 3, 4}


@pytest.mark.parametrize("name", regs_cases.NAMES)
def test_host_form_equals_the_core_and_the_case_holds(name):
    case = regs_cases.get(name)
    res = host_result(name)
    L = load_library()
    got4 = run_cpu(L.bmh_finalize_regs, case, 4)
    assert np.array_equal(got4[1], res.opr) and np.array_equal(got4[0], res.out)
    core = run_cpu(core_lib().regs_core_run, case, 1)
    if case.core_error:
        assert core == case.core_error
    else:
        assert np.array_equal(core[1], res.opr)
        assert np.array_equal(core[0], res.out), np.nonzero((core[0] != res.out).any(1))[0][:5]
    assert (res.out[:, 0] == np.repeat(np.arange(len(res.opr)), res.opr.astype(np.int64))).all()
    check_must(case, res)


@pytest.fixture(scope="module")
def ref_tail():
    import oracle_py
    oracle_py.build(ref=True)
    if not oracle_py.RefTail.available():
        pytest.skip("oracle/_ref/libref_tail.so not built (needs the reference's sources)")
    return oracle_py.RefTail()


@pytest.mark.parametrize("name", regs_cases.NAMES)
def test_host_form_equals_the_reference_tail(ref_tail, name):
    """Per read: the reference's three functions on the same regions.  Same order, fields [1]..[12] (with an ALT table [11] is secondary_all, and is_alt /
    alt_sc ride in [15]), and the MAPQ of every record with secondary < 0 after the cap of mem_reg2sam (src/bwamem.c:1737-1757) restated here."""
    case = regs_cases.get(name)
    res = host_result(name)
    co, ep, po = options(case)
    opt_i = (ep.a, ep.b, ep.o_del, ep.e_del, ep.o_ins, ep.e_ins, co.w, co.min_seed_len, co.max_chain_gap, po.mapQ_coef_fac)
    opt_f = (co.mask_level, po.mask_level_redun, po.mapQ_coef_len)
    score, qb, qe, rb, re, _ = regs_cases.fields(case)
    rid = regs_cases.rid_of(case, rb, re)
    alt_mode = case.is_alt is not None
    for r, sl in enumerate(regs_cases.read_slices(case)):
        ia = case.is_alt[rid[sl]] if alt_mode else None
        want = ref_tail.run(opt_i, opt_f, regs_cases.L_PAC, case.pac, case.reads[r], po.id0 + r, float(case.frac_rep[r]), case.regs[sl], rid[sl], ia)
        got = res.per_read[r]
        assert len(got) == len(want), (name, r)
        if not len(got):
            continue
        assert np.array_equal(got[:, 1:11], want[:, 1:11]), (name, r, np.nonzero((got[:, 1:11] != want[:, 1:11]).any(1))[0][:5])
        assert np.array_equal(got[:, 12], want[:, 12]), (name, r)
        assert np.array_equal(got[:, 11], want[:, 14] if alt_mode else want[:, 11]), (name, r)
        if alt_mode:
            assert np.array_equal(got[:, 15] >> 1, (want[:, 15] & 1) | (want[:, 15] >> 2 << 1)), (name, r)
        # the selection and the cap of mem_reg2sam on the reference's records
        mapq = want[:, 13].copy()
        l, first = 0, 0
        for k in range(len(want)):
            p = want[k]
            if p[1] < po.T:
                continue
            if p[12] >= 0 and ((p[15] & 1) or not po.flag_all):
                continue
            if 0 <= p[12] < 0x7FFFFFFF and p[1] < want[p[12], 1] * np.float32(co.drop_ratio):
                continue
            if l and not (p[15] & 1) and mapq[k] > mapq[first]:
                mapq[k] = mapq[first]
            if l == 0:
                first = k
            l += 1
        pri = want[:, 12] < 0
        assert np.array_equal(got[pri, 13], mapq[pri]), (name, r)
