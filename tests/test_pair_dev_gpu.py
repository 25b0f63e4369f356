"""The device's pairing stage on its own (csrc/pair_dev.hip): pair_kernel against the host walk of csrc/pair_post.cpp, record for record, on the hand-made
regions of tests/pair_cases.py; the hand-back of pair scores too close to an integer; the merge of the host's records and the scan against numpy.
Everything is exact equality."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

import pair_cases as pc

pytestmark = pytest.mark.gpu

SENT = -0x12345678


@pytest.fixture(scope="module")
def dev():
    import torch
    import bwamem_hip as B
    from bwamem_hip import fmindex
    lib = B.load_library()
    vp, u32, i64 = C.c_void_p, C.c_uint32, C.c_int64
    lib.bmh_pair_limit.restype = C.c_int; lib.bmh_pair_limit.argtypes = []
    lib.bmh_pairs_device_records.restype = i64
    lib.bmh_pairs_device_records.argtypes = [vp] * 6 + [vp, vp, u32, vp, C.c_uint64, vp, vp, C.c_int, vp] + [vp] * 8
    lib.bmh_pair_merge_counts.restype = C.c_int; lib.bmh_pair_merge_counts.argtypes = [u32, vp, u32] + [vp] * 11
    lib.bmh_pair_merge_records.restype = C.c_int; lib.bmh_pair_merge_records.argtypes = [u32] + [vp] * 9
    lib.bmh_pair_scan_bytes.restype = C.c_size_t; lib.bmh_pair_scan_bytes.argtypes = [u32]
    lib.bmh_pair_scan.restype = C.c_int; lib.bmh_pair_scan.argtypes = [vp, vp, u32, vp, C.c_size_t, vp]
    g = pc.genome()
    dindex = B.Index.upload(fmindex.build_fmd_index(g), pac=pc.pack_pac(g), l_pac=pc.L_PAC)
    yield SimpleNamespace(torch=torch, lib=lib, index=dindex, B=B)
    dindex.free()


def up(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def device_records(dev, opt, regs, rpr, frac, reads, pes):
    """bmh_pairs_device_records on host arrays -> (m, fin [m, 16], opr, off, h_rec, unflag, todo) as numpy arrays."""
    from bwamem_hip import synth
    torch, lib = dev.torch, dev.lib
    n, nr = len(rpr), len(regs)
    d_reads = up(torch, synth.codes_to_ascii(reads.reshape(-1)))
    d_offs = up(torch, (np.arange(n, dtype=np.int64) * pc.L).astype(np.int32))
    d_regs = up(torch, regs if nr else np.zeros((1, 8), np.int32))
    d_rpr, d_frac = up(torch, rpr.astype(np.uint32)), up(torch, frac.astype(np.float32))
    full = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")
    d_fin, d_dedup = full((nr + 1, 16), torch.int32, SENT), full((nr + 1, 16), torch.int32, SENT)
    d_opr, d_off, d_h, d_uf = (full((n + 1,), torch.int32, SENT) for _ in range(4))
    d_todo = full((n // 2 + 1,), torch.uint8, 0xEE)
    ctg = np.array(pc.CTG_OFF, np.int64) if opt.contigs else None
    pes = np.ascontiguousarray(pes, dtype=np.float64)
    torch.cuda.synchronize()
    m = lib.bmh_pairs_device_records(dev.index.handle, C.byref(opt.co), C.byref(opt.ep), C.byref(opt.po), C.byref(opt.pe), pes.ctypes.data,
                                     d_reads.data_ptr(), d_offs.data_ptr(), n, d_regs.data_ptr(), nr, d_rpr.data_ptr(), d_frac.data_ptr(),
                                     len(opt.contigs) if opt.contigs else 1, ctg.ctypes.data if ctg is not None else None,
                                     d_fin.data_ptr(), d_dedup.data_ptr(), d_opr.data_ptr(), d_off.data_ptr(), d_h.data_ptr(), d_uf.data_ptr(), d_todo.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert m >= 0, dev.B.lib._err(lib)
    fin = d_fin.cpu().numpy()
    assert (fin[m:] == SENT).all() and d_todo.cpu().numpy()[n // 2] == 0xEE
    return SimpleNamespace(m=int(m), fin=fin[:m], opr=d_opr.cpu().numpy()[:n].view(np.uint32), off=d_off.cpu().numpy()[:n].view(np.uint32), h=d_h.cpu().numpy()[:n],
                           uf=d_uf.cpu().numpy()[:n], todo=d_todo.cpu().numpy()[:n // 2])


@pytest.mark.parametrize("name", list(pc.CONFIGS))
def test_pair_kernel_equals_host_walk(dev, name):
    """Per configuration: the device's records, h_rec and unflag of every pair it keeps equal the host walk's, int for int; it hands back exactly the pairs
    beyond its limit of hits, and none for a score near an integer (tests/test_pair_dev.py keeps the scores 1e-4 away).  A pair with a hit on an ALT
    sequence stays the device's: todo is 0 or 2 there as everywhere.  (The hand-back for n_sub + 1 >= n_log takes 65 535 candidates: out of reach.)"""
    g = pc.case(name)
    d = device_records(dev, g.opt, g.regs, g.rpr, g.frac, g.reads, g.pes)
    assert d.m == len(g.fin)
    assert np.array_equal(d.opr, g.per_read)
    assert np.array_equal(d.off.astype(np.int64), g.off[:-1])
    lim = dev.lib.bmh_pair_limit()
    assert lim == 64
    n_both = g.per_read[0::2].astype(np.int64) + g.per_read[1::2]
    print(name, "pairs", g.n_pairs, "todo", np.bincount(d.todo, minlength=3).tolist())
    assert np.array_equal(d.todo == 2, n_both > lim), (np.nonzero(d.todo == 2)[0], np.nonzero(n_both > lim)[0])
    assert not (d.todo == 1).any() and set(np.unique(d.todo).tolist()) <= {0, 2}
    assert (n_both > lim).sum() >= 8 and (n_both == lim).sum() >= 8
    bad = []
    for p in np.nonzero(d.todo == 0)[0]:
        lo, hi = g.off[2 * p], g.off[2 * p + 2]
        if not (np.array_equal(d.fin[lo:hi], g.fin[lo:hi]) and np.array_equal(d.h[2 * p:2 * p + 2], g.h_rec[2 * p:2 * p + 2]) and np.array_equal(d.uf[2 * p:2 * p + 2], g.unflag[2 * p:2 * p + 2])):
            bad.append(int(p))
    for p in bad[:6]:
        lo, hi = g.off[2 * p], g.off[2 * p + 2]
        print("pair", p, "built as", g.intent[p], "took", sorted(g.labels[p]), "h_rec", d.h[2 * p:2 * p + 2], g.h_rec[2 * p:2 * p + 2], "unflag", d.uf[2 * p:2 * p + 2], g.unflag[2 * p:2 * p + 2])
        print(" device:\n", d.fin[lo:hi], "\n host:\n", g.fin[lo:hi])
    assert not bad, (len(bad), sorted({g.intent[p] for p in bad}), sorted(set().union(*[g.labels[p] for p in bad])))


def near_integer_avg(target_frac):
    """The mean insert for which a 100 + 100 pair at distance 330 (std 30) scores 198 + target_frac before truncation: by bisection (the score grows with the mean below 330)."""
    def val(avg):
        ns = (330 - avg) / 30.
        return 200. + .721 * math.log(2. * math.erfc(abs(ns) * math.sqrt(0.5))) * 1 + .499
    lo, hi = 250., 265.
    assert val(lo) < 198 + target_frac < val(hi)
    for _ in range(200):
        mid = .5 * (lo + hi)
        if val(mid) < 198 + target_frac:
            lo = mid
        else:
            hi = mid
    return hi, val(hi)


def test_pair_kernel_hands_back_scores_near_an_integer(dev):
    """Statistics set by hand (there is no host reference: the host computes its own): scores 3e-7 above and below an integer go back to the host (todo 1), a
    score 1e-4 above one stays, with the record choice and the proper-pair flag of the restatement."""
    opt = pc.options("default")
    rng = np.random.default_rng(5)
    n_pairs = 301
    rows, P = [], rng.integers(1000, 60_000, size=n_pairs)
    for p in range(n_pairs):
        for r, (sc, qb, qe, rb, re) in enumerate((pc.fwd(P[p], 100), pc.rev(P[p] + 330 - (pc.L - 1), 100))):
            rows.append([2 * p + r, sc, qb, qe, rb & 0xFFFFFFFF, rb >> 32, re & 0xFFFFFFFF, re >> 32])
    regs = np.array(rows, np.int64).astype(np.uint32).view(np.int32).reshape(-1, 8)
    rpr = np.ones(2 * n_pairs, np.uint32); frac = np.zeros(2 * n_pairs, np.float32)
    reads = rng.integers(0, 4, size=(2 * n_pairs, pc.L)).astype(np.uint8)
    for target, want_todo in ((3e-7, 1), (-3e-7, 1), (1e-4, 0)):
        avg, v = near_integer_avg(target)
        assert abs(v - (198 + target)) < 2e-8, (avg, v)
        pes = np.array([[0, 0, 1, 0, 0], [1, 1000, 0, avg, 30.], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]], np.float64)
        d = device_records(dev, opt, regs, rpr, frac, reads, pes)
        print("avg", repr(avg), "score", repr(v), "todo", np.bincount(d.todo, minlength=3).tolist())
        assert (d.todo == want_todo).all(), np.bincount(d.todo)
        if want_todo == 0:
            po = pc.plain_opt(opt)
            for p in range(n_pairs):
                R = pc.restate_pair([[pc.hit_of(d.fin[2 * p])], [pc.hit_of(d.fin[2 * p + 1])]], pes, po, p, 0., 0.)
                assert R.paired and R.proper and R.o == 198 and len(R.cands) == 1
                assert d.h[2 * p:2 * p + 2].tolist() == R.z == [0, 0] and (d.uf[2 * p:2 * p + 2] == 0).all()
                assert d.fin[2 * p, 14] == 0x43 and d.fin[2 * p + 1, 14] == 0x83 and (d.fin[2 * p:2 * p + 2, 15] & 1).all()


def scan_dev(dev, a, in_place=False):
    torch, lib = dev.torch, dev.lib
    n = len(a)
    d_in = up(torch, a)
    d_out = d_in if in_place else torch.full((n + 1,), SENT, dtype=torch.int32, device="cuda")
    tb = lib.bmh_pair_scan_bytes(n)
    tmp = torch.empty(max(int(tb), 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.bmh_pair_scan(d_in.data_ptr(), d_out.data_ptr(), n, tmp.data_ptr(), tb, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert in_place or out[n] == SENT
    return out[:n].view(np.uint32)


def test_pair_merge_and_scan_equal_numpy(dev):
    """The host's records take their places among the device's (pair_scatter_slot_kernel, pair_counts_kernel, the scan, pair_merge_kernel) as a numpy gather says."""
    torch, lib = dev.torch, dev.lib
    rng = np.random.default_rng(11)
    for n in (1, 2, 255, 256, 257, 100_003):
        a = rng.integers(0, 6, size=n).astype(np.uint32)
        want = (np.cumsum(a) - a).astype(np.uint32)
        assert np.array_equal(scan_dev(dev, a), want), n
        assert np.array_equal(scan_dev(dev, a, in_place=True), want), n      # (the mate rescue's kernels scan in place)
    n_pairs = 1003; n = 2 * n_pairs
    st = torch.cuda.current_stream().cuda_stream
    opr_dev = rng.integers(0, 6, size=n).astype(np.uint32)
    off_dev = (np.cumsum(opr_dev) - opr_dev).astype(np.uint32)
    fin_dev = rng.integers(-2**31, 2**31, size=(int(opr_dev.sum()), 16)).astype(np.int32)
    h_dev, uf_dev = rng.integers(-1, 5, size=n).astype(np.int32), rng.integers(0, 256, size=n).astype(np.int32)
    tenth = np.unique(np.concatenate([[0, n_pairs - 1], rng.choice(n_pairs, n_pairs // 10, replace=False)])).astype(np.uint32)
    for todo in (np.zeros(0, np.uint32), np.arange(n_pairs, dtype=np.uint32), tenth):
        nt = len(todo)
        opr_h = rng.integers(0, 6, size=2 * nt).astype(np.uint32)
        off_h = (np.cumsum(opr_h) - opr_h).astype(np.uint32)
        fin_h = rng.integers(-2**31, 2**31, size=(int(opr_h.sum()), 16)).astype(np.int32)
        h_h, uf_h = rng.integers(-1, 5, size=2 * nt).astype(np.int32), rng.integers(256, 512, size=2 * nt).astype(np.int32)
        # numpy: every read's place, then a gather
        slot = np.full(n, -1, np.int32)
        slot[2 * todo] = 2 * np.arange(nt); slot[2 * todo + 1] = 2 * np.arange(nt) + 1
        s = np.maximum(slot, 0)
        pick = lambda hst, dv: np.where(slot >= 0, hst[s] if nt else dv, dv)
        opr = pick(opr_h, opr_dev).astype(np.uint32); h = pick(h_h, h_dev); uf = pick(uf_h, uf_dev)
        off = (np.cumsum(opr) - opr).astype(np.uint32)
        parts = [(fin_h[off_h[slot[r]]:off_h[slot[r]] + opr[r]] if slot[r] >= 0 else fin_dev[off_dev[r]:off_dev[r] + opr[r]]) for r in range(n)]
        fin = np.concatenate(parts) if parts else np.zeros((0, 16), np.int32)
        total = int(opr.sum())
        assert len(fin) == total
        pad = lambda a_, shape: a_ if len(a_) else np.zeros(shape, a_.dtype)
        D = {k: up(torch, v) for k, v in dict(todo=pad(todo, 1), opr_dev=opr_dev, off_dev=off_dev, fin_dev=pad(fin_dev, (1, 16)), h_dev=h_dev, uf_dev=uf_dev, opr_h=pad(opr_h, 1),
                                              off_h=pad(off_h, 1), fin_h=pad(fin_h, (1, 16)), h_h=pad(h_h, 1), uf_h=pad(uf_h, 1)).items()}
        O = {k: torch.full((n + 1,), SENT, dtype=torch.int32, device="cuda") for k in ("slot", "opr", "h", "uf", "off")}
        d_fin = torch.full((total + 8, 16), SENT, dtype=torch.int32, device="cuda")
        tb = lib.bmh_pair_scan_bytes(n)
        tmp = torch.empty(int(tb), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        P = lambda t: t.data_ptr()
        assert lib.bmh_pair_merge_counts(n, P(D["todo"]), nt, P(O["slot"]), P(D["opr_dev"]), P(D["h_dev"]), P(D["uf_dev"]), P(D["opr_h"]), P(D["h_h"]), P(D["uf_h"]),
                                         P(O["opr"]), P(O["h"]), P(O["uf"]), st) == 0
        assert lib.bmh_pair_scan(P(O["opr"]), P(O["off"]), n, P(tmp), tb, st) == 0
        assert lib.bmh_pair_merge_records(n, P(O["slot"]), P(D["fin_dev"]), P(D["off_dev"]), P(D["fin_h"]), P(D["off_h"]), P(O["opr"]), P(O["off"]), P(d_fin), st) == 0
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in O.items()}
        for k, want in (("slot", slot), ("opr", opr.view(np.int32)), ("h", h), ("uf", uf), ("off", off.view(np.int32))):
            assert np.array_equal(got[k][:n], want), (nt, k)
            assert got[k][n] == SENT, (nt, k)
        gf = d_fin.cpu().numpy()
        assert np.array_equal(gf[:total], fin), nt
        assert (gf[total:] == SENT).all(), nt
