"""The device job builder's full case, shared by tests/test_gpu_parity.py and tests/test_chain_classes_gpu.py: reads -> seeds -> chains / jobs ->
extension -> regions on the device against the host job builder and the oracle."""
import numpy as np
import pytest

import common


def _to_dev(torch, a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dt is not None:
        t = t.view(dt) if t.dtype.itemsize == torch.empty(0, dtype=dt).element_size() else t.to(dt)
    return t.cuda()


def _pack_pac(g):
    pad = (-len(g)) % 4
    codes = np.concatenate([g, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    pac = ((codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([pac, np.zeros(1, np.uint8)]))      # + the .pac tail byte slot


def _device_chain_case(B, oracle, g, idx, reads, opt_over=None, heavy=None, scoring=False, sub=None, contigs=None, grid_max=None, on_counts=None):
    """reads -> bmh_seed_batch -> bmh_chain_batch -> bmh_extend_batch -> bmh_chain_merge, all in HBM, against the
    host job builder on the same seeds (byte-identical batch) and its merge of the oracle's extension results.
    contigs: [(name, length)], the sequences of the reference (device and host builder); grid_max: knob CHAIN_GRID_MAX, the blocks of the cooperative
    chaining kernels stride over their lists; on_counts(seeds, lens, counts): called with the host copy of the seeds and ChainWorkspace.class_counts()
    after each of the three chaining calls (the materialised batch, the bare descriptors, the one-call form)."""
    import ctypes as C, os, torch
    from bwamem_hip import synth
    from bwamem_hip.lib import ChainOpt, ChainWorkspace, HostJobs, dev_jobs_to_host, seeds_to_host, load_library
    if isinstance(reads, np.ndarray):
        n, L = reads.shape
        flat = np.ascontiguousarray(reads.reshape(-1))
        offs_h = np.arange(n, dtype=np.uint64) * L; lens_h = np.full(n, L, np.uint32)
    else:                                                    # ragged: a list of reads of different lengths
        flat, offs_h, lens_h = common.ragged_reads(reads)
        n = len(reads)
    dindex = B.Index.upload(idx, pac=_pack_pac(g), l_pac=len(g))
    ws = B.SeedWorkspace(n, max(int(flat.size), 1), max_cands=max(int(flat.size), 64), max_occ=1 << 22)
    r = _to_dev(torch, synth.codes_to_ascii(flat))
    o = torch.from_numpy(offs_h.astype(np.int64)).to(torch.int32).cuda()
    l = torch.from_numpy(lens_h.astype(np.int64)).to(torch.int32).cuda()
    s = ws.seed_batch(dindex, r, o, l, 19)
    opt = ChainOpt(); load_library().bmh_chain_opt_default(C.byref(opt))
    for k, v in (opt_over or {}).items():
        setattr(opt, k, v)
    cw = ChainWorkspace(n, max(int(s.n_seeds), 1), opt=opt)
    if contigs:
        cw.set_contigs(contigs)
    # scoring: the extension runs with the chain options' scores too (otherwise with the defaults, whatever opt_over says)
    ext_p = B.ExtParams(opt.a, opt.b, opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, 0, 5) if scoring else B.ExtParams.default()
    import oracle_py
    ksw_p = oracle_py.KswParams(ext_p.a, ext_p.b, ext_p.o_del, ext_p.e_del, ext_p.o_ins, ext_p.e_ins, 0, 5, 1)
    # heavy: reads with more sampled seeds than this leave the lane kernel; sub: mask of the classes (<= 16 / 32 / 64 entries) chained four reads per wave
    # (knob CHAIN_SUB; 0 = their round-5 forms: a lane per read over the class list, a wave per read)
    if heavy is not None:
        os.environ["BMH_CHAIN_HEAVY"] = str(heavy)
    if sub is not None:
        os.environ["BMH_CHAIN_SUB"] = str(sub)
    if grid_max is not None:
        load_library().bmh_tune_set(b"CHAIN_GRID_MAX", int(grid_max), 0)
    try:
        return _chain_case_body(B, oracle, g, flat, offs_h, lens_h, n, dindex, ws, cw, r, o, l, s, opt, ext_p, ksw_p, contigs, on_counts)
    finally:                                                 # (the knobs hold for every chaining call of the case)
        os.environ.pop("BMH_CHAIN_HEAVY", None)
        os.environ.pop("BMH_CHAIN_SUB", None)
        load_library().bmh_tune_set(b"CHAIN_GRID_MAX", 0, 1)


def _chain_case_body(B, oracle, g, flat, offs_h, lens_h, n, dindex, ws, cw, r, o, l, s, opt, ext_p, ksw_p, contigs, on_counts):
    import ctypes as C, torch
    from bwamem_hip.lib import HostJobs, dev_jobs_to_host, seeds_to_host, load_library
    seeds_h = seeds_to_host(s, n)
    dj = cw.chain_batch(dindex, r, o, l, s)
    if on_counts:
        on_counts(seeds_h, lens_h, cw.class_counts())
    got = dev_jobs_to_host(dj, n)
    hj = HostJobs(g, flat, offs_h, lens_h, seeds_h, n_threads=4, opt=opt, contigs=contigs)
    assert int(dj.n_jobs) == hj.n_jobs and int(dj.n_regs) == hj.n_regs
    for k in ("qlen", "tlen", "h0", "job_read", "job_reg", "job_side", "qoff", "toff", "regs_per_read", "q", "t"):
        assert np.array_equal(got[k], getattr(hj, k)), k
    assert np.array_equal(got["frac_rep"], hj.frac_rep())
    # extension + merge on the device vs oracle extension + host merge
    out3 = torch.zeros(max(hj.n_jobs, 1), 3, dtype=torch.int32, device="cuda")
    regs = torch.zeros(max(hj.n_regs, 1), 8, dtype=torch.int32, device="cuda")
    if hj.n_jobs:
        rc = load_library().bmh_extend_batch(dj.d_q, dj.d_qoff, dj.d_qlen, dj.d_t, dj.d_toff, dj.d_tlen, dj.d_h0, int(dj.n_jobs),
                                             C.byref(ext_p), out3.data_ptr(), None, None)
        assert rc == 0
    cw.merge(out3, regs)
    torch.cuda.synchronize()
    want3, _, _ = oracle.extend_batch(*hj.jobs(), params=ksw_p) if hj.n_jobs else (np.zeros((0, 3), np.int32), None, None)
    assert np.array_equal(out3.cpu().numpy()[: hj.n_jobs], want3)
    assert np.array_equal(regs.cpu().numpy()[: hj.n_regs], hj.merge(want3))
    # the same without materialised base arrays: bmh_chain_extend reads the bases from the reads / 2-bit reference
    cw.set_materialize(False)
    dj2 = cw.chain_batch(dindex, r, o, l, s)
    assert int(dj2.n_jobs) == hj.n_jobs and not dj2.d_q and not dj2.d_t
    if on_counts:
        on_counts(seeds_h, lens_h, cw.class_counts())
    out3b = torch.full((max(hj.n_jobs, 1), 3), -7, dtype=torch.int32, device="cuda")
    raw6 = torch.zeros(max(hj.n_jobs, 1), 6, dtype=torch.int32, device="cuda")
    regs2 = torch.zeros(max(hj.n_regs, 1), 8, dtype=torch.int32, device="cuda")
    cw.extend(out3b, params=ext_p, raw_t=raw6)
    cw.merge(out3b, regs2)
    torch.cuda.synchronize()
    assert np.array_equal(out3b.cpu().numpy()[: hj.n_jobs], want3)
    assert np.array_equal(regs2.cpu().numpy()[: hj.n_regs], hj.merge(want3))
    # the one-call form (two passes, the heavy reads' chaining hidden behind the first pass's extension): same regions, read order
    regs3 = torch.full((hj.n_regs + 3, 8), -9, dtype=torch.int32, device="cuda")
    dj3 = cw.extend_merge(dindex, r, o, l, s, regs3, params=ext_p)
    torch.cuda.synchronize()
    assert int(dj3.n_jobs) == hj.n_jobs and int(dj3.n_regs) == hj.n_regs
    if on_counts:
        on_counts(seeds_h, lens_h, cw.class_counts())
    assert np.array_equal(regs3.cpu().numpy()[: hj.n_regs], hj.merge(want3)) and (regs3.cpu().numpy()[hj.n_regs:] == -9).all()
    tm = cw.extend_merge_timing()
    assert tm["jobs_a"] + tm["jobs_b"] == hj.n_jobs
    if hj.n_regs > 1:
        with pytest.raises(RuntimeError, match="capacity"):
            cw.extend_merge(dindex, r, o, l, s, regs3[: hj.n_regs - 1])
    stats = (hj.n_jobs, hj.n_regs, int(dj.n_heavy_reads))
    hj.free(); cw.free(); ws.free(); dindex.free()
    return stats
