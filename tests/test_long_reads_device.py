"""Reads beyond 700 bases on the device job builder and the native pipeline: bmh_chain_batch / bmh_chain_extend /
bmh_chain_extend_merge chain them in wide records (chain_long_kernel) and extend their flanks up to the workspace's cap
(bmh_chain_ws_set_max_qlen), against the host job builder + bmh_extend_batch_long; the cap's refusals; and
Aligner(long_reads=True).align_file streamed through bmh_aligner_run_file against the batch-by-batch Python loop."""
import ctypes as C
import os

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

LENS = (150, 701, 790, 1000, 2500, 8000, 16000)


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _pack_pac(g):
    pad = (-len(g)) % 4
    codes = np.concatenate([g, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    pac = ((codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([pac, np.zeros(1, np.uint8)]))


def _mutate(rng, x, rate=0.01, n_run=False):
    """point substitutions at `rate`, a few 1-3 base indels, optionally a run of N"""
    x = x.copy()
    k = rng.random(len(x)) < rate
    x[k] = (x[k] + rng.integers(1, 4, size=int(k.sum()))) & 3
    for _ in range(len(x) // 800):
        p = int(rng.integers(50, len(x) - 50))
        if rng.random() < 0.5:
            x = np.concatenate([x[:p], rng.integers(0, 4, size=int(rng.integers(1, 4))).astype(np.uint8), x[p:]])
        else:
            x = np.concatenate([x[:p], x[p + int(rng.integers(1, 4)):]])
    if n_run:
        p = int(rng.integers(0, len(x) - 30))
        x[p:p + int(rng.integers(5, 30))] = 4
    return x


def _reads(rng, g, lens, per_len=4, starts=None):
    """reads of every length in `lens`, both strands, some with runs of N; starts: optional positions to draw from"""
    rows = []
    for ln in lens:
        for k in range(per_len):
            if starts is not None:
                p = int(starts[(k + ln) % len(starts)]) - ln // 2
                p = min(max(p, 0), len(g) - ln - 10)
            else:
                p = int(rng.integers(0, len(g) - ln - 10))
            x = _mutate(rng, g[p:p + ln], n_run=(k % 3 == 2))[:ln]
            rows.append(synth_revcomp(x) if k & 1 else x)
    return rows


def synth_revcomp(x):
    from bwamem_hip import synth
    return synth.revcomp(x)


def _genome(kind):
    from bwamem_hip import synth
    if kind == "repeats":
        g = synth.make_genome(400_000, seed=11, repeat_frac=0.4, repeat_len=(300, 3000), repeat_copies=(5, 60), repeat_div=0.03)
        return g, None
    g = synth.make_genome(400_000, seed=12)
    return g, [("chrA", 230_000), ("chrB", 170_000)]


def _chain_setup(B, g, contigs, rows, opt_over=None):
    import torch
    from bwamem_hip import fmindex, synth
    from bwamem_hip.lib import ChainOpt, ChainWorkspace, load_library
    idx = fmindex.build_fmd_index(g)
    dindex = B.Index.upload(idx, pac=_pack_pac(g), l_pac=len(g))
    flat, offs, lens = common.ragged_reads(rows)
    n = len(rows)
    ws = B.SeedWorkspace(n, int(flat.size), max_cands=int(flat.size), max_occ=1 << 22)
    r = torch.from_numpy(np.ascontiguousarray(synth.codes_to_ascii(flat))).cuda()
    o = torch.from_numpy(offs.astype(np.int64)).to(torch.int32).cuda()
    l = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).cuda()
    s = ws.seed_batch(dindex, r, o, l, 19)
    opt = ChainOpt(); load_library().bmh_chain_opt_default(C.byref(opt))
    for k, v in (opt_over or {}).items():
        setattr(opt, k, v)
    cw = ChainWorkspace(n, max(int(s.n_seeds), 1), opt=opt)
    cw.set_materialize(False)
    if contigs:
        cw.set_contigs(contigs)
    return dict(dindex=dindex, ws=ws, r=r, o=o, l=l, s=s, opt=opt, cw=cw, flat=flat, offs=offs, lens=lens, n=n)


@pytest.mark.parametrize("kind", ["repeats", "two_contigs"])
@pytest.mark.parametrize("W", [0, 5])
def test_device_builder_long_reads_equal_host_builder(hip, kind, W):
    """150 .. 16 000 bp reads, both strands, runs of N (two contigs: reads across the boundary too): bmh_chain_batch ->
    bmh_chain_extend (cap EXT_LONG_MAX) -> bmh_chain_merge and bmh_chain_extend_merge against HostJobs + extend_batch(long_queries)
    + its merge.  Jobs equal as a multiset, regions / regs_per_read / frac_rep byte for byte."""
    import torch
    from bwamem_hip.lib import EXT_LONG_MAX, HostJobs, dev_jobs_to_host, extend_batch, seeds_to_host
    B = hip
    rng = np.random.default_rng(100 + W + (kind == "repeats"))
    g, contigs = _genome(kind)
    rows = _reads(rng, g, LENS, per_len=4)
    if contigs:
        rows += _reads(rng, g, (1000, 2500, 8000), per_len=2, starts=[contigs[0][1]])
    t = _chain_setup(B, g, contigs, rows, {"min_chain_weight": W} if W else None)
    cw, n = t["cw"], t["n"]
    cw.set_max_qlen(EXT_LONG_MAX)
    dj = cw.chain_batch(t["dindex"], t["r"], t["o"], t["l"], t["s"])
    got = dev_jobs_to_host(dj, n)
    hj = HostJobs(g, t["flat"], t["offs"], t["lens"], seeds_to_host(t["s"], n), n_threads=4, opt=t["opt"], contigs=contigs)
    assert int(dj.n_jobs) == hj.n_jobs and int(dj.n_regs) == hj.n_regs
    keys = ("qlen", "tlen", "h0", "job_read", "job_reg", "job_side")
    dev_jobs = sorted(zip(*[np.asarray(got[k]).tolist() for k in keys]))
    host_jobs = sorted(zip(*[np.asarray(getattr(hj, k)).tolist() for k in keys]))
    assert dev_jobs == host_jobs
    assert np.array_equal(got["regs_per_read"], hj.regs_per_read)
    assert got["frac_rep"].tobytes() == np.ascontiguousarray(hj.frac_rep(), dtype=np.float32).tobytes()
    assert int(np.max(hj.qlen)) > 768, "the batch must have flanks for the long-query classes"
    # extension + merge: device descriptors against the host builder's jobs on bmh_extend_batch_long
    ext_p = B.ExtParams.default()
    out3 = torch.zeros(max(hj.n_jobs, 1), 3, dtype=torch.int32, device="cuda")
    regs = torch.zeros(max(hj.n_regs, 1), 8, dtype=torch.int32, device="cuda")
    cw.extend(out3, params=ext_p)
    cw.merge(out3, regs)
    torch.cuda.synchronize()
    h3 = torch.zeros(max(hj.n_jobs, 1), 3, dtype=torch.int32, device="cuda")
    d = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x)).cuda() for x in hj.jobs()]
    extend_batch(*d, h3, params=ext_p, long_queries=True)
    want = np.ascontiguousarray(hj.merge(h3[:hj.n_jobs].cpu().numpy()))
    assert regs.cpu().numpy()[:hj.n_regs].tobytes() == want.tobytes()
    # the one-call form (the native pipeline's): same regions in read order
    regs2 = torch.full((hj.n_regs + 16, 8), -7, dtype=torch.int32, device="cuda")
    dj2 = cw.extend_merge(t["dindex"], t["r"], t["o"], t["l"], t["s"], regs2, params=ext_p)
    torch.cuda.synchronize()
    assert int(dj2.n_regs) == hj.n_regs
    assert regs2.cpu().numpy()[:hj.n_regs].tobytes() == want.tobytes()
    hj.free(); cw.free(); t["ws"].free()


def test_extension_cap(hip):
    """Default cap 768: 720-790 bp reads with short flanks align on the device; a 1 000 bp read with a ~960-base flank makes
    bmh_chain_extend and bmh_chain_extend_merge return BMH_EINVAL naming 768, with no region written; a read over 16 384 bases
    is refused with a message that gives the cap."""
    import torch
    from bwamem_hip import synth
    B = hip
    rng = np.random.default_rng(7)
    g = synth.make_genome(300_000, seed=3)
    short = []
    for ln in (720, 750, 790):
        for k in range(4):
            p = int(rng.integers(0, len(g) - ln))
            x = g[p:p + ln].copy(); x[ln // 2] = (x[ln // 2] + 1) & 3            # two seeds of ~ln/2: flanks of ~ln/2
            short.append(synth.revcomp(x) if k & 1 else x)
    t = _chain_setup(B, g, None, short)
    cw = t["cw"]
    dj = cw.chain_batch(t["dindex"], t["r"], t["o"], t["l"], t["s"])
    nr = int(dj.n_regs)
    assert nr >= len(short)
    out3 = torch.zeros(max(int(dj.n_jobs), 1), 3, dtype=torch.int32, device="cuda")
    regs = torch.zeros(max(nr, 1), 8, dtype=torch.int32, device="cuda")
    cw.extend(out3, params=B.ExtParams.default()); cw.merge(out3, regs)
    torch.cuda.synchronize()
    rg = regs.cpu().numpy()[:nr]
    assert (rg[:, 1] > 0).all() and (rg[:, 1] < 1000).all()                   # (no INT32_MIN folded into a score)
    cw.free(); t["ws"].free()

    far = []
    for k in range(4):
        p = int(rng.integers(0, len(g) - 1000))
        x = g[p:p + 1000].copy(); x[40::23] = (x[40::23] + 1) & 3                # exact over 40 bases only: a right flank of ~960
        far.append(x)
    t = _chain_setup(B, g, None, far)
    cw = t["cw"]
    dj = cw.chain_batch(t["dindex"], t["r"], t["o"], t["l"], t["s"])
    out3 = torch.zeros(max(int(dj.n_jobs), 1), 3, dtype=torch.int32, device="cuda")
    regs = torch.full((max(int(dj.n_regs), 1) + 8, 8), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="768"):
        cw.extend(out3, params=B.ExtParams.default())
    cw.merge(out3, regs)
    torch.cuda.synchronize()
    assert (regs.cpu().numpy() == -7).all()
    regs.fill_(-7)
    with pytest.raises(RuntimeError, match="768"):
        cw.extend_merge(t["dindex"], t["r"], t["o"], t["l"], t["s"], regs, params=B.ExtParams.default())
    torch.cuda.synchronize()
    assert (regs.cpu().numpy() == -7).all()
    cw.free(); t["ws"].free()

    p = 1000
    huge = [g[p:p + 17_000].copy(), g[5000:5150].copy()]
    t = _chain_setup(B, g, None, huge)
    t["cw"].set_max_qlen(16384)
    with pytest.raises(RuntimeError, match="16384"):
        t["cw"].chain_batch(t["dindex"], t["r"], t["o"], t["l"], t["s"])
    with pytest.raises(ValueError):
        t["cw"].set_max_qlen(16385)
    t["cw"].free(); t["ws"].free()


def _write_fasta(path, rows, names):
    from bwamem_hip import synth
    with open(path, "w") as f:
        for nm, x in zip(names, rows):
            f.write(f">{nm}\n{synth.codes_to_ascii(np.asarray(x)).tobytes().decode()}\n")


def _pairs(rng, g, ln, n):
    rows = []
    for _ in range(n):
        ins = int(rng.integers(ln + 200, ln + 1200))
        p = int(rng.integers(0, len(g) - ins - 10))
        rows.append(_mutate(rng, g[p:p + ln])[:ln])
        rows.append(synth_revcomp(_mutate(rng, g[p + ins - ln:p + ins])[:ln]))
    return rows


@pytest.mark.parametrize("case", ["1k_se", "2500_se", "mix_se", "1k_pe", "mix_pe"])
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_native_streaming_equals_batch_loop(hip, tmp_path, monkeypatch, case, fmt):
    """Aligner(long_reads=True).align_file through bmh_aligner_run_file (several batches, -C and -R) equals the same aligner with
    BMH_ALIGNER_NATIVE=0 (HostJobs-free batch loop in Python) byte for byte."""
    import io
    from bwamem_hip import fmindex, synth
    from bwamem_hip.aligner import Aligner
    g = synth.make_genome(300_000, seed=5, repeat_frac=0.2, repeat_len=(300, 2000), repeat_copies=(5, 40), repeat_div=0.03)
    prefix = str(tmp_path / "g.fa")
    fmindex.write_index(prefix, fmindex.build_fmd_index(g)); fmindex.write_bns(prefix, g)
    rng = np.random.default_rng(hash(case) & 0xFFFF)
    paired = case.endswith("_pe")
    if case == "1k_se":
        rows = [r[:1000] for r in _reads(rng, g, (1000,), per_len=40)]
    elif case == "2500_se":
        rows = _reads(rng, g, (2500,), per_len=20)
    elif case == "mix_se":
        rows = _reads(rng, g, (150,), per_len=60) + _reads(rng, g, (1000,), per_len=20)
        rows = [rows[i] for i in rng.permutation(len(rows))]
    elif case == "1k_pe":
        rows = _pairs(rng, g, 1000, 20)
    else:
        rows = _pairs(rng, g, 150, 30) + _pairs(rng, g, 1000, 10)
    names = [f"q{i // 2 if paired else i}" for i in range(len(rows))]
    comments = [f"BC:Z:{i % 7}" for i in range(len(rows))]
    path = str(tmp_path / ("reads.fq" if fmt == "fastq" else "reads.fa"))
    if fmt == "fastq":
        with open(path, "w") as f:
            for nm, c, x in zip(names, comments, rows):
                q = (33 + rng.integers(2, 41, size=len(x))).astype(np.uint8).tobytes().decode()
                f.write(f"@{nm} {c}\n{synth.codes_to_ascii(np.asarray(x)).tobytes().decode()}\n+\n{q}\n")
    else:
        _write_fasta(path, rows, [f"{nm} {c}" for nm, c in zip(names, comments)])
    chunk = 24_000 if paired else 20_000

    def run(native):
        monkeypatch.setenv("BMH_ALIGNER_NATIVE", "1" if native else "0")
        al = Aligner(prefix, n_threads=2, long_reads=True)
        al.set_options(["-C", "-R", "@RG\\tID:grp1\\tSM:s1"])
        buf = io.BytesIO()
        al.align_file(path, buf, paired=paired, chunk_bases=chunk)
        st = getattr(al, "last_stats", None)
        al.close()
        return buf.getvalue(), st
    nat, st = run(True)
    assert st is not None and st.n_batches > 1, "the native pipeline must have streamed the file in several batches"
    loop, _ = run(False)
    assert nat.count(b"\n") > len(rows)
    assert nat == loop
