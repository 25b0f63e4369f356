"""Re-seeding (gase_aln -g): BWA-MEM's second and third seeding rounds (mem_collect_intv with re_seed, src/bwamem.c:231-300).

The oracle restates mem_collect_intv in Python over the reference's own bwt_smem1 / bwt_seed_strategy1 / bwt_sa (oracle/_ref/libref.so);
the device's bmh_seed_batch_reseed must equal it field by field, the chain stage on its seeds must equal the host job builder, the
aligner's paths must write the same SAM with -g, and a read from one copy of a recent duplication must see the other copy."""
import ctypes as C
import io

import numpy as np
import pytest

import common


# ---------------------------------------------------------------------------------------------------------------- the oracle

class _Intv(C.Structure):
    _fields_ = [("x", C.c_uint64 * 3), ("info", C.c_uint64), ("n_miss_match", C.c_int)]


class _IntvV(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(_Intv))]


def _bind(ref):
    L = ref.lib
    L.bwt_smem1.restype = C.c_int
    L.bwt_smem1.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(_IntvV), C.c_void_p]
    L.bwt_seed_strategy1.restype = C.c_int
    L.bwt_seed_strategy1.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.POINTER(_Intv)]
    return L


def collect_intv(ref, bwt, q, k, reseed=None):
    """mem_collect_intv (seed_type 1) for one read of nt4 codes: [(begin, end, x0, x2, round)] in the order of ks_introsort(mem_intv)"""
    L = _bind(ref)
    q = np.ascontiguousarray(q, dtype=np.uint8)
    qp = q.ctypes.data_as(C.POINTER(C.c_uint8))
    n = len(q)
    v = _IntvV(0, 0, None)

    def smem1(x, min_intv):
        x = L.bwt_smem1(bwt, n, qp, x, min_intv, C.byref(v), None)
        return x, [(int(v.a[i].info >> 32), int(v.a[i].info & 0xFFFFFFFF), int(v.a[i].x[0]), int(v.a[i].x[2])) for i in range(v.n)]
    mem, x = [], 0
    while x < n:
        if q[x] < 4:
            x, got = smem1(x, 1)
            mem += [g + (1,) for g in got if g[1] - g[0] >= k]
        else:
            x += 1
    if reseed is not None and reseed.get("enable", 1):
        sf, sw, mi = reseed.get("split_factor", 1.5), reseed.get("split_width", 10), reseed.get("max_mem_intv", 20)
        split_len = int(float(np.float32(k) * np.float32(sf)) + .499)        # int * float + .499, as C evaluates it
        for b, e, _, s, _ in list(mem):
            if e - b < split_len or s > sw:
                continue
            _, got = smem1((b + e) >> 1, s + 1)
            mem += [g + (2,) for g in got if g[1] - g[0] >= k]
        if mi > 0:
            x, m = 0, _Intv()
            while x < n:
                if q[x] < 4:
                    x = L.bwt_seed_strategy1(bwt, n, qp, x, k, mi, C.byref(m))
                    if m.x[2] > 0:
                        mem.append((int(m.info >> 32), int(m.info & 0xFFFFFFFF), int(m.x[0]), int(m.x[2]), 3))
                else:
                    x += 1
    mem.sort(key=lambda t: (t[0], t[1]))
    return mem


def ref_seeds(ref, bwt, flat, offs, lens, k=19, reseed=None):
    """the mem_seed_v_gpu columns of collect_intv's groups (occurrences by bwt_sa in SA-row order), plus groups per round"""
    groups, per_read, rounds = [], np.zeros(len(lens), np.uint32), np.zeros(4, np.int64)
    for r in range(len(lens)):
        g = collect_intv(ref, bwt, flat[int(offs[r]):int(offs[r]) + int(lens[r])], k, reseed)
        for t in g:
            rounds[t[4]] += 1
        per_read[r] = sum(t[3] for t in g)
        groups += g
    ns = int(per_read.sum())
    rbeg = np.zeros(ns, np.uint64); qbeg = np.zeros((ns, 2), np.int32); score = np.zeros(ns, np.uint32)
    o = 0
    for b, e, x0, s, _ in groups:
        ref.lib.ref_locate(bwt, x0, s, rbeg[o:].ctypes.data_as(C.POINTER(C.c_uint64)))
        qbeg[o:o + s] = (b, e); score[o] = s
        o += s
    prefix = np.zeros(len(lens), np.uint32)
    prefix[1:] = np.cumsum(per_read)[:-1]
    return dict(rbeg=rbeg, qbeg=qbeg, score=score, n_ref_pos=per_read, prefix=prefix, n_smems=len(groups), rounds=rounds[1:])


def test_oracle_without_reseeding_is_ref_collect_smems(ref):
    """self-check of the restatement: re-seeding off, it is the harness's first round (ref_collect_smems)"""
    from bwamem_hip import synth
    g, idx = common.genome_and_index(200_000, seed=5)
    b = ref.bwt_from_index(idx)
    reads, _ = synth.make_reads(g, 300, 150, seed=6, sub_rate=0.02)
    flat, offs, lens = common.ragged_reads(list(reads) + common.edge_reads(g, np.random.default_rng(7)))
    common.assert_seeds_equal(ref_seeds(ref, b, flat, offs, lens), ref.seed_reads(b, flat, offs, lens, 19), "oracle: ")
    with_rs = ref_seeds(ref, b, flat, offs, lens, reseed=dict())
    assert with_rs["n_smems"] > ref_seeds(ref, b, flat, offs, lens)["n_smems"]


# ---------------------------------------------------------------------------------------------------------------- the device

@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()           # raises if the HIP extension is missing: no fallback
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _dup_genome(n=400_000, seed=11, copies=((30_000, 230_000, 0.02),), plen=4000):
    """random genome with planted copies: (src, dst, divergence) copies plen bases from src to dst with substitutions"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=n).astype(np.uint8)
    for src, dst, div in copies:
        seg = g[src:src + plen].copy()
        m = rng.random(plen) < div
        seg[m] = (seg[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
        g[dst:dst + plen] = seg
    return g


def _seed_dev(B, idx, flat, offs, lens, k=19, reseed=None, densify=None, genome=None):
    import torch
    from bwamem_hip import synth
    from bwamem_hip.lib import ReseedOpt, seeds_to_host
    from test_gpu_parity import _pack_pac, _to_dev
    dindex = B.Index.upload(idx) if genome is None else B.Index.upload(idx, pac=_pack_pac(genome), l_pac=len(genome))
    if densify:
        dindex.densify_sa(densify)
    ws = B.SeedWorkspace(max(len(lens), 1), max(int(flat.size), 1), max_cands=max(int(flat.size), 64), max_occ=1 << 20)
    r = _to_dev(torch, synth.codes_to_ascii(flat))
    o = torch.from_numpy(offs.astype(np.int64)).to(torch.int32).cuda()
    l = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).cuda()
    ro = None if reseed is None else ReseedOpt.default(**{"enable": 1, **reseed})
    s = ws.seed_batch(dindex, r, o, l, k, reseed=ro)
    out = seeds_to_host(s, len(lens))
    out["n_smems"] = int(s.n_smems)
    ws.free(); dindex.free()
    return out


def _check(B, ref, idx, flat, offs, lens, k=19, reseed=None, what="", **kw):
    b = ref.bwt_from_index(idx)
    want = ref_seeds(ref, b, flat, offs, lens, k, reseed=reseed if reseed is not None else None)
    got = _seed_dev(B, idx, flat, offs, lens, k, reseed=reseed, **kw)
    common.assert_seeds_equal(got, want, what)
    assert got["n_smems"] == want["n_smems"], (what, got["n_smems"], want["n_smems"])
    return want


@pytest.mark.gpu
def test_reseed_seeds_equal_reference_on_repeats(hip, ref):
    """20 000 x 150 bp and 20 000 x 300 bp reads of a genome with low-divergence repeats; rounds 2 and 3 both add groups"""
    from bwamem_hip import fmindex, synth
    g = synth.make_genome(1_000_000, seed=21, repeat_frac=0.4, repeat_len=(300, 3000), repeat_copies=(2, 30), repeat_div=0.02)
    idx = fmindex.build_fmd_index(g)
    for L, seed in ((150, 1), (300, 2)):
        reads, _ = synth.make_reads(g, 20_000, L, seed=seed, sub_rate=0.01)
        flat, offs, lens = common.flat_reads(reads)
        want = _check(hip, ref, idx, flat, offs, lens, reseed=dict(), what=f"{L} bp: ", genome=g)
        assert want["rounds"][1] > 100 and want["rounds"][2] > 1000, want["rounds"]


@pytest.mark.gpu
def test_reseed_edge_reads_and_thresholds(hip, ref):
    """edge reads (N, shorter than k, ...), SMEMs of exactly split_len bases, SMEMs of split_width and split_width + 1 occurrences"""
    from bwamem_hip import fmindex
    rng = np.random.default_rng(3)
    g = rng.integers(0, 4, size=300_000).astype(np.uint8)
    seg10, seg11 = g[1000:1100].copy(), g[2000:2100].copy()
    for c in range(1, 10):
        g[10_000 + c * 5000:10_000 + c * 5000 + 100] = seg10          # 10 copies in all
    for c in range(1, 11):
        g[100_000 + c * 5000:100_000 + c * 5000 + 100] = seg11        # 11 copies in all
    idx = fmindex.build_fmd_index(g)
    rows = common.edge_reads(g, rng)
    rows += [seg10[10:90].copy(), seg11[10:90].copy(), seg10.copy(), seg11.copy()]
    for ln in (26, 27, 28, 29, 30):                                    # a genome stretch of about split_len bases between unrelated flanks
        for _ in range(40):
            p = int(rng.integers(200_000, 290_000))
            rows.append(np.concatenate([rng.integers(0, 4, size=40), g[p:p + ln], rng.integers(0, 4, size=40)]).astype(np.uint8))
    for _ in range(50):                                                # N bases in the middle of repeats
        r = seg10.copy(); r[rng.integers(0, 100, size=3)] = 4; rows.append(r)
    flat, offs, lens = common.ragged_reads(rows)
    b = ref.bwt_from_index(idx)
    lens_ok = [t[1] - t[0] for r in range(len(rows)) for t in collect_intv(ref, b, rows[r], 19) if t[4] == 1]
    assert 28 in lens_ok
    occ = [t[3] for r in range(len(rows)) for t in collect_intv(ref, b, rows[r], 19)]
    assert 10 in occ and 11 in occ
    _check(hip, ref, idx, flat, offs, lens, reseed=dict(), what="edge: ")
    _check(hip, ref, idx, flat, offs, lens, reseed=dict(split_width=11), what="edge, split_width 11: ")


@pytest.mark.gpu
@pytest.mark.parametrize("k,densify,opt", [
    (15, None, dict()), (23, None, dict()), (19, 1, dict()), (19, None, dict(split_factor=1.0, split_width=3, max_mem_intv=0)),
    (19, 1, dict(split_factor=2.2, split_width=30, max_mem_intv=5)), (15, 1, dict(max_mem_intv=0)), (23, None, dict(split_factor=1.25, max_mem_intv=50))])
def test_reseed_options(hip, ref, k, densify, opt):
    """-k 15 / 23, sa_intv 16 and 1, non-default split_factor / split_width / max_mem_intv (0: no third round)"""
    from bwamem_hip import fmindex, synth
    g = synth.make_genome(600_000, seed=31, repeat_frac=0.4, repeat_len=(300, 2000), repeat_copies=(2, 60), repeat_div=0.03)
    idx = fmindex.build_fmd_index(g)
    reads, _ = synth.make_reads(g, 3000, 150, seed=32, sub_rate=0.02)
    flat, offs, lens = common.ragged_reads(list(reads) + common.edge_reads(g, np.random.default_rng(33)))
    want = _check(hip, ref, idx, flat, offs, lens, k=k, reseed=opt, densify=densify, genome=g if densify else None, what=f"k {k} {opt}: ")
    if opt.get("max_mem_intv", 20) == 0:
        assert want["rounds"][2] == 0


@pytest.mark.gpu
def test_reseed_long_reads(hip, ref):
    """reads of 2-16 kb out of repeats (long forward lists, many round-3 seeds), beside short ones"""
    from bwamem_hip import fmindex, synth
    g = synth.make_genome(600_000, seed=41, repeat_frac=0.5, repeat_len=(2000, 8000), repeat_copies=(2, 8), repeat_div=0.01)
    idx = fmindex.build_fmd_index(g)
    rng = np.random.default_rng(42)
    rows = []
    for ln in (2000, 4096, 8000, 12_000, 16_384):
        for _ in range(3):
            p = int(rng.integers(0, len(g) - ln)); r = g[p:p + ln].copy()
            m = rng.random(ln) < 0.01; r[m] = (r[m] + 1) & 3
            rows.append(synth.revcomp(r) if rng.random() < 0.5 else r)
    rows.append(np.zeros(3000, np.uint8))                                # poly-A: one long low-complexity run
    rows += list(synth.make_reads(g, 200, 150, seed=43)[0])
    flat, offs, lens = common.ragged_reads(rows)
    _check(hip, ref, idx, flat, offs, lens, reseed=dict(), what="long: ", genome=g)


@pytest.mark.gpu
def test_reseed_off_is_bmh_seed_batch(hip):
    """enable = 0: the output of bmh_seed_batch, byte for byte"""
    from bwamem_hip import synth
    g, idx = common.genome_and_index(400_000, seed=31)
    reads, _ = synth.make_reads(g, 5000, 150, seed=32, sub_rate=0.02)
    flat, offs, lens = common.ragged_reads(list(reads) + common.edge_reads(g, np.random.default_rng(33)))
    a = _seed_dev(hip, idx, flat, offs, lens, reseed=None)
    b = _seed_dev(hip, idx, flat, offs, lens, reseed=dict(enable=0))
    common.assert_seeds_equal(a, b, "enable 0: ")
    assert a["n_smems"] == b["n_smems"]


@pytest.mark.gpu
def test_reseed_device_job_builder_matches_host_builder(hip):
    """bmh_chain_batch on re-seeded seeds (nested groups, duplicates) equals bmh_build_jobs on the same seeds"""
    import torch
    from bwamem_hip import fmindex, synth
    from bwamem_hip.lib import ChainWorkspace, HostJobs, ReseedOpt, dev_jobs_to_host, seeds_to_host
    from test_gpu_parity import _pack_pac, _to_dev
    cases = []
    gr = synth.make_genome(600_000, seed=9, repeat_frac=0.6, repeat_len=(200, 800), repeat_copies=(2, 400), repeat_div=0.02)
    cases.append((gr, synth.make_reads(gr, 3000, 150, seed=8, sub_rate=0.01)[0]))
    cases.append((gr, synth.make_reads(gr, 800, 300, seed=7, sub_rate=0.02)[0]))
    g2 = _dup_genome()
    cases.append((g2, synth.make_reads(g2, 2000, 150, seed=5, sub_rate=0.005)[0]))
    for g, reads in cases:
        idx = fmindex.build_fmd_index(g)
        n, L = reads.shape
        flat = np.ascontiguousarray(reads.reshape(-1)); offs = np.arange(n, dtype=np.uint64) * L; lens = np.full(n, L, np.uint32)
        dindex = hip.Index.upload(idx, pac=_pack_pac(g), l_pac=len(g))
        ws = hip.SeedWorkspace(n, flat.size, max_cands=flat.size, max_occ=1 << 22)
        r = _to_dev(torch, synth.codes_to_ascii(flat))
        o = torch.from_numpy(offs.astype(np.int64)).to(torch.int32).cuda(); l = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).cuda()
        s = ws.seed_batch(dindex, r, o, l, 19, reseed=ReseedOpt.default(enable=1))
        cw = ChainWorkspace(n, max(int(s.n_seeds), 1))
        dj = cw.chain_batch(dindex, r, o, l, s)
        got = dev_jobs_to_host(dj, n)
        hj = HostJobs(g, flat, offs, lens, seeds_to_host(s, n), n_threads=4, opt=cw.opt)
        assert int(dj.n_jobs) == hj.n_jobs and int(dj.n_regs) == hj.n_regs
        for k in ("qlen", "tlen", "h0", "job_read", "job_reg", "job_side", "qoff", "toff", "regs_per_read", "q", "t"):
            assert np.array_equal(got[k], getattr(hj, k)), k
        assert np.array_equal(got["frac_rep"], hj.frac_rep())
        cw.free(); ws.free(); dindex.free()


def _index_files(tmp_path, g):
    from bwamem_hip import fmindex
    prefix = str(tmp_path / "g.fa")
    fmindex.write_index(prefix, fmindex.build_fmd_index(g)); fmindex.write_bns(prefix, g)
    return prefix


def test_g_option_is_accepted_and_takes_no_value():
    """-g turns re-seeding on (no value, as in the reference's getopt string); -r -s -y stay refused on the option list"""
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import ReseedOpt
    al = Aligner.__new__(Aligner)                              # the option parser alone: no index, no device
    from bwamem_hip.lib import ChainOpt, ExtParams, PeOpt, PostOpt, load_library
    Lb = load_library()
    al.copt = ChainOpt(); Lb.bmh_chain_opt_default(C.byref(al.copt)); al.ep = ExtParams.default()
    al.po = PostOpt(); Lb.bmh_post_opt_default(C.byref(al.po)); al.pe = PeOpt(); Lb.bmh_pe_opt_default(C.byref(al.pe))
    al.reseed = ReseedOpt.default()
    assert (al.reseed.enable, round(al.reseed.split_factor, 3), al.reseed.split_width, al.reseed.max_mem_intv) == (0, 1.5, 10, 20)
    al.set_options(["-g", "-k", "23"])
    assert al.reseed.enable == 1 and al.copt.min_seed_len == 23
    al.set_options([], split_factor=2.0, split_width=4, max_mem_intv=0)
    assert (al.reseed.split_factor, al.reseed.split_width, al.reseed.max_mem_intv) == (2.0, 4, 0)
    for f in ("-r", "-s", "-y"):
        with pytest.raises(ValueError):
            al.set_options([f, "1"])


@pytest.mark.gpu
def test_reseed_finds_the_second_copy_of_a_duplication(hip, tmp_path):
    """reads from copy A of a 2-copy duplication at ~2 % divergence: MAPQ 60 without a second hit; with -g most see copy B (XS:i, lower MAPQ)"""
    from bwamem_hip import synth
    from bwamem_hip.aligner import Aligner
    g = _dup_genome(n=400_000, copies=((30_000, 230_000, 0.02),), plen=6000)
    prefix = _index_files(tmp_path, g)
    rng = np.random.default_rng(4)
    pos = rng.integers(30_000, 30_000 + 6000 - 150, size=300)
    reads = [g[p:p + 150].copy() for p in pos]
    names = ["r%d" % i for i in range(len(reads))]
    seqs = [synth.codes_to_ascii(r).tobytes().decode() for r in reads]
    al = Aligner(prefix, n_threads=4)

    def recs(text):
        out = []
        for line in text.split("\n"):
            if not line or line[0] == "@":
                continue
            f = line.split("\t")
            if int(f[1]) & 0x900:
                continue
            xs = [int(t[5:]) for t in f[11:] if t.startswith("XS:i:")]
            out.append((int(f[4]), xs[0] if xs else 0))
        return out
    base = recs(al.align_batch(names, seqs))
    assert len(base) == 300 and sum(1 for q, xs in base if q == 60 and xs == 0) >= 270, base[:10]
    al.set_options(["-g"])
    rs = recs(al.align_batch(names, seqs))
    gained = sum(1 for (q0, _), (q, xs) in zip(base, rs) if xs > 0 and q < q0)
    assert gained >= 150, (gained, rs[:10])
    al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_reseed_sam_same_on_every_path(hip, tmp_path, paired, monkeypatch):
    """with -g: align_batch (the batch-by-batch loop), the native align_file and its host formatter write the same SAM, FASTA and FASTQ"""
    from bwamem_hip import synth
    from bwamem_hip.aligner import Aligner
    from test_fastq import _hard_reads, _write_pair_files
    g = synth.make_genome(800_000, seed=42, repeat_frac=0.4, repeat_len=(300, 3000), repeat_copies=(2, 30), repeat_div=0.02)
    prefix = _index_files(tmp_path, g)
    reads = _hard_reads(g, 4000, 150, paired, seed=12)
    fq, fa, _, _ = _write_pair_files(tmp_path, list(reads), paired, "r")
    al = Aligner(prefix, n_threads=4)
    al.set_options(["-g"])
    texts = {}
    for path in (fa, fq):
        for env in ("", "BMH_ALIGNER_HOST_FORMAT", "BMH_ALIGNER_NATIVE"):
            if env:
                monkeypatch.setenv(env, "0" if env == "BMH_ALIGNER_NATIVE" else "1")
            buf = io.BytesIO()
            al.align_file(path, buf, batch_reads=1500, paired=paired)
            texts[(path, env)] = buf.getvalue()
            if env:
                monkeypatch.delenv(env)
        for env in ("BMH_ALIGNER_HOST_FORMAT", "BMH_ALIGNER_NATIVE"):
            assert texts[(path, env)] == texts[(path, "")], (path, env)
    plain = Aligner(prefix, n_threads=4)
    buf = io.BytesIO(); plain.align_file(fa, buf, batch_reads=1500, paired=paired)
    assert buf.getvalue() != texts[(fa, "")]                            # -g changes records on this genome
    plain.close(); al.close()
