"""Long reads: the long-query extension kernel (769 .. 16 384 bases) through bmh_extend_batch_long, bit-exact against the CPU
oracle and the reference's own ksw_extend2; bmh_cigar_batch on regions beyond 704 bases against the oracle's mem_reg2aln;
the opt-in Aligner(long_reads=True) on reads of 1 000 and 2 500 bp."""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

INT32_MIN = np.iinfo(np.int32).min


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _pack(qs, ts, h0):
    qlen = np.array([len(x) for x in qs], np.uint32); tlen = np.array([len(x) for x in ts], np.uint32)
    qoff = np.concatenate([[0], np.cumsum(qlen)[:-1]]).astype(np.uint32)
    toff = np.concatenate([[0], np.cumsum(tlen)[:-1]]).astype(np.uint32)
    return (np.concatenate(qs).astype(np.uint8), qoff, qlen, np.concatenate(ts).astype(np.uint8), toff, tlen, np.array(h0, np.uint32))


def _cat(*batches):
    qs, ts, h0 = [], [], []
    for q, qoff, qlen, t, toff, tlen, h in batches:
        for k in range(len(qlen)):
            qs.append(q[qoff[k]:qoff[k] + qlen[k]]); ts.append(t[toff[k]:toff[k] + tlen[k]]); h0.append(int(h[k]))
    return _pack(qs, ts, h0)


def _special_jobs(rng, lens=(800, 1500, 2100, 3000)):
    """identical sequences (no trim, the row spans every strip), unrelated ones (early m == 0), tlen < qlen and tlen >> qlen,
    N bases, and long indels placed on and around the strip boundaries of the long kernel (multiples of 512 / 1024 columns)"""
    qs, ts, h0 = [], [], []
    for ql in lens:
        t = rng.integers(0, 4, size=2 * ql + 50).astype(np.uint8)
        qs.append(t[:ql].copy()); ts.append(t[:ql + 20].copy()); h0.append(int(rng.integers(5, 100)))          # identical
        qs.append(rng.integers(0, 4, size=ql).astype(np.uint8)); ts.append(rng.integers(0, 4, size=ql).astype(np.uint8)); h0.append(3)   # unrelated
        qs.append(t[:ql].copy()); ts.append(t[:ql // 3].copy()); h0.append(40)                                  # tlen < qlen
        qs.append(t[:ql].copy()); ts.append(t.copy()); h0.append(40)                                            # tlen > qlen
        q = t[:ql].copy(); q[rng.random(ql) < 0.03] = 4; tt = t[:ql + 30].copy(); tt[rng.random(len(tt)) < 0.03] = 4
        qs.append(q); ts.append(tt); h0.append(60)                                                             # N bases
        for bp in (512, 1024, 1023, 1536):
            if bp + 80 >= ql:
                continue
            for L in (1, 7, 30, 60):
                qs.append(np.concatenate([t[:bp], t[bp + L:bp + L + ql - bp]])); ts.append(t[:ql + 80].copy()); h0.append(30)            # deletion
                qs.append(np.concatenate([t[:bp], rng.integers(0, 4, size=L).astype(np.uint8), t[bp:ql - L]])); ts.append(t[:ql + 80].copy()); h0.append(30)   # insertion
    return _pack(qs, ts, h0)


def _very_long_jobs(rng):
    qs, ts, h0 = [], [], []
    for ql, tl, mode in ((8000, 8200, 0), (12000, 9000, 1), (16384, 16600, 0), (16384, 16384, 2)):
        t = rng.integers(0, 4, size=tl).astype(np.uint8)
        q = np.resize(t, ql).copy()
        if mode == 0:
            q[rng.random(ql) < 0.01] = rng.integers(0, 4)
        elif mode == 1:
            q = np.concatenate([q[:5000], q[5040:], rng.integers(0, 4, size=40).astype(np.uint8)])
        qs.append(q); ts.append(t); h0.append(int(rng.integers(10, 200)))
    return _pack(qs, ts, h0)


def gpu_extend_long(B, jobs, zdrop=0, end_bonus=5, long_queries=True, raw=True, max_qlen=0, scoring=(1, 4, 6, 1, 6, 1)):
    """scoring: (a, b, o_del, e_del, o_ins, e_ins)"""
    import torch
    q, qoff, qlen, t, toff, tlen, h0 = jobs
    n = len(qlen)
    d = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x)).cuda()
         for x in (q, qoff, qlen, t, toff, tlen, h0)]
    out = torch.zeros(n, 3, dtype=torch.int32, device="cuda")
    r6 = torch.zeros(n, 6, dtype=torch.int32, device="cuda") if raw else None
    prm = B.ExtParams(*scoring, zdrop, end_bonus)
    B.extend_batch(*d, out, params=prm, raw_t=r6, long_queries=long_queries, max_qlen=max_qlen)
    torch.cuda.synchronize()
    n_bad = int(B.load_library().bmh_extend_last_unsupported())
    return out.cpu().numpy(), (r6.cpu().numpy() if raw else None), n_bad


def _oracle_params(zdrop, end_bonus):
    import oracle_py
    return oracle_py.KswParams(1, 4, 6, 1, 6, 1, zdrop, end_bonus, 1)


@pytest.fixture(scope="module")
def long_jobs():
    rng = np.random.default_rng(7)
    mixed = common.make_ext_jobs(300, rng, maxq=3000)
    return _cat(mixed, _special_jobs(rng), _very_long_jobs(rng))


@pytest.mark.parametrize("zdrop", [0, 100])
def test_long_extension_matches_oracle(hip, oracle, long_jobs, zdrop):
    jobs = long_jobs
    qlen = jobs[2]
    assert (qlen > 768).sum() > 150 and (qlen <= 768).sum() > 30 and qlen.max() == 16384
    want3, want6, _ = oracle.extend_batch(*jobs, params=_oracle_params(zdrop, 5), n_threads=16, want_raw=True)
    got3, got6, n_bad = gpu_extend_long(hip, jobs, zdrop=zdrop)
    assert n_bad == 0
    bad = np.flatnonzero((got6 != want6).any(1) | (got3 != want3).any(1))
    assert not bad.size, f"{bad.size} jobs differ, first {bad[:5]} (qlen {qlen[bad[:5]]}): got {got6[bad[:3]]} want {want6[bad[:3]]}"
    # the production form (no raw 6-tuple) gives the same three numbers
    got3b, _, _ = gpu_extend_long(hip, jobs, zdrop=zdrop, raw=False)
    assert np.array_equal(got3b, want3)
    # jobs of at most 768 bases take the kernels of bmh_extend_batch: same outputs as there
    short = qlen <= 768
    g3s, g6s, _ = gpu_extend_long(hip, jobs, zdrop=zdrop, long_queries=False)
    assert np.array_equal(g3s[short], got3[short]) and np.array_equal(g6s[short], got6[short])
    assert (g3s[~short] == INT32_MIN).all()


def test_long_extension_cap(hip, oracle):
    rng = np.random.default_rng(11)
    qs, ts, h0 = [], [], []
    for ql in (16385, 20000, 769, 16384, 300):
        t = rng.integers(0, 4, size=ql + 10).astype(np.uint8)
        qs.append(t[:ql].copy()); ts.append(t); h0.append(50)
    jobs = _pack(qs, ts, h0)
    got3, _, n_bad = gpu_extend_long(hip, jobs)
    assert n_bad == 2 and (got3[:2] == INT32_MIN).all()
    want3, _, _ = oracle.extend_batch(*jobs, n_threads=8)
    assert np.array_equal(got3[2:], want3[2:])
    # a smaller cap of the caller's
    got3, _, n_bad = gpu_extend_long(hip, jobs, max_qlen=1000)
    assert n_bad == 3 and (got3[[0, 1, 3]] == INT32_MIN).all() and np.array_equal(got3[[2, 4]], want3[[2, 4]])


def test_long_extension_matches_reference_ksw(hip, ref):
    """the reference's own ksw_extend2 with a band wider than any alignment (w >= qlen + tlen): the GPU contract has no band"""
    rng = np.random.default_rng(3)
    jobs = _cat(common.make_ext_jobs(60, rng, maxq=2500), _special_jobs(rng, lens=(900, 2000)))
    w = int((jobs[2].astype(np.int64) + jobs[5]).max()) + 1
    for zdrop in (0, 100):
        want3, want6 = ref.extend_batch(*jobs, params=_oracle_params(zdrop, 5), w=w)
        got3, got6, n_bad = gpu_extend_long(hip, jobs, zdrop=zdrop)
        assert n_bad == 0
        assert np.array_equal(got3, want3) and np.array_equal(got6, want6)


def _mutate(rng, x, n_sub, indels):
    """substitutions at n_sub random places, then indels [(pos, +len insertion / -len deletion)] from the right"""
    x = x.copy()
    p = rng.choice(len(x), size=n_sub, replace=False)
    x[p] = (x[p] + rng.integers(1, 4, size=n_sub)) & 3
    for pos, L in sorted(indels, reverse=True):
        x = np.concatenate([x[:pos], rng.integers(0, 4, size=L).astype(np.uint8), x[pos:]]) if L > 0 else np.concatenate([x[:pos], x[pos - L:]])
    return x


def test_long_cigar_matches_oracle(hip, oracle):
    """Regions of 1 000 - 5 000 bp reads (substitutions, 1 - 60 bp indels, a 250 bp deletion whose band is wider than the fast path's,
    local scores the first band cannot reach so that the reference retries with a doubled band), both strands, against the oracle's
    restatement of mem_reg2aln; regions of at most 704 bases give the same buffers alone and beside the long ones."""
    import torch
    from bwamem_hip import synth
    from bwamem_hip.lib import cigar_batch
    from test_gpu_parity import _pack_pac, _to_dev
    g, idx = common.genome_and_index(400_000, seed=9)
    l_pac = len(g)
    pac = _pack_pac(g)
    rng = np.random.default_rng(17)
    reads, regs = [], []
    cases = []
    for k in range(48):
        kind = k % 4
        ln = int(rng.integers(1000, 5001)) if kind < 3 else int(rng.integers(150, 600))
        span = ln + (250 if kind == 1 else 0)
        p = int(rng.integers(1000, l_pac - span - 1000))
        ref = g[p:p + span]
        if kind == 1:                                        # one long deletion (the read lacks 250 reference bases)
            x = np.concatenate([ref[:ln // 2], ref[ln // 2 + 250:]])
            x = _mutate(rng, x, ln // 100, [])
        else:
            ind = [(int(rng.integers(50, ln - 100)), int(rng.choice([1, 2, 5, 13, 30, 60])) * int(rng.choice([-1, 1]))) for _ in range(int(rng.integers(1, 6)))]
            x = _mutate(rng, ref, ln // 100, ind)
        rev = bool(k & 4)
        read = synth.revcomp(x) if rev else x
        rb, re = (2 * l_pac - (p + span), 2 * l_pac - p) if rev else (p, p + span)
        n_sub, n_ind = ln // 100, 6
        truesc = len(x) - 5 * n_sub - 20 * n_ind if kind != 2 else len(x)        # kind 2: a local score nothing reaches (retries)
        reads.append(read); cases.append((len(reads) - 1, truesc, 0, len(read), rb, re))
    flat = np.concatenate(reads); lens = np.array([len(r) for r in reads], np.int64); offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rg = np.zeros((len(cases), 8), np.int32)
    for i, (rd, sc, qb, qe, rb, re) in enumerate(cases):
        rg[i] = [rd, sc, qb, qe, rb & 0xFFFFFFFF, rb >> 32, re & 0xFFFFFFFF, re >> 32]
    dindex = hip.Index.upload(idx, pac=pac, l_pac=l_pac)
    r = _to_dev(torch, synth.codes_to_ascii(flat))
    o = torch.from_numpy(offs).to(torch.int32).cuda(); l = torch.from_numpy(lens).to(torch.int32).cuda()
    regs_t = torch.from_numpy(rg).cuda()
    cigar, aln, md = cigar_batch(dindex, r, o, l, regs_t, len(cases), max_cigar=512, md_cap=1024)
    torch.cuda.synchronize()
    cigar = cigar.cpu().numpy().view(np.uint32); aln = aln.cpu().numpy(); md = md.cpu().numpy()
    n_gap = 0
    for i, (rd, sc, qb, qe, rb, re) in enumerate(cases):
        want = oracle.reg2aln(pac, l_pac, reads[rd], qb, qe, rb, re, sc)
        a = aln[i]
        pos = int(np.uint32(a[0])) | (int(a[1]) << 32)
        assert a[7] == 0, (i, a)
        assert (pos, int(a[2]), int(a[4]), int(a[5])) == (want["pos"], want["is_rev"], want["NM"], want["score"]), (i, a, want)
        assert np.array_equal(cigar[i][: a[3]], want["cigar"]), (i, cigar[i][: a[3]], want["cigar"])
        assert bytes(md[i][: a[6]]).decode() == want["MD"], i
        n_gap += int(((want["cigar"] & 0xf) == 2).any())
    assert n_gap > 20
    # the regions of at most 704 bases alone: the same buffers as in the mixed batch
    short = np.flatnonzero((rg[:, 3] - rg[:, 2]) <= 704)
    assert short.size >= 8
    sel = torch.from_numpy(short.astype(np.int32)).cuda()
    c2, a2, m2 = cigar_batch(dindex, r, o, l, regs_t, len(short), sel_t=sel, max_cigar=512, md_cap=1024)
    torch.cuda.synchronize()
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), cigar[short]) and np.array_equal(a2.cpu().numpy(), aln[short])
    assert np.array_equal(m2.cpu().numpy(), md[short])
    dindex.free()


def test_aligner_long_reads(hip, tmp_path):
    """1 000 bp reads exact only over their first 40 bases (a right flank of ~960 bases) and 2 500 bp reads, both strands:
    Aligner(long_reads=True) maps every one at its simulated position and strand; the default Aligner still refuses them."""
    from bwamem_hip import fmindex, synth
    from bwamem_hip.aligner import Aligner
    g = synth.make_genome(300_000, seed=3)
    prefix = str(tmp_path / "g.fa")
    fmindex.write_index(prefix, fmindex.build_fmd_index(g)); fmindex.write_bns(prefix, g)
    rng = np.random.default_rng(2)
    al = Aligner(prefix, n_threads=2, long_reads=True)
    for ln in (1000, 2500):
        rows, truth = [], []
        for k in range(12):
            p = int(rng.integers(0, len(g) - ln))
            x = g[p:p + ln].copy()
            x[40:ln:23] = (x[40:ln:23] + 1) & 3
            rev = bool(k & 1)
            rows.append(synth.codes_to_ascii(synth.revcomp(x) if rev else x)); truth.append((p, rev))
        names = [f"r{ln}_{i}" for i in range(len(rows))]
        txt = al.align_batch(names, rows)
        recs = {}
        for line in txt.splitlines():
            f = line.split("\t")
            if line.startswith("@") or int(f[1]) & 0x900:
                continue
            recs[f[0]] = (int(f[1]), int(f[3]), f[5])
        for nm, (p, rev) in zip(names, truth):
            flag, pos, cig = recs[nm]
            assert not flag & 4, (nm, recs[nm])
            assert bool(flag & 16) == rev and abs(pos - (p + 1)) <= 3, (nm, recs[nm], p, rev)
    al.close()
    al0 = Aligner(prefix, n_threads=2)
    with pytest.raises(NotImplementedError, match="768"):
        al0.align_batch(names, rows)
    al0.close()


SCORING_OPTS = "-A 2 -B 8 -O 12,14 -E 2,3 -T 60 -w 60"      # given in full: the Aligner does not rescale the penalties by -A


@pytest.mark.parametrize("readlen,n_reads,mode,opts", [(1000, 1500, "se_hard", ""), (2500, 600, "se_hard", ""), (1000, 1500, "pe", ""),
                                                        (1000, 1500, "se_hard", SCORING_OPTS), (1000, 1500, "pe", SCORING_OPTS)],
                         ids=["1000-1500-se_hard", "2500-600-se_hard", "1000-1500-pe", "1000-1500-se_hard-scoring", "1000-1500-pe-scoring"])
def test_reference_gase_aln_long_reads(hip, tmp_path, readlen, n_reads, mode, opts):
    """The reference's own host code (oracle/_ref/dropin/bwa-gasal2, linked on this library) with BMH_GASAL_MAX_SEQ_LEN against
    Aligner(long_reads=True) on the same reads (one length per file: the reference's host code aborts on mixed lengths), at the
    default scoring and at another one with asymmetric gap penalties (both sides get the same options)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "oracle", "_ref", "dropin", "bwa-gasal2")):
        pytest.skip("oracle/_ref/dropin/bwa-gasal2 not built (needs the reference sources at build time)")
    env = dict(os.environ, E2E_LONG="1", E2E_READLEN=str(readlen), E2E_TAG=f"long{readlen}_{mode}" + ("_scoring" if opts else ""))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "e2e_dropin.py"), str(tmp_path), "2000000", str(n_reads), "1", mode] + ([opts] if opts else []),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
    out = r.stdout.decode()
    assert r.returncode == 0 and "SAM IDENTICAL" in out, out[-3000:]
