"""The K-mer bitmap of an index handle (csrc/kmer_bits.hip) and the forward search's use of it (smem_forward_kernel).

The rule: a candidate [x, e) of the forward search that is shorter than K is not emitted when read[e-K .. e) holds an N or is no
K-mer of the indexed text T = fwd . revcomp(fwd).  It is exact because such a candidate could only be kept with a begin b,
e - b >= min_seed_len >= K, and then T would hold that window.  Checked three ways: the rule restated in plain Python over the
oracle's rank function against the oracle's SMEMs (CPU); the device bitmap against numpy's K-mer set; the device seeds with the
bitmap on and off against each other and against the oracle.
"""
import functools
import os

import numpy as np
import pytest

import common
import oracle_py
from bwamem_hip import fmindex, synth

from seed_cases import MAX_K, kmer_k, kmer_keys, kmer_table, smems_by_rule, text_of, window_alive      # (the restatement lives beside the seeding case table)


def case_reads(g: np.ndarray, K: int, rng, n_random: int, special=()):
    """reads that reach every branch of the forward search's test (the docstrings of the tests name them)"""
    n = len(g)
    rows = []
    for rate, sd in ((0.01, 1), (0.05, 2)):
        rd, _ = synth.make_reads(g, n_random, 150, seed=sd, sub_rate=rate)
        rows += list(rd)

    def at(p, ln=150):
        return g[p:p + ln].copy()

    def sub(r, *pos):
        for p in pos:
            if 0 <= p < len(r):
                r[p] = (r[p] + 1 + p % 3) & 3
        return r
    pos = iter(rng.integers(1000, n - 1000, size=4000).tolist())
    for o in range(41):                                          # an N at every offset 0..40 (beside a substitution that opens a second pass)
        r = sub(at(next(pos)), 45); r[o] = 4; rows.append(r)
    for o in (20, 25, 31, 40, 47):                               # two Ns fewer than K apart, the second pass begins between or behind them
        r = at(next(pos)); r[o] = 4; r[o + K - 3] = 4; rows.append(r)
        r = sub(at(next(pos)), o - 4); r[o] = 4; r[o + 2] = 4; rows.append(r)
    for ln in (1, K - 1, K, 19, 20, 33, 150, 151):
        rows.append(at(next(pos), ln))
        rows.append(sub(at(next(pos), ln), ln // 2))
        rows.append(sub(at(next(pos), ln), ln - 1))
    r = sub(at(next(pos)), 149); rows.append(r)                  # a pass that starts on the last base (the read's last base is an error)
    r = at(next(pos)); r[148] = 4; rows.append(r)                # ... and behind an N
    r = sub(at(next(pos), 151), 12, 150); rows.append(r)
    for p in special:                                            # tandem repeats / low-divergence copies: many short candidates survive
        for d in range(0, 40, 3):
            rows.append(sub(at(p + d), 30 + d, 90))
            rows.append(synth.revcomp(sub(at(p + 7 * d), 75)))
    t = text_of(g)
    for a in (150, 149, 140, 131, 120, 100, 75, 50, 30, 19, 18, K, K - 1, 5, 1, 0):   # across the forward / reverse boundary of T
        rows.append(t[n - a:n - a + 150].copy())
        rows.append(sub(t[n - a:n - a + 150].copy(), 40, 110))
    for a in (0, 10, 75, 140):                                   # across the middle of the text, where the second contig begins
        rows.append(sub(at(n // 2 - a), 33, 99))
    # substitutions at every offset: the second pass's candidates end on every residue of the packed read words (mod 16 and mod 32), through the
    # rank walk and, with the text on the device, through the unique-interval compare
    for qp in range(4, 92):
        rows.append(sub(at(next(pos)), qp))
        rows.append(sub(at(next(pos)), qp, qp + 9))
        rows.append(sub(at(next(pos)), qp, qp + K + 2, qp + 2 * K + 5))
    return rows


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_sizing_rule():
    assert kmer_k(6_200_000_000) == 18 and kmer_k(2 * 3_100_000_000 * 4) == 18
    assert kmer_k(400_000) == 11 and kmer_k(4_000_000) == 13 and kmer_k(2) == 2 and kmer_k(8) == 3


def test_rule_restated_on_the_cpu_keeps_every_smem():
    """the exactness argument on the CPU: dropping dead candidates before the backward walks changes no SMEM, and saves walks"""
    orc = oracle_py.Oracle()
    g, idx = common.genome_and_index(100_000)
    f = orc.fmd(idx)
    K = kmer_k(idx.seq_len)
    assert K == 11
    rng = np.random.default_rng(5)
    rows = case_reads(g, K, rng, 25)[::3]
    flat, offs, lens = common.ragged_reads(rows)
    tot = {}
    for msl in (K, 19):
        want = orc.seed_reads(f, flat, offs, lens, min_seed_len=msl)
        tab = kmer_table(g, K)
        n_c, n_s = [0, 0], [0, 0]
        for r, q in enumerate(rows):
            m = want["smem_read"] == r
            ref = sorted(zip(want["smem_qb"][m].tolist(), want["smem_qe"][m].tolist(), want["smem_k"][m].tolist(), want["smem_s"][m].tolist()))
            for v, t in enumerate((None, tab)):
                got, nc, ns = smems_by_rule(orc, f, q, msl, t, K)
                assert sorted(got) == ref, (msl, r, v)
                n_c[v] += nc; n_s[v] += ns
        tot[msl] = (n_c, n_s)
        assert n_c[1] < n_c[0] and n_s[1] < n_s[0], (msl, n_c, n_s)
    print("candidates, backward steps (without, with the rule):", tot)


# ---------------------------------------------------------------------------------------------------------------- the device

@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()           # raises if the HIP extension is missing: no fallback
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _index(B, idx, g=None, kbits=True, whole_sa=True):
    from test_gpu_parity import _pack_pac
    old = os.environ.get("BMH_SEED_KBITS")
    os.environ["BMH_SEED_KBITS"] = "1" if kbits else "0"
    try:
        d = B.Index.upload(idx) if g is None else B.Index.upload(idx, pac=_pack_pac(g), l_pac=len(g))
    finally:
        if old is None:
            del os.environ["BMH_SEED_KBITS"]
        else:
            os.environ["BMH_SEED_KBITS"] = old
    if whole_sa:
        d.densify_sa(1)
    return d


def _seed(B, dindex, flat, offs, lens, msl=19, reseed=None):
    import torch
    from bwamem_hip.lib import ReseedOpt, seeds_to_host
    ws = B.SeedWorkspace(len(lens), int(flat.size), max_cands=max(int(flat.size), 64), max_occ=1 << 22)
    r = torch.from_numpy(synth.codes_to_ascii(flat)).cuda()
    o = torch.from_numpy(offs.astype(np.int64)).to(torch.int32).cuda()
    l = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).cuda()
    s = ws.seed_batch(dindex, r, o, l, msl, reseed=ReseedOpt.default(enable=1) if reseed else None)
    out = seeds_to_host(s, len(lens))
    out["n_smems"], out["n_cands"] = int(s.n_smems), int(s.n_cands)
    ws.free()
    return out


@functools.lru_cache(maxsize=1)
def _world():
    """~2 Mbp, 30 % repeats, plus a tandem repeat and a 1 % diverged duplication; its index; the reads; the oracle's seeds by min_seed_len"""
    rng = np.random.default_rng(77)
    g = synth.make_genome(2_000_000, seed=71, repeat_frac=0.3, repeat_len=(300, 3000), repeat_copies=(2, 40), repeat_div=0.03)
    unit = rng.integers(0, 4, size=23).astype(np.uint8)
    g[300_000:300_000 + 23 * 120] = np.tile(unit, 120)
    g[310_000:310_000 + 7 * 300] = np.tile(unit[:7], 300)
    dup = g[500_000:506_000].copy()
    m = rng.random(6000) < 0.01
    dup[m] = (dup[m] + 1) & 3
    g[1_400_000:1_406_000] = dup
    import torch
    idx = fmindex.build_fmd_index(g, device="cuda" if torch.cuda.is_available() else None)
    K = kmer_k(idx.seq_len)
    rows = case_reads(g, K, rng, 550, special=(300_100, 310_050, 500_200, 1_400_900))
    flat, offs, lens = common.ragged_reads(rows)
    orc = oracle_py.Oracle()
    f = orc.fmd(idx)
    want = {msl: orc.seed_reads(f, flat, offs, lens, min_seed_len=msl, n_threads=8) for msl in (K - 1, K, K + 1, 19)}
    return g, idx, K, (flat, offs, lens), want


@pytest.mark.gpu
def test_bitmap_equals_numpy_kmer_set(hip):
    """~200 kbp in two contigs (a contig boundary is a position of the packed text), a hole (filled with random bases, as the packed text
    holds it) and a tandem repeat: the bits read back are exactly the K-mers of fwd . revcomp(fwd), K by the sizing rule"""
    rng = np.random.default_rng(3)
    c1, c2 = rng.integers(0, 4, size=120_011).astype(np.uint8), rng.integers(0, 4, size=80_002).astype(np.uint8)
    c1[40_000:40_700] = rng.integers(0, 4, size=700)             # the hole's fill
    c1[90_000:90_000 + 5 * 400] = np.tile(c1[90_000:90_005], 400)
    c2[-33:] = 0                                                 # poly-A into the forward / reverse boundary
    g = np.concatenate([c1, c2])
    idx = fmindex.build_fmd_index(g, device="cuda")
    K = kmer_k(idx.seq_len)
    assert K == 11
    d = _index(hip, idx, g, whole_sa=False)
    k_dev, ptr, n_words = d.kbits_info()
    assert (k_dev, n_words) == (K, 4 ** K // 32) and ptr
    words = d.kbits_to_host()
    d.free()
    got = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    want = kmer_table(g, K)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"missing {int((want & ~got).sum())}, spurious {int((got & ~want).sum())} of {int(want.sum())}"


@pytest.mark.gpu
def test_seeds_equal_with_bitmap_on_and_off(hip):
    """~1 700 reads: 1 % and 5 % substitutions; an N at every offset 0..40, two Ns fewer than K apart; lengths 1, K-1, K, 19, 20, 33, 150, 151;
    a pass that starts on the last base; tandem-repeat and duplication reads; reads across the forward / reverse boundary and the middle of the
    text; substitutions at every offset 4..91 (candidate ends on every residue mod 16 / 32, rank walk and unique-interval compare: the index
    has the text and the whole suffix array).  on == off == oracle, and the bitmap does remove candidates."""
    g, idx, K, (flat, offs, lens), want = _world()
    on, off = _index(hip, idx, g), _index(hip, idx, g, kbits=False)
    assert on.kbits_info()[0] == K == 13 and off.kbits_info() == (0, 0, 0)
    a, b = _seed(hip, on, flat, offs, lens), _seed(hip, off, flat, offs, lens)
    on.free(); off.free()
    common.assert_seeds_equal(a, b, "on vs off: ")
    common.assert_seeds_equal(a, want[19], "on vs oracle: ")
    assert a["n_smems"] == b["n_smems"]
    print(f"candidates: {b['n_cands']} without, {a['n_cands']} with the bitmap; {len(lens)} reads")
    assert a["n_cands"] < b["n_cands"]


@pytest.mark.gpu
def test_min_seed_len_around_k(hip):
    """min_seed_len = K-1: the test is off (as many candidates as without a bitmap); K and K+1: on; all equal the oracle"""
    g, idx, K, (flat, offs, lens), want = _world()
    on, off = _index(hip, idx, g), _index(hip, idx, g, kbits=False)
    for msl in (K - 1, K, K + 1):
        a, b = _seed(hip, on, flat, offs, lens, msl), _seed(hip, off, flat, offs, lens, msl)
        common.assert_seeds_equal(a, want[msl], f"min_seed_len {msl}, on vs oracle: ")
        common.assert_seeds_equal(b, want[msl], f"min_seed_len {msl}, off vs oracle: ")
        assert (a["n_cands"] == b["n_cands"]) if msl < K else (a["n_cands"] < b["n_cands"]), (msl, a["n_cands"], b["n_cands"])
    on.free(); off.free()


@pytest.mark.gpu
def test_index_without_text_has_no_bitmap(hip):
    g, idx, K, (flat, offs, lens), want = _world()
    d = _index(hip, idx, None, whole_sa=False)
    assert d.kbits_info() == (0, 0, 0) and d.kbits_to_host().size == 0
    common.assert_seeds_equal(_seed(hip, d, flat, offs, lens), want[19], "no text: ")
    d.free()


@pytest.mark.gpu
def test_reseeding_equal_with_bitmap_on_and_off(hip):
    """bmh_seed_batch_reseed (-g) reads kept results only: identical with and without the bitmap, and it does add seeds here"""
    g, idx, K, (flat, offs, lens), want = _world()
    on, off = _index(hip, idx, g), _index(hip, idx, g, kbits=False)
    a, b = _seed(hip, on, flat, offs, lens, reseed=True), _seed(hip, off, flat, offs, lens, reseed=True)
    on.free(); off.free()
    common.assert_seeds_equal(a, b, "re-seeding, on vs off: ")
    assert a["n_smems"] == b["n_smems"] > int((want[19]["score"] > 0).sum())
