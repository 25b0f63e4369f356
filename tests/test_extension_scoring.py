"""The extension and CIGAR kernels under every kind of scoring the C ABI accepts, at every length class.

include/bwamem_hip.h promises results bit-identical to ksw_extend2 without a band for any non-negative gap penalties.  The CPU
tests pin the oracle (oracle/ksw_oracle.c, oracle/cigar_oracle.c) to the reference's own ksw_extend2 / ksw_global2 over a grid of
scorings; the GPU tests hold every kernel class (closed form, packed 16-bit, 16-lane rows, wide, streamed long target, long-query)
to that oracle under the same grid, with z-drop and end bonus crossed in, at the router's and the gates' boundaries."""
import numpy as np
import pytest

import common
from test_long_reads import _cat, _pack, _special_jobs, gpu_extend_long

INT32_MIN = np.iinfo(np.int32).min

# (a, b, o_del, e_del, o_ins, e_ins)
SCORINGS = {
    "default": (1, 4, 6, 1, 6, 1),
    "scaled2": (2, 8, 12, 2, 12, 2),
    "ins_dear": (1, 4, 6, 1, 9, 3),          # insertions cost more
    "del_dear": (1, 4, 9, 3, 6, 1),          # deletions cost more
    "lut_edge": (3, 31, 9, 3, 9, 3),         # the edge of the bit-field score table (|a|, |b| < 32)
    "generic": (33, 40, 50, 7, 50, 7),       # compare / select form
    "b0": (1, 0, 6, 1, 6, 1),                # b = 0: never packed
    "free_open": (1, 4, 0, 1, 0, 1),
    "free_ext": (1, 4, 6, 0, 6, 0),
}
END_BONUS = (0, 5, 60)


def _settings():
    """(name, scoring, zdrop, end_bonus, r): a Latin square, so that every scoring meets each of zdrop 0 / 1 / 100 a and each
    end bonus exactly once (r = the row of the square)"""
    out = []
    for k, (name, sc) in enumerate(SCORINGS.items()):
        for r in range(3):
            out.append((name, sc, (0, 1, 100 * sc[0])[r], END_BONUS[(r + k) % 3], r))
    return out


SETTINGS = _settings()


def _very_long_row(name):
    """the setting that gets the queries beyond 8 192 (class 53, extend_long_kernel<16, 16>): zdrop 0 for every other scoring,
    zdrop 100 a for the rest, so that the z-drop branches of that kernel run under non-default scorings too"""
    return 2 if list(SCORINGS).index(name) % 2 else 0
SETTING_IDS = [f"{n}-z{z}-eb{eb}" for n, _, z, eb, _ in SETTINGS]


def _params(sc, zdrop, end_bonus):
    import oracle_py
    return oracle_py.KswParams(*sc, zdrop, end_bonus, 1)


def _scale_h0(jobs, a, rng, h0_min=0):
    """seed scores scale with the match score; a few jobs get h0 = h0_min .. 1 (the reference's ksw_extend2 asserts h0 > 0)"""
    h0 = jobs[6].astype(np.int64) * a
    k = max(4, len(h0) // 40)
    h0[rng.choice(len(h0), size=k, replace=False)] = np.arange(k) % (2 - h0_min) + h0_min
    return jobs[:6] + (h0.astype(np.uint32),)


def _subs(rng, x, k):
    x = x.copy()
    if k and len(x):
        p = rng.choice(len(x), size=min(k, len(x)), replace=False)
        x[p] = (x[p] + rng.integers(1, 4, size=len(p))) & 3
    return x


def _boundary_jobs(rng, lens, tls):
    """for every query length: a mutated copy (3 % substitutions), an identical copy and an unrelated query, against targets of
    every length in tls(ql)"""
    qs, ts, h0 = [], [], []
    for ql in lens:
        for tl in tls(ql):
            t = rng.integers(0, 4, size=tl).astype(np.uint8)
            base = np.resize(t, ql).copy()
            qs.append(_subs(rng, base, max(1, ql // 33))); ts.append(t); h0.append(int(rng.integers(5, 120)))
            qs.append(base); ts.append(t); h0.append(int(rng.integers(5, 120)))
            qs.append(rng.integers(0, 4, size=ql).astype(np.uint8)); ts.append(t); h0.append(int(rng.integers(5, 120)))
    return _pack(qs, ts, h0)


def _strip_jobs(rng, lens):
    """long queries with 1 % substitutions and one indel placed across a strip boundary of the long kernel (multiples of 512
    columns; 1024 in the class beyond 8192), plus a target shorter than the query"""
    qs, ts, h0 = [], [], []
    for ql in lens:
        t = rng.integers(0, 4, size=ql + 100).astype(np.uint8)
        strip = 1024 if ql > 8192 else 512
        bp = max(1, ((ql - 1) // strip) * strip)
        bp = bp if bp + 40 < ql else max(1, bp - strip)
        L = int(rng.choice([1, 7, 30]))
        x = _subs(rng, t[:ql + L], (ql + L) // 100)
        if rng.random() < 0.5:
            q = np.concatenate([x[:bp], x[bp + L:]])[:ql]                                          # deletion at the strip edge
        else:
            q = np.concatenate([x[:bp], rng.integers(0, 4, size=L).astype(np.uint8), x[bp:]])[:ql]  # insertion at the strip edge
        qs.append(q); ts.append(t); h0.append(int(rng.integers(5, 120)))
        qs.append(_subs(rng, t[:ql], ql // 100)); ts.append(t[:max(1, ql // 3)].copy()); h0.append(40)
    return _pack(qs, ts, h0)


SHORT_LENS = (1, 16, 17, 128, 129, 136, 137, 256, 257, 288, 289, 320, 512, 513, 640, 768)
LONG_LENS = (769, 1024, 1025, 1535, 1536, 1537, 2048, 2049, 3584, 3585, 4096, 4097, 7680, 7681, 8192)
VERY_LONG_LENS = (8193, 9216, 9217, 16384)


def _short_jobs(rng, a):
    """bmh_extend_batch's classes: query lengths on both sides of every class boundary up to 768, targets past the LDS staging
    caps (385, 513, 641) and past EXT_T_CAP (1025: the wide kernel streams them), and chain2aln-shaped jobs"""
    b = _boundary_jobs(rng, SHORT_LENS, lambda ql: (max(1, ql // 3), ql + 7, 385, 641, 1025, 2 * ql + 50))
    return _scale_h0(_cat(b, common.make_ext_jobs(300, rng, maxq=768)), a, rng)


def _long_jobs(rng, a, very_long):
    b = _strip_jobs(rng, LONG_LENS + (VERY_LONG_LENS if very_long else ()))
    return _scale_h0(_cat(b, _special_jobs(rng, lens=(800, 1600)), common.make_ext_jobs(30, rng, maxq=3000)), a, rng)


def _diff(got3, got6, want3, want6, jobs):
    bad = np.flatnonzero((got6 != want6).any(1) | (got3 != want3).any(1))
    return f"{bad.size} jobs differ, first {bad[:4]} qlen {jobs[2][bad[:4]]} tlen {jobs[5][bad[:4]]} h0 {jobs[6][bad[:4]]}: " \
           f"got {got6[bad[:2]].tolist()} / {got3[bad[:2]].tolist()} want {want6[bad[:2]].tolist()} / {want3[bad[:2]].tolist()}"


# --------------------------------------------------------------------------------------------------------------- CPU

def _ref_extend_threads(ref, jobs, p, w, n_threads=16):
    """the reference's (single-threaded) ksw_extend2 on n_threads slices of the batch, longest jobs spread over the slices"""
    from concurrent.futures import ThreadPoolExecutor
    q, qoff, qlen, t, toff, tlen, h0 = jobs
    n = len(qlen)
    order = np.argsort(-(qlen.astype(np.int64) * tlen))
    parts = [order[k::n_threads] for k in range(n_threads) if order[k::n_threads].size]
    out3 = np.zeros((n, 3), np.int32); raw6 = np.zeros((n, 6), np.int32)

    def run(ix):
        return ix, ref.extend_batch(q, qoff[ix], qlen[ix], t, toff[ix], tlen[ix], h0[ix], params=p, w=w)
    with ThreadPoolExecutor(len(parts)) as ex:
        for ix, (o3, r6) in ex.map(run, parts):
            out3[ix] = o3; raw6[ix] = r6
    return out3, raw6


@pytest.mark.parametrize("name,sc,zdrop,end_bonus,r", SETTINGS, ids=SETTING_IDS)
def test_oracle_extend_matches_reference_under_scorings(oracle, ref, name, sc, zdrop, end_bonus, r):
    """oracle_extend_batch == the reference's ksw_extend2 with a band wider than any alignment, raw 6-tuple and the three results,
    on short and long queries (up to 3 000 bases; beyond 8 192 in one setting of every scoring, _very_long_row)"""
    rng = np.random.default_rng(1000 + 7 * list(SCORINGS).index(name) + r)
    parts = [_boundary_jobs(rng, (1, 17, 129, 289, 513, 768), lambda ql: (max(1, ql // 3), ql + 7, 2 * ql + 50)),
             common.make_ext_jobs(120, rng, maxq=3000), _special_jobs(rng, lens=(800, 2100)),
             _strip_jobs(rng, (1025, 1537, 2049) + ((8193, 16384) if r == _very_long_row(name) else ()))]
    jobs = _scale_h0(_cat(*parts), sc[0], rng, h0_min=1)
    qlen = jobs[2]
    assert (qlen > 768).sum() >= 60 and (qlen <= 288).sum() >= 30 and ((qlen > 288) & (qlen <= 768)).sum() >= 20
    assert r != _very_long_row(name) or (qlen > 8192).sum() >= 4
    p = _params(sc, zdrop, end_bonus)
    w = int((qlen.astype(np.int64) + jobs[5]).max()) + 1
    want3, want6 = _ref_extend_threads(ref, jobs, p, w)
    got3, got6, _ = oracle.extend_batch(*jobs, params=p, n_threads=16, want_raw=True)
    assert np.array_equal(got6, want6) and np.array_equal(got3, want3), _diff(got3, got6, want3, want6, jobs)


def _global_cases(rng, n, w):
    """(query, target) pairs with substitutions, indels, N bases and |tlen - qlen| <= w - 3 (the bands bwa_gen_cigar2 uses)"""
    out = []
    while len(out) < n:
        ql = int(rng.integers(1, 400))
        t = rng.integers(0, 4, size=ql + int(rng.integers(0, 40))).astype(np.uint8)
        q = _subs(rng, t[:ql], int(rng.integers(0, 6)))
        for _ in range(int(rng.integers(0, 3))):
            if len(q) < 10:
                break
            pos = int(rng.integers(1, len(q) - 1)); k = int(rng.integers(1, 1 + min(12, w)))
            q = np.concatenate([q[:pos], rng.integers(0, 4, size=k).astype(np.uint8), q[pos:]]) if rng.random() < 0.5 else np.concatenate([q[:pos], q[pos + k:]])
        if rng.random() < 0.05 and len(q):
            q[int(rng.integers(0, len(q)))] = 4
        if rng.random() < 0.3:
            t = t[: max(1, len(q) + int(rng.integers(-8, 9)))]
        if len(q) == 0 or abs(len(t) - len(q)) > w - 3:
            continue
        out.append((q, t))
    return out


@pytest.mark.parametrize("name", [n for n, sc in SCORINGS.items() if sc[3] > 0 and sc[5] > 0])
def test_oracle_global2_matches_reference_under_scorings(oracle, ref, name):
    """oracle_ksw_global2 == the reference's ksw_global2 (score and every CIGAR operation) for the scoring grid (without e = 0)
    at bands 5, 20, 100 and 300"""
    sc = SCORINGS[name]
    rng = np.random.default_rng(50 + list(SCORINGS).index(name))
    p = _params(sc, 0, 5)
    n_indel = 0
    for w in (5, 20, 100, 300):
        for q, t in _global_cases(rng, 250, w):
            a = oracle.global2(q, t, w, p); b = ref.global2(q, t, w, p)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]), (name, w, len(q), len(t), a, b)
            n_indel += int(((a[1] & 0xf) == 1).any() or ((a[1] & 0xf) == 2).any())
    assert n_indel >= 200


# --------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


N_CLS = 54
PK_CLASSES = slice(28, 49)          # packed 16-bit kernels
LANE16_CLASSES = slice(1, 19)       # 16-lane rows (extend16)
WIDE_CLASSES = slice(19, 27)        # extend_wide_kernel (19: also the streamed long targets)
CLOSED_CLS, PK17_CLS, LONG_BASE = 27, 41, 49


def class_sizes(B):
    """jobs per kernel class of the last extension batch"""
    s = np.zeros(N_CLS, np.uint32)
    n = B.load_library().bmh_extend_last_class_sizes(s.ctypes.data, N_CLS)
    assert n == N_CLS, n
    return s


def _check_short(hip, oracle, jobs, sc, zdrop, end_bonus, packed):
    """gpu_extend (default launch, EXT_PERSIST 0 / 1 / 3, three-result form) against the oracle; returns the class sizes of the
    default launch"""
    from test_gpu_parity import gpu_extend
    want3, want6, _ = oracle.extend_batch(*jobs, params=_params(sc, zdrop, end_bonus), n_threads=16, want_raw=True)
    got3, got6 = gpu_extend(hip, jobs, zdrop=zdrop, scoring=sc, packed=packed, end_bonus=end_bonus)
    assert np.array_equal(got6, want6) and np.array_equal(got3, want3), _diff(got3, got6, want3, want6, jobs)
    return class_sizes(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("name,sc,zdrop,end_bonus,r", SETTINGS, ids=SETTING_IDS)
def test_short_extension_under_scorings(hip, oracle, name, sc, zdrop, end_bonus, r, packed):
    """bmh_extend_batch (queries up to 768) on every class: closed form, packed, 16-lane rows, wide, streamed long targets"""
    rng = np.random.default_rng(2000 + 7 * list(SCORINGS).index(name) + r)
    jobs = _short_jobs(rng, sc[0])
    qlen, tlen = jobs[2], jobs[5]
    cs = _check_short(hip, oracle, jobs, sc, zdrop, end_bonus, packed)
    assert cs[0] == 0 and cs.sum() == len(qlen)
    assert cs[WIDE_CLASSES].sum() + cs[CLOSED_CLS] >= ((qlen > 288) & (qlen <= 768)).sum() >= 100
    assert cs[WIDE_CLASSES].sum() >= 100
    assert cs[19] >= ((qlen <= 288) & (tlen > 1024)).sum() >= 30                 # the streamed long targets
    pk_ok = packed and sc[0] > 0 and sc[1] >= 1
    assert (cs[PK_CLASSES].sum() >= (20 if sc[0] > 8 else 100)) if pk_ok else (cs[PK_CLASSES].sum() == 0)
    assert cs[LANE16_CLASSES].sum() >= (10 if pk_ok else 100)


@pytest.mark.gpu
@pytest.mark.parametrize("name,sc,zdrop,end_bonus,r", SETTINGS, ids=SETTING_IDS)
def test_long_extension_under_scorings(hip, oracle, name, sc, zdrop, end_bonus, r):
    """bmh_extend_batch_long on queries of 769 .. 16 384 (beyond 8 192 in one setting of every scoring, _very_long_row): both sides of every
    class boundary and of the strip edges, indels across strip edges; raw 6-tuple and the production three-result form"""
    rng = np.random.default_rng(3000 + 7 * list(SCORINGS).index(name) + r)
    vl = r == _very_long_row(name)
    jobs = _long_jobs(rng, sc[0], very_long=vl)
    qlen = jobs[2]
    want3, want6, _ = oracle.extend_batch(*jobs, params=_params(sc, zdrop, end_bonus), n_threads=16, want_raw=True)
    got3, got6, n_bad = gpu_extend_long(hip, jobs, zdrop=zdrop, end_bonus=end_bonus, scoring=sc)
    assert n_bad == 0
    cs = class_sizes(hip)
    assert np.array_equal(got6, want6) and np.array_equal(got3, want3), _diff(got3, got6, want3, want6, jobs)
    for k, (lo, hi) in enumerate(((769, 1024), (1025, 2048), (2049, 4096), (4097, 8192))):
        assert cs[LONG_BASE + k] == ((qlen >= lo) & (qlen <= hi)).sum() >= 4, (k, cs[LONG_BASE:])
    assert cs[LONG_BASE + 4] == (qlen > 8192).sum() >= (8 if vl else 0)
    got3b, _, _ = gpu_extend_long(hip, jobs, zdrop=zdrop, end_bonus=end_bonus, scoring=sc, raw=False)
    assert np.array_equal(got3b, want3), _diff(got3b, want6, want3, want6, jobs)


def _router_jobs(rng, a):
    """queries around the 129..136 class and the packed limit of 288, seed scores with h0 + qlen a at 2047 .. 2049 and 4095 .. 4097,
    0 / 1 / 2 substitutions (the closed form's cases), targets as long as the query, a little longer, shorter"""
    qs, ts, h0 = [], [], []
    for ql in (100, 128, 129, 132, 136, 137, 144, 160, 161, 200, 256, 257, 287, 288):
        for T in (2048, 4096):
            for dh in (-1, 0, 1):
                h = T + dh - ql * a
                if h < 1:
                    continue
                for k in (0, 1, 2):
                    for tl in (ql, ql + 7, ql - 5):
                        t = rng.integers(0, 4, size=tl + 5).astype(np.uint8)
                        qs.append(_subs(rng, t[:ql], k)); ts.append(t[:tl]); h0.append(h)
    return _pack(qs, ts, h0)


@pytest.mark.gpu
@pytest.mark.parametrize("sc", [(2, 8, 12, 2, 12, 2), (3, 31, 9, 3, 9, 3), (3, 5, 11, 2, 13, 1)], ids=["a2", "a3_lut", "a3_asym"])
def test_router_boundaries_at_larger_match_scores(hip, oracle, sc):
    """h0 + qlen a on both sides of 2048 (the 17-pair class) and 4096 (16-bit keys) for a = 2, 3: exact whichever kernel takes
    the job; with z-drop 1 the closed form is off (b > zdrop) and every job goes to a DP kernel"""
    rng = np.random.default_rng(40 + sc[0] + sc[1])
    jobs = _router_jobs(rng, sc[0])
    hq = jobs[6].astype(np.int64) + jobs[2].astype(np.int64) * sc[0]
    assert all(((hq == v).sum() >= 20) for v in (2047, 2048, 2049, 4095, 4096, 4097))
    for zdrop in (0, 1, 100 * sc[0]):
        for packed in (1, 0):
            cs = _check_short(hip, oracle, jobs, sc, zdrop, 5, packed)
            if packed:
                assert cs[PK_CLASSES].sum() >= 50 and cs[PK17_CLS] >= 5, cs
            if zdrop == 1:
                assert cs[CLOSED_CLS] == 0 and cs[LANE16_CLASSES].sum() >= 50, cs
            elif sc[0] + sc[1] < min(sc[2] + sc[3], sc[4] + sc[5]):
                assert cs[CLOSED_CLS] >= 100, cs


# scoring, packed route expected: both sides of each condition of the packed kernels' gate
GATE = [((1, 254, 6, 1, 6, 1), True), ((1, 255, 6, 1, 6, 1), False),              # a + b <= 255
        ((1, 4, 4094, 1, 6, 1), True), ((1, 4, 4095, 1, 6, 1), False),            # o_del + e_del < 4096
        ((1, 4, 6, 1, 4094, 1), True), ((1, 4, 6, 1, 4095, 1), False),            # o_ins + e_ins < 4096
        ((1, 4, 6, 1, 6, 127), True), ((1, 4, 6, 1, 6, 128), False)]              # e_ins * 32 < 4096


@pytest.mark.gpu
@pytest.mark.parametrize("sc,pk", GATE, ids=[f"{'-'.join(map(str, s))}" for s, _ in GATE])
def test_packed_gate_boundaries(hip, oracle, sc, pk):
    rng = np.random.default_rng(60 + sc[1] + sc[2] + sc[4] + sc[5])
    jobs = common.make_ext_jobs(1500, rng, maxq=288)
    for zdrop in (0, 100):
        cs = _check_short(hip, oracle, jobs, sc, zdrop, 5, None)
        assert (cs[PK_CLASSES].sum() >= 500) if pk else (cs[PK_CLASSES].sum() == 0 and cs[LANE16_CLASSES].sum() >= 500), cs
        cs0 = _check_short(hip, oracle, jobs, sc, zdrop, 5, 0)
        assert cs0[PK_CLASSES].sum() == 0


def _closed_form_jobs(rng):
    """jobs the closed form decides when its parameters allow it: 0, 1 and 2 substitutions (near and far apart), tlen >= qlen"""
    qs, ts, h0 = [], [], []
    for _ in range(600):
        ql = int(rng.integers(1, 513)); tl = ql + int(rng.integers(0, 30))
        t = rng.integers(0, 4, size=tl).astype(np.uint8)
        k = int(rng.integers(0, 3))
        q = t[:ql].copy()
        if k == 2 and ql > 3 and rng.random() < 0.5:              # two substitutions close together
            p = int(rng.integers(0, ql - 3)); d = int(rng.integers(1, 4))
            q[[p, p + d]] = (q[[p, p + d]] + rng.integers(1, 4, size=2)) & 3
        else:
            q = _subs(rng, q, k)
        qs.append(q); ts.append(t); h0.append(int(rng.integers(1, 60)))
    return _pack(qs, ts, h0)


# scoring, zdrop, closed form allowed: b = zdrop and b = zdrop + 1; a + b = min(o + e) - 1 and = min(o + e) on either side
CLOSED = [((1, 4, 6, 1, 6, 1), 4, True), ((1, 4, 6, 1, 6, 1), 3, False),
          ((1, 5, 6, 1, 6, 1), 0, True), ((1, 6, 6, 1, 6, 1), 0, False),
          ((1, 4, 6, 1, 5, 1), 0, True), ((1, 5, 6, 1, 5, 1), 0, False),
          ((1, 4, 5, 1, 6, 1), 0, True), ((1, 5, 5, 1, 6, 1), 0, False),
          ((2, 3, 6, 2, 7, 1), 3, True), ((2, 3, 6, 2, 7, 1), 2, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("sc,zdrop,allowed", CLOSED, ids=[f"{'-'.join(map(str, s))}-z{z}" for s, z, _ in CLOSED])
def test_closed_form_gate_boundaries(hip, oracle, sc, zdrop, allowed):
    rng = np.random.default_rng(80 + sc[1] + zdrop)
    jobs = _closed_form_jobs(rng)
    for packed in (1, 0):
        cs = _check_short(hip, oracle, jobs, sc, zdrop, 5, packed)
        assert (cs[CLOSED_CLS] >= 200) if allowed else (cs[CLOSED_CLS] == 0), cs


def _cigar_case(rng, g, l_pac, sc, n_short, n_long):
    """reads with substitutions and 1 - 60 bp indels (regions of 150, 300 and up to 704 bases, and of 1 000 - 5 000), a 250 bp deletion
    wider than the first band, and local scores the first band cannot reach (the band is doubled and retried), both strands"""
    from bwamem_hip import synth
    from test_long_reads import _mutate
    a, b, od, ed, oi, ei = sc
    reads, cases = [], []
    for k in range(n_short + n_long):
        long_ = k >= n_short
        kind = k % 4
        ln = int(rng.integers(1000, 5001)) if long_ else (150, 300, int(rng.integers(301, 705)), int(rng.integers(100, 705)))[kind]
        big_del = long_ and kind == 1
        span = ln + (250 if big_del else 0)
        p = int(rng.integers(1000, l_pac - span - 1000))
        ref_ = g[p:p + span]
        n_sub = max(1, ln // 100)
        if big_del:
            x = _mutate(rng, np.concatenate([ref_[:ln // 2], ref_[ln // 2 + 250:]]), n_sub, [])
            n_ind = 1
        else:
            ind = [(int(rng.integers(20, ln - 20)), int(rng.choice([1, 2, 5, 13, 30, 60] if long_ else [1, 2, 5, 13])) * int(rng.choice([-1, 1])))
                   for _ in range(int(rng.integers(0, 4)))]
            x = _mutate(rng, ref_, n_sub, ind)
            n_ind = len(ind)
        rev = bool(k & 4)
        read = synth.revcomp(x) if rev else x
        rb, re = (2 * l_pac - (p + span), 2 * l_pac - p) if rev else (p, p + span)
        truesc = a * len(x) - (a + b) * n_sub - (max(od, oi) + 10 * max(ed, ei)) * n_ind
        if kind == 2:
            truesc = a * len(x)                            # a local score nothing reaches: the reference retries with a doubled band
        reads.append(read); cases.append((len(reads) - 1, max(truesc, 1), 0, len(read), rb, re))
    return reads, cases


@pytest.mark.gpu
@pytest.mark.parametrize("opt_w", [20, 100, 300])
@pytest.mark.parametrize("name", ["default", "scaled2", "ins_dear", "del_dear", "generic"])
def test_cigar_under_scorings(hip, oracle, name, opt_w):
    """bmh_cigar_batch == the oracle's mem_reg2aln (POS, strand, CIGAR, NM, MD, score) under other scorings and bands"""
    import torch
    from bwamem_hip import synth
    from bwamem_hip.lib import cigar_batch
    from test_gpu_parity import _pack_pac, _to_dev
    sc = SCORINGS[name]
    g, idx = common.genome_and_index(400_000, seed=9)
    l_pac = len(g); pac = _pack_pac(g)
    rng = np.random.default_rng(500 + opt_w + list(SCORINGS).index(name))
    reads, cases = _cigar_case(rng, g, l_pac, sc, 24, 12)
    flat = np.concatenate(reads); lens = np.array([len(r) for r in reads], np.int64); offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rg = np.zeros((len(cases), 8), np.int32)
    for i, (rd, s, qb, qe, rb, re) in enumerate(cases):
        rg[i] = [rd, s, qb, qe, rb & 0xFFFFFFFF, rb >> 32, re & 0xFFFFFFFF, re >> 32]
    dindex = hip.Index.upload(idx, pac=pac, l_pac=l_pac)
    try:
        r = _to_dev(torch, synth.codes_to_ascii(flat))
        o = torch.from_numpy(offs).to(torch.int32).cuda(); l = torch.from_numpy(lens).to(torch.int32).cuda()
        regs_t = torch.from_numpy(rg).cuda()
        prm = hip.ExtParams(*sc, 0, 5)
        cigar, aln, md = cigar_batch(dindex, r, o, l, regs_t, len(cases), params=prm, opt_w=opt_w, max_cigar=512, md_cap=1024)
        torch.cuda.synchronize()
        cigar = cigar.cpu().numpy().view(np.uint32); aln = aln.cpu().numpy(); md = md.cpu().numpy()
        n_gap = n_long = n_wide = 0
        for i, (rd, s, qb, qe, rb, re) in enumerate(cases):
            want = oracle.reg2aln(pac, l_pac, reads[rd], qb, qe, rb, re, s, reg_w=opt_w, opt_w=opt_w, params=_params(sc, 0, 5))
            a = aln[i]
            pos = int(np.uint32(a[0])) | (int(a[1]) << 32)
            assert a[7] == 0, (i, qe - qb, re - rb, a)
            assert (pos, int(a[2]), int(a[4]), int(a[5])) == (want["pos"], want["is_rev"], want["NM"], want["score"]), (i, len(reads[rd]), a, want)
            assert np.array_equal(cigar[i][: a[3]], want["cigar"]), (i, cigar[i][: a[3]], want["cigar"])
            assert bytes(md[i][: a[6]]).decode() == want["MD"], i
            n_gap += int(((want["cigar"] & 0xf) == 1).any() or ((want["cigar"] & 0xf) == 2).any())
            long_ = max(qe - qb, re - rb) > 704
            n_long += int(long_)
            # a length difference that forces a band wider than the retries' cap of 4 opt_w (ksw_global2's w >= |tlen - qlen| + 3)
            n_wide += int(long_ and abs((re - rb) - (qe - qb)) + 3 > 4 * opt_w)
        assert n_gap >= 12 and n_long >= 12
        assert n_wide >= (3 if opt_w == 20 else 0)
        # e = 0 (free extensions): the band inference divides by e, in the reference too -- refused up front
        with pytest.raises(RuntimeError, match="bad argument"):
            cigar_batch(dindex, r, o, l, regs_t, len(cases), params=hip.ExtParams(*SCORINGS["free_ext"], 0, 5), opt_w=opt_w, max_cigar=512, md_cap=1024)
    finally:
        dindex.free()
