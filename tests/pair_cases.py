"""Hand-made region sets for the pairing stage (csrc/pair_dev.hip against the host walk of csrc/pair_post.cpp) and a plain restatement of
mem_pair / the pair's MAPQ in Python ints and floats, written from csrc/pair_post.cpp (pair_regs, sam_pe).  No GPU is needed here.

A region is the 8-int record {read, score, qb, qe, rb, re} the region tail takes.  What keeps the tail from merging or dropping anything:
regions are full length (qb = 0, qe = L) except where a read is split on purpose; hits of one read lie at least 120 bp apart on the
reference; the two halves of a split read go on opposite strands or different sequences.  A forward hit at P is rb = P, re = P + len; a
reverse hit covering forward [Q, Q + len) is rb = 2 l_pac - (Q + len), re = 2 l_pac - Q.

Every configuration is a calibration population (single-hit forward/reverse pairs, insert ~ N(300, 30), which leaves orientation 1 alive;
`two_orient` adds reverse/forward pairs, orientation 2) mixed with case classes, each built to force one branch of the pairing:
  a  two to six candidate pairs with close scores (n_sub 1, 2, >= 3; runners-up at and beyond the score window)
  b  exactly two candidates, the better one first or last by position          c  two candidates of equal score and insert (the hash decides)
  d  the best pair uses a hit that is not its read's first                     e  the pairable hits are worse than the best ones by more than pen_unpaired
  f  a read split into two primary hits (is_multi)                             g  no candidate pair: other sequence, too far, a dead orientation, no hit, below T
  h  in range in concatenated coordinates but across a sequence boundary, and the same pair moved inside one sequence
  i  the pair on the reverse strand (read 1 reverse, read 2 forward); hits in the first and the last 200 bp
  j  63, 64, 65 hits together (the device's limit and its neighbours)          k  frac_rep in {0, 0.3, 0.9} (drawn for every read)
  l  a single candidate at insert low - 1, low, high, high + 1
The classes a pair was built for are its `intent`; what it really did is judged from the restatement (labels_of)."""
from __future__ import annotations

import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np

L = 100
CONTIG_LENS = (70_000, 50_003, 29_997)
L_PAC = sum(CONTIG_LENS)
CTG_OFF = (0, 70_000, 120_003)
ID0 = 123456                                    # even: a pair's reads are 2 p and 2 p + 1 of the run
M64 = (1 << 64) - 1

CONFIGS = {
    "default": {},
    "two_orient": dict(two=True),
    "no_pairing": dict(pe=dict(no_pairing=1)),
    "pen9": dict(pe=dict(pen_unpaired=9)),
    "scoring": dict(scoring=dict(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2)),
    "flag_all": dict(po=dict(flag_all=1, T=20)),
    "one_contig": dict(one=True),
    "alt": dict(alt=True),
}


def pack_pac(g):
    pad = (-len(g)) % 4
    codes = np.concatenate([g, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    pac = ((codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([pac, np.zeros(1, np.uint8)]))


@functools.lru_cache(maxsize=1)
def genome():
    return np.random.default_rng(2024).integers(0, 4, size=L_PAC).astype(np.uint8)


def fwd(P, score, qb=0, qe=L):
    return (int(score), qb, qe, int(P), int(P) + (qe - qb))


def rev(Q, score, qb=0, qe=L):
    n = qe - qb
    return (int(score), qb, qe, 2 * L_PAC - (int(Q) + n), 2 * L_PAC - int(Q))


def options(name):
    """The option structs of a configuration (and the arrays they point to, kept alive in the result)."""
    import bwamem_hip as B
    from bwamem_hip.lib import ChainOpt, PeOpt, PostOpt
    lib = B.load_library()
    spec = CONFIGS[name]
    co = ChainOpt(); lib.bmh_chain_opt_default(C.byref(co))
    po = PostOpt(); lib.bmh_post_opt_default(C.byref(po)); po.id0 = ID0
    pe = PeOpt(); lib.bmh_pe_opt_default(C.byref(pe)); pe.no_rescue = 1
    ep = B.ExtParams.default()
    for k, v in spec.get("scoring", {}).items():
        setattr(ep, k, v); setattr(co, k, v)
    for k, v in spec.get("po", {}).items():
        setattr(po, k, v)
    for k, v in spec.get("pe", {}).items():
        setattr(pe, k, v)
    contigs = None if spec.get("one") else [("c%d" % i, n) for i, n in enumerate(CONTIG_LENS)]
    alt = None
    if spec.get("alt"):
        alt = np.array([0, 0, 1], np.uint8)
        co.contig_is_alt = alt.ctypes.data; po.contig_is_alt = alt.ctypes.data
    return SimpleNamespace(co=co, ep=ep, po=po, pe=pe, contigs=contigs, alt=alt)


def plain_opt(o):
    """The numbers the restatement needs, as Python values."""
    tmp = max(o.ep.a + o.ep.b, o.ep.o_del + o.ep.e_del, o.ep.o_ins + o.ep.e_ins)
    return SimpleNamespace(a=o.ep.a, tmp=tmp, T=o.po.T, pen_unpaired=o.pe.pen_unpaired, no_pairing=o.pe.no_pairing, mask_level=float(o.co.mask_level),
                           ctg_off=list(CTG_OFF) if o.contigs else [0], alt=[int(x) for x in o.alt] if o.alt is not None else None, id0=int(o.po.id0))


# ---- the generator
def generate(name, bounds):
    """bounds = (low, high) of orientation 1 as the host will compute them (class l sits on them; see case())."""
    spec = CONFIGS[name]
    o = options(name)
    rng = np.random.default_rng(sum(name.encode()) + 77)
    a, T, pen = o.ep.a, o.po.T, o.pe.pen_unpaired
    S = lambda x: int(x) * a
    low, high = bounds
    below = T - 5
    pairs = []                                                        # (intent, hits of read 1, hits of read 2)

    def room(ctg, span=L, lo=300, hi=300):
        return int(rng.integers(CTG_OFF[ctg] + lo, CTG_OFF[ctg] + CONTIG_LENS[ctg] - span - hi))

    def locus(taken, span=L, ctgs=(0, 1, 2)):                         # a place far from the pair's other places
        while True:
            p = room(int(rng.choice(ctgs)), span, 600, 600)
            if all(abs(p - t) > 3000 + span for t in taken):
                taken.append(p)
                return p

    def ins():
        return int(rng.integers(240, 361))

    def fr(P, d, s1, s2):                                             # forward hit at P, its mate reverse at insert d
        return fwd(P, s1), rev(P + d - (L - 1), s2)

    def put(intent, f_hits, r_hits, flip=None):
        """f_hits: the hits of the read that lies forward in the class's picture; flip gives them to read 2."""
        f_hits, r_hits = list(f_hits), list(r_hits)
        rng.shuffle(f_hits); rng.shuffle(r_hits)
        if flip is None:
            flip = bool(rng.integers(0, 2))
        pairs.append((intent, r_hits, f_hits) if flip else (intent, f_hits, r_hits))

    for _ in range(1000):                                             # calibration
        x, y = fr(room(int(rng.integers(0, 3)), 700), max(60, int(round(rng.normal(300, 30)))), S(100), S(100))
        put("cal", [x], [y], flip=False)
    if spec.get("two"):
        for _ in range(150):                                          # read 1 reverse on the left, read 2 forward on the right: orientation 2
            Q = room(int(rng.integers(0, 3)), 1200)
            d = max(60, int(round(rng.normal(500, 40))))
            put("cal2", [rev(Q, S(100))], [fwd(Q + L - 1 + d, S(100))], flip=False)

    deltas = [2, 3, 5, 7, 8, 10, 14, 21]
    for _ in range(120):                                              # a
        n0, n1 = [(1, 2), (2, 1), (2, 2), (2, 3), (3, 2), (1, 3), (3, 1)][int(rng.integers(0, 7))]
        P = room(int(rng.integers(0, 2)), 1400, 600, 600); d = ins()
        fh = [fwd(P + 130 * i, S(100 - (0 if i == 0 else rng.choice(deltas)))) for i in range(n0)]
        rh = [rev(P + d - (L - 1) + 130 * j, S(100 - (0 if j == 0 else rng.choice(deltas)))) for j in range(n1)]
        put("a", fh, rh)
    for k in range(36):                                               # b, c
        for cls in "bc":
            t = []
            P1 = locus(t, 700, (0, 1)); P2 = locus(t, 700, (0, 1))
            d1 = ins(); d2 = d1 if cls == "c" else ins()
            s2 = (100, 100) if cls == "c" else (int(rng.integers(85, 95)), int(rng.integers(85, 95)))
            x1, y1 = fr(P1, d1, S(100), S(100)); x2, y2 = fr(P2, d2, S(s2[0]), S(s2[1]))
            put(cls, [x1, x2], [y1, y2])
    for k in range(40):                                               # d
        t = []
        P = locus(t, 700, (0, 1)); x, y = fr(P, ins(), S(95), S(100 if k & 1 else 96))
        fh, rh = [x, fwd(locus(t), S(100))], [y]
        if not k & 1:
            rh.append(rev(locus(t), S(100)))
        put("d", fh, rh)
    for k in range(36):                                               # e
        t = []
        P = locus(t, 700, (0, 1))
        da, dc = (pen + 4 + int(rng.integers(0, 4)), 0) if k & 1 else (pen // 2 + 3, pen - pen // 2 + 2)
        x, y = fr(P, ins(), S(100) - da, S(100) - dc)
        fh, rh = [x, fwd(locus(t), S(100))], [y]
        if dc:
            rh.append(fwd(locus(t), S(100)))
        put("e", fh, rh)
    for k in range(36):                                               # f
        t = []
        P = locus(t, 700, (0, 1)); d = ins()
        other = locus(t)
        half2 = rev(other, S(48), 50, 100) if k & 1 else rev(P + 40, S(48), 50, 100)         # (k even: the same place, the other strand)
        put("f", [fwd(P, S(50), 0, 50), half2], [rev(P + d - (L - 1), S(100))])
    for k in range(8):                                                # g
        X = int(rng.integers(1000, 25_000)); d = ins()
        put("g_ctg", [fwd(CTG_OFF[0] + X, S(100))], [rev(CTG_OFF[1] + X + d - (L - 1), S(100))])
        x, y = fr(room(0, 5000), 3000 + int(rng.integers(0, 1000)), S(100), S(100)); put("g_far", [x], [y])
        P = room(1, 700); put("g_ff", [fwd(P, S(100))], [fwd(P + ins(), S(100))])
        x, y = fr(room(0, 700), ins(), S(100), S(100)); put("g_none1", [x], [])
        put("g_none2", [], [])
        x, y = fr(room(0, 700), ins(), below, S(100)); put("g_lowT", [x], [y])
        t = []; x, y = fr(locus(t, 700, (0, 1)), ins(), below, S(100)); put("g_lowT2", [x, fwd(locus(t), below - 3)], [y, rev(locus(t), S(90))])
        t = []; put("g_lowT3", [fwd(locus(t), below)], [rev(locus(t), below - 1)])
    for k in range(34):                                               # h
        B = CTG_OFF[1] if (k & 1 or spec.get("alt")) else CTG_OFF[2]
        d = int(rng.integers(260, 341))
        P = B - int(rng.integers(L, d - (L - 1) + 1))                 # P + L <= B <= Q = P + d - (L - 1)
        x, y = fr(P, d, S(100), S(100)); put("h_cross", [x], [y])
        x, y = fr(P - 1000, d, S(100), S(100)); put("h_inside", [x], [y])
    for k in range(44):                                               # i
        d = ins()
        if k < 8:
            P = int(rng.integers(0, 100))
        elif k < 16:
            P = L_PAC - int(rng.integers(0, 100)) - d - 1             # the mate ends in the last 100 bp
        else:
            P = room(int(rng.integers(0, 3)), 700)
        x, y = fr(P, d, S(100), S(int(rng.integers(90, 101)))); put("i", [x], [y], flip=k % 4 != 3)
    lim = 64
    for k in range(36):                                               # j
        n = lim - 1 + k % 3
        n0 = [1, 32, n - 1, 20][(k // 3) % 4]
        P = room(0, 130 * 66 + 800, 600, 600); d = ins()
        fh = [fwd(P + 130 * i, S(int(rng.integers(40, 101)))) for i in range(n0)]
        rh = [rev(P + d - (L - 1) + 130 * j, S(int(rng.integers(40, 101)))) for j in range(n - n0)]
        put("j%d" % n, fh, rh)
    for k in range(32):                                               # l
        x, y = fr(room(int(rng.integers(0, 3)), 900), [low - 1, low, high, high + 1][k % 4], S(100), S(100)); put("l", [x], [y])
    if spec.get("alt"):
        # classes a, d, e, g again with a hit on the ALT sequence for one or both reads: better than the best hit of the primary assembly, worse, below T
        n_base = len(pairs)
        k = 0
        for intent, h0, h1 in pairs[:n_base]:
            if intent[0] not in "adeg" or intent == "g_none2":
                continue
            who = (k // 3) % 3                                          # read 1, read 2, both
            hh = [list(h0), list(h1)]
            for r in (0, 1):
                if who == r or who == 2:
                    best = max([h[0] for h in hh[r]], default=S(90))
                    sc = [best + 3 * a, best - 10 * a, below][k % 3]
                    hh[r].append(fwd(room(2, L, 600, 600), sc))
            pairs.append(("alt_" + intent, hh[0], hh[1])); k += 1
        for k in range(16):                                           # the hit of the primary assembly below T, the ALT hit above it: no candidate pair, the ALT hit is the mate's view
            t = []
            h0 = [fwd(locus(t, L, (0, 1)), below), fwd(room(2, L, 600, 600), S(90))]
            h1 = [rev(locus(t, L, (0, 1)), below if k & 1 else S(100))] + ([fwd(room(2, L, 600, 600), S(88))] if k & 1 else [])
            put("alt_lowT", h0, h1)
    while len(pairs) % 64 == 0:                                       # not a multiple of the kernel's block
        x, y = fr(room(0, 700), 300, S(100), S(100)); put("cal", [x], [y], flip=False)
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    n = 2 * len(pairs)
    rows, rpr = [], np.zeros(n, np.uint32)
    for p, (_, h0, h1) in enumerate(pairs):
        for r, hs in enumerate((h0, h1)):
            rpr[2 * p + r] = len(hs)
            for (sc, qb, qe, rb, re) in hs:
                rows.append([2 * p + r, sc, qb, qe, rb & 0xFFFFFFFF, rb >> 32, re & 0xFFFFFFFF, re >> 32])
    regs = np.array(rows, np.int64).astype(np.uint32).view(np.int32).reshape(-1, 8)
    frac = rng.choice(np.array([0.0, 0.3, 0.9], np.float32), size=n, p=[0.6, 0.2, 0.2]).astype(np.float32)
    reads = rng.integers(0, 4, size=(n, L)).astype(np.uint8)
    return SimpleNamespace(name=name, opt=o, intent=[p[0] for p in pairs], n_pairs=len(pairs), n_reads=n, regs=np.ascontiguousarray(regs), rpr=rpr, frac=frac, reads=reads)


def run_host(g):
    """bmh_finalize_pairs without the mate rescue on a generated set -> (fin [m, 16], per_read, h_rec, unflag, pes [4, 5])."""
    from bwamem_hip.lib import finalize_pairs
    o = g.opt
    return finalize_pairs(o.co, o.ep, o.po, L_PAC, pack_pac(genome()), g.reads.reshape(-1), np.arange(g.n_reads, dtype=np.uint64) * L, np.full(g.n_reads, L, np.uint32),
                          g.regs, g.rpr, g.frac, contigs=o.contigs, n_threads=2, pe=o.pe)


@functools.lru_cache(maxsize=None)
def case(name):
    """A configuration's regions, the host walk's records for them and the restatement's verdict on every pair; computed once.  Class l needs the insert
    bounds the host will compute: they depend on the quartiles of the calibration inserts alone (class l lies outside the preliminary bounds the mean is taken
    within), so a second generation with the bounds of the first run reproduces them -- asserted."""
    bounds = (152, 446)
    for _ in range(2):
        g = generate(name, bounds)
        fin, per_read, h_rec, unflag, pes = run_host(g)
        got = (int(pes[1, 0]), int(pes[1, 1]))
        if got == bounds:
            break
        bounds = got
    assert got == bounds, (got, bounds)
    off = np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64)
    po = plain_opt(g.opt)
    res = []
    for p in range(g.n_pairs):
        hits = [[hit_of(fin[k]) for k in range(off[2 * p + r], off[2 * p + r + 1])] for r in (0, 1)]
        res.append(restate_pair(hits, pes, po, p, g.frac[2 * p], g.frac[2 * p + 1]))
    g.fin, g.per_read, g.h_rec, g.unflag, g.pes, g.off, g.res, g.popt = fin, per_read, h_rec, unflag, pes, off, res, po
    g.labels = [labels_of(g, p) for p in range(g.n_pairs)]
    return g


# ---- the restatement
def hash64(k):
    k = (k + (~(k << 32) & M64)) & M64; k ^= k >> 22
    k = (k + (~(k << 13) & M64)) & M64; k ^= k >> 8
    k = (k + (k << 3)) & M64; k ^= k >> 15
    k = (k + (~(k << 27) & M64)) & M64; k ^= k >> 31
    return k


def hit_of(rec):
    r = [int(x) for x in rec]
    return SimpleNamespace(score=r[1], qb=r[2], qe=r[3], rb=(r[4] & 0xFFFFFFFF) | r[5] << 32, re=(r[6] & 0xFFFFFFFF) | r[7] << 32)


def rid_of(po, h):
    f = h.rb if h.rb < L_PAC else 2 * L_PAC - 1 - (h.re - 1)
    return max(i for i, s in enumerate(po.ctg_off) if f >= s)


def raw_mapq(diff, a):
    return int(6.02 * diff / a + .499)


def infer_dir(b1, b2):
    r1, r2 = b1 >= L_PAC, b2 >= L_PAC
    p2 = b2 if r1 == r2 else 2 * L_PAC - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def mem_pair(hits, n_pri, pes, po, pid):
    """pair_regs of csrc/pair_post.cpp -> (o, sub, n_sub, z, candidates); a candidate is (q, un-truncated score, orientation, distance)."""
    v = []
    for r in (0, 1):
        for i in range(n_pri[r]):
            e = hits[r][i]
            rv = e.rb >= L_PAC
            x = e.rb if not rv else 2 * L_PAC - 1 - e.rb
            x = e.rid << 32 | (x - (po.ctg_off[e.rid] if len(po.ctg_off) > 1 else 0))
            v.append((x, e.score << 32 | i << 2 | int(rv) << 1 | r))
    v.sort()
    y = [-1] * 4
    u, cands = [], []
    for i in range(len(v)):
        for r in (0, 1):
            d = r << 1 | (v[i][1] >> 1 & 1)
            if pes[d][2]:
                continue
            which = r << 1 | ((v[i][1] & 1) ^ 1)
            if y[which] < 0:
                continue
            for k in range(y[which], -1, -1):
                if (v[k][1] & 3) != which:
                    continue
                dist = v[i][0] - v[k][0]
                if dist > int(pes[d][1]):
                    break
                if dist < int(pes[d][0]):
                    continue
                ns = (dist - float(pes[d][3])) / float(pes[d][4])
                val = float((v[i][1] >> 32) + (v[k][1] >> 32)) + .721 * math.log(2. * math.erfc(abs(ns) * math.sqrt(0.5))) * po.a + .499
                q = max(int(val), 0)
                py = k << 32 | i
                u.append((q << 32 | (hash64(py ^ ((pid << 8) & M64)) & 0xFFFFFFFF), py))
                cands.append((q, val, d, dist))
        y[v[i][1] & 3] = i
    z = [0, 0]
    if not u:
        return 0, 0, 0, z, cands
    u.sort()
    i, k = u[-1][1] >> 32, u[-1][1] & 0xFFFFFFFF
    z[v[i][1] & 1] = (v[i][1] & 0xFFFFFFFF) >> 2
    z[v[k][1] & 1] = (v[k][1] & 0xFFFFFFFF) >> 2
    sub = u[-2][0] >> 32 if len(u) > 1 else 0
    n_sub = sum(1 for j in range(len(u) - 1) if sub - (u[j][0] >> 32) <= po.tmp)
    return u[-1][0] >> 32, sub, n_sub, z, cands


def restate_pair(hits, pes, po, p, fr0, fr1):
    """What sam_pe of csrc/pair_post.cpp decides for pair p from its reads' hits in record order (the hits of the primary assembly first)."""
    n_pri = [0, 0]
    for r in (0, 1):
        for e in hits[r]:
            e.rid = rid_of(po, e)
            e.alt = bool(po.alt and po.alt[e.rid])
        n_pri[r] = sum(not e.alt for e in hits[r])
        assert all(not e.alt for e in hits[r][:n_pri[r]])
        prim = []                                                     # `secondary` among the hits of the primary assembly (mem_mark_primary_se's overlap test)
        for i in range(n_pri[r]):
            e = hits[r][i]; e.secondary = -1
            for j in prim:
                f = hits[r][j]
                b_max, e_min = max(e.qb, f.qb), min(e.qe, f.qe)
                if e_min > b_max and e_min - b_max >= min(e.qe - e.qb, f.qe - f.qb) * po.mask_level:
                    e.secondary = j
                    break
            if e.secondary < 0:
                prim.append(i)
    R = SimpleNamespace(paired=False, proper=False, o=0, subo=0, n_sub=0, z=[0, 0], q_pe=None, cands=[], is_multi=False, n_pri=n_pri, n=[len(hits[0]), len(hits[1])], score_un=None, zsel=[0, 0], hits=hits)
    pid = po.id0 // 2 + p
    if not po.no_pairing and n_pri[0] and n_pri[1]:
        R.o, R.subo, R.n_sub, R.zsel, R.cands = mem_pair(hits, n_pri, pes, po, pid)
        if R.o > 0:
            R.is_multi = any(hits[r][j].secondary < 0 and hits[r][j].score >= po.T for r in (0, 1) for j in range(1, n_pri[r]))
            if not R.is_multi:
                R.paired = True
                R.score_un = hits[0][0].score + hits[1][0].score - po.pen_unpaired
                subo = max(R.subo, R.score_un)
                q_pe = raw_mapq(R.o - subo, po.a)
                if R.n_sub > 0:
                    q_pe -= int(4.343 * math.log(R.n_sub + 1) + .499)
                q_pe = min(max(q_pe, 0), 60)
                R.q_pe = int(q_pe * (1. - .5 * float(np.float32(fr0) + np.float32(fr1))) + .499)
                R.proper = R.o > R.score_un
                R.z = list(R.zsel) if R.proper else [0, 0]
    if not R.paired:
        hh = []
        for r in (0, 1):
            h = -1
            if hits[r]:
                if hits[r][0].score >= po.T:
                    h = 0
                elif n_pri[r] < len(hits[r]) and hits[r][n_pri[r]].score >= po.T:
                    h = n_pri[r]
            hh.append(h)
        R.z = hh
        if not po.no_pairing and hh[0] >= 0 and hh[1] >= 0 and hits[0][hh[0]].rid == hits[1][hh[1]].rid:
            d, dist = infer_dir(hits[0][0].rb, hits[1][0].rb)
            R.proper = bool(not pes[d][2] and int(pes[d][0]) <= dist <= int(pes[d][1]))
    return R


def labels_of(g, p):
    """The branches pair p really took (by the restatement), as class names."""
    R, intent, po = g.res[p], g.intent[p], g.popt
    low, high = int(g.pes[1, 0]), int(g.pes[1, 1])
    nc = len(R.cands)
    out = set()
    if R.paired and 2 <= nc <= 6 and intent in ("a", "alt_a"):
        out.add("a")
    if R.paired and nc == 2:
        qs = sorted(c[0] for c in R.cands)
        out.add("c" if qs[0] == qs[1] and R.cands[0][3] == R.cands[1][3] else "b")
    if R.paired and R.proper and max(R.z) > 0:
        out.add("d")
        if min(R.z) > 0:
            out.add("d_both")
    if R.paired and not R.proper:
        out.add("e")
    if R.o > 0 and R.is_multi:
        out.add("f")
    if R.paired and R.proper and any(R.hits[r][R.z[r]].score < po.T for r in (0, 1)):
        out.add("lowT_chosen")                                        # mem_pair does not look at T: the chosen hit is written whatever its score
    if not R.paired and nc == 0:
        out.add("g")
        if intent.startswith("g_") or intent.startswith("alt_g_"):
            out.add(intent[4:] if intent.startswith("alt_") else intent)
    if not R.paired and R.proper:
        out.add("g_position")                                         # 0x2 from the position test of the first hits
    if intent == "h_cross" and nc == 0 and len(po.ctg_off) > 1:
        out.add("h")
    if intent == "h_inside" and R.paired and R.proper:
        out.add("h_inside")
    if intent == "i" and R.paired and R.proper:
        out.add("i" if R.hits[0][R.z[0]].rb >= L_PAC else "i_fwd")
    if sum(R.n) in (63, 64, 65):
        out.add("j%d" % sum(R.n))
    if g.frac[2 * p] > 0 or g.frac[2 * p + 1] > 0:
        out.add("k")
    if nc <= 1 and intent == "l":
        out.add("l_in" if nc else "l_out")
    if R.paired and R.n_sub >= 1:
        out.add("n_sub%d" % min(R.n_sub, 3))
        qs = sorted((c[0] for c in R.cands), reverse=True)
        if any(qs[1] - q == po.tmp for q in qs[2:]):
            out.add("sub_edge_in")                                    # a runner-up exactly mark_tmp below the second best
        if any(qs[1] - q == po.tmp + 1 for q in qs[2:]):
            out.add("sub_edge_out")
    if R.n[0] > R.n_pri[0] or R.n[1] > R.n_pri[1]:
        out.add("alt_hit")
    return out


def class_counts(g):
    cnt = {}
    for s in g.labels:
        for k in s:
            cnt[k] = cnt.get(k, 0) + 1
    return dict(sorted(cnt.items()))


def dump_case(g, path):
    """The case file of tests/pair_post_host.cpp (see there)."""
    o = g.opt
    nc = len(o.contigs) if o.contigs else 1
    hd = np.array([g.n_reads, len(g.regs), nc, L, int(o.alt is not None), C.sizeof(o.co), C.sizeof(o.ep), C.sizeof(o.po), C.sizeof(o.pe)], np.int32)
    pac = pack_pac(genome())
    pac = np.concatenate([pac, np.zeros(L_PAC // 4 + 2 - len(pac), np.uint8)])
    with open(path, "wb") as f:
        for part in (hd, bytes(o.co), bytes(o.ep), bytes(o.po), bytes(o.pe), o.alt if o.alt is not None else np.zeros(nc, np.uint8),
                     np.array(CTG_OFF[:nc], np.int64), np.array(CONTIG_LENS if nc > 1 else [L_PAC], np.int32), np.array([L_PAC], np.int64), pac, g.reads, g.regs,
                     g.rpr.astype(np.uint32), g.frac.astype(np.float32)):
            f.write(part if isinstance(part, bytes) else np.ascontiguousarray(part).tobytes())


def load_result(path, n_reads):
    raw = open(path, "rb").read()
    m = int(np.frombuffer(raw, np.int64, 1)[0]); at = 8
    fin = np.frombuffer(raw, np.int32, 16 * m, at).reshape(m, 16); at += 64 * m
    opr = np.frombuffer(raw, np.uint32, n_reads, at); at += 4 * n_reads
    h = np.frombuffer(raw, np.int32, n_reads, at); at += 4 * n_reads
    uf = np.frombuffer(raw, np.int32, n_reads, at); at += 4 * n_reads
    pes = np.frombuffer(raw, np.float64, 20, at).reshape(4, 5)
    assert at + 160 == len(raw)
    return fin, opr, h, uf, pes
